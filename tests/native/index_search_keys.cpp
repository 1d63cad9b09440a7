// index_search_keys.cpp -- AffineHessianDetector::buildIndex / queryIndex / clearIndex through hesaff_amd/csrc/hesaff.hpp: detect on
// the given images with a vocabulary set, build the index from the detector's own (word, dist2) rows, and query it with the words
// of the first image (tests/test_image_index_host.py compiles it; tests/test_image_index.py runs it).
//
//   index_search_keys <vocabulary file> <top> <image> [<image> ...]
//
// Prints per result   R <rank> <image index> <score as %.17g>   and then   C <results of a query after clearIndex: refused>
#include <cstdio>
#include <cstdlib>

#include "../../hesaff_amd/csrc/hesaff.hpp"

using namespace hesaff_amd;

int main(int argc, char **argv)
{
   if (argc < 4) {
      fprintf(stderr, "usage: index_search_keys <vocabulary file> <top> <image> [<image> ...]\n");
      return 2;
   }
   try {
      uint8_t *rows = nullptr;
      int k = 0;
      if (hesaff_read_vocabulary(argv[1], &rows, &k) != HESAFF_OK) {
         fprintf(stderr, "cannot read %s\n", argv[1]);
         return 1;
      }
      AffineHessianDetector det;
      det.setVocabulary(rows, k);
      hesaff_free(rows);
      std::vector<int32_t> counts, words, first;
      for (int a = 3; a < argc; a++) {
         uint8_t *data = nullptr;
         int w = 0, h = 0, ch = 0;
         if (hesaff_read_image(argv[a], &data, &w, &h, &ch) != HESAFF_OK) {
            fprintf(stderr, "cannot read %s\n", argv[a]);
            return 1;
         }
         det.detectPyramidKeypoints(data, w, h, ch);
         hesaff_free(data);
         const size_t n = det.keys.size();
         counts.push_back((int32_t)n);
         if (n) words.insert(words.end(), det.words(), det.words() + 2 * n);
         if (a == 3 && n) first.assign(det.words(), det.words() + 2 * n);
      }
      det.buildIndex(counts, words.data(), 2, k);
      const std::vector<std::pair<int32_t, double>> res = det.queryIndex(first.data(), (int)(first.size() / 2), 2, atoi(argv[2]));
      for (size_t r = 0; r < res.size(); r++) printf("R %zu %d %.17g\n", r + 1, res[r].first, res[r].second);
      det.clearIndex();
      bool refused = false;
      try { det.queryIndex(first.data(), (int)(first.size() / 2), 2, 1); }
      catch (const std::invalid_argument &) { refused = true; }
      printf("C %s\n", refused ? "refused" : "answered");
   } catch (const std::exception &e) {
      fprintf(stderr, "index_search_keys: %s\n", e.what());
      return 1;
   }
   return 0;
}
