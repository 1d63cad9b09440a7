// index_growth_members.cpp -- AffineHessianDetector::addToIndex / saveIndex / loadIndex through hesaff_amd/csrc/hesaff.hpp: detect on
// the given images with a vocabulary set, build the index from all but the last, add the last, save, load into a second detector,
// and query both with the words of the last image (tests/test_index_growth.py compiles and runs it).
//
//   index_growth_members <vocabulary file> <index file to write> <image> <image> [<image> ...]
//
// Prints per result of the grown index   A <rank> <image index> <score as %.17g>   of the loaded one   L <rank> ...   and then
// P <an addToIndex on a detector without an index: refused>
#include <cstdio>
#include <cstdlib>

#include "../../hesaff_amd/csrc/hesaff.hpp"

using namespace hesaff_amd;

int main(int argc, char **argv)
{
   if (argc < 5) {
      fprintf(stderr, "usage: index_growth_members <vocabulary file> <index file> <image> <image> [<image> ...]\n");
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
      std::vector<int32_t> counts, words, last;
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
         if (a + 1 < argc) {
            counts.push_back((int32_t)n);
            if (n) words.insert(words.end(), det.words(), det.words() + 2 * n);
         } else if (n) last.assign(det.words(), det.words() + 2 * n);
      }
      const int n_last = (int)(last.size() / 2);
      det.buildIndex(counts, words.data(), 2, k);
      det.addToIndex(std::vector<int32_t>(1, n_last), last.data(), 2);
      const int top = (int)counts.size() + 1;
      std::vector<std::pair<int32_t, double>> res = det.queryIndex(last.data(), n_last, 2, top);
      for (size_t r = 0; r < res.size(); r++) printf("A %zu %d %.17g\n", r + 1, res[r].first, res[r].second);
      det.saveIndex(argv[2]);
      AffineHessianDetector other;
      other.loadIndex(argv[2]);
      res = other.queryIndex(last.data(), n_last, 2, top);
      for (size_t r = 0; r < res.size(); r++) printf("L %zu %d %.17g\n", r + 1, res[r].first, res[r].second);
      AffineHessianDetector plain;
      bool refused = false;
      try { plain.addToIndex(std::vector<int32_t>(1, n_last), last.data(), 2); }
      catch (const std::invalid_argument &) { refused = true; }
      printf("P %s\n", refused ? "refused" : "added");
   } catch (const std::exception &e) {
      fprintf(stderr, "index_growth_members: %s\n", e.what());
      return 1;
   }
   return 0;
}
