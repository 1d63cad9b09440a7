// index_remove_members.cpp -- AffineHessianDetector::removeFromIndex through hesaff_amd/csrc/hesaff.hpp: detect on the given images
// with a vocabulary set, build the index from all of them, remove the image with the given number, and query with the words of the
// last image (tests/test_index_remove.py compiles and runs it).
//
//   index_remove_members <vocabulary file> <number of the image to remove> <image> <image> [<image> ...]
//
// Prints   M <old number> <new number>   per image, per result of the query   R <rank> <image index> <score as %.17g>   and then
// T <a number given twice: refused>   A <every image: refused>   P <a removal on a detector without an index: refused>
#include <cstdio>
#include <cstdlib>

#include "../../hesaff_amd/csrc/hesaff.hpp"

using namespace hesaff_amd;

static const char *refused(AffineHessianDetector &det, const std::vector<int> &images)
{
   try { det.removeFromIndex(images); }
   catch (const std::invalid_argument &) { return "refused"; }
   return "removed";
}

int main(int argc, char **argv)
{
   if (argc < 5) {
      fprintf(stderr, "usage: index_remove_members <vocabulary file> <number to remove> <image> <image> [<image> ...]\n");
      return 2;
   }
   try {
      uint8_t *rows = nullptr;
      int k = 0;
      if (hesaff_read_vocabulary(argv[1], &rows, &k) != HESAFF_OK) {
         fprintf(stderr, "cannot read %s\n", argv[1]);
         return 1;
      }
      const int gone = atoi(argv[2]);
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
         counts.push_back((int32_t)n);
         if (n) words.insert(words.end(), det.words(), det.words() + 2 * n);
         if (a + 1 == argc && n) last.assign(det.words(), det.words() + 2 * n);
      }
      const int n_last = (int)(last.size() / 2);
      det.buildIndex(counts, words.data(), 2, k);
      const char *twice = refused(det, std::vector<int>(2, gone));
      std::vector<int> all;
      for (size_t i = 0; i < counts.size(); i++) all.push_back((int)i);
      const char *every = refused(det, all);
      const std::vector<int32_t> remap = det.removeFromIndex(std::vector<int>(1, gone));
      for (size_t i = 0; i < remap.size(); i++) printf("M %zu %d\n", i, remap[i]);
      std::vector<std::pair<int32_t, double>> res = det.queryIndex(last.data(), n_last, 2, (int)counts.size());
      for (size_t r = 0; r < res.size(); r++) printf("R %zu %d %.17g\n", r + 1, res[r].first, res[r].second);
      AffineHessianDetector plain;
      printf("T %s\nA %s\nP %s\n", twice, every, refused(plain, std::vector<int>(1, 0)));
   } catch (const std::exception &e) {
      fprintf(stderr, "index_remove_members: %s\n", e.what());
      return 1;
   }
   return 0;
}
