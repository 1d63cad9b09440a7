// verify_keys.cpp -- AffineHessianDetector::verifyMatches through hesaff_amd/csrc/hesaff.hpp: detect on the given images with a
// vocabulary set, export every image's words file, read the whole rows back (hesaff_read_words_rows) and verify the images after the
// first against the first (tests/test_verify_host.py compiles it; tests/test_verify.py runs it).
//
//   verify_keys <vocabulary file> <tolerance> <pairs> <directory for the words files> <query image> <image> [<image> ...]
//
// Prints per candidate, in verified order   V <rank> <candidate> <inliers> <used> <found> <inert keys>   and then
//   C <a call with 0 pairs: refused>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../hesaff_amd/csrc/hesaff.hpp"

using namespace hesaff_amd;

int main(int argc, char **argv)
{
   if (argc < 7) {
      fprintf(stderr, "usage: verify_keys <vocabulary file> <tolerance> <pairs> <directory> <query image> <image> [<image> ...]\n");
      return 2;
   }
   try {
      uint8_t *vocabulary = nullptr;
      int k = 0;
      if (hesaff_read_vocabulary(argv[1], &vocabulary, &k) != HESAFF_OK) {
         fprintf(stderr, "cannot read %s\n", argv[1]);
         return 1;
      }
      AffineHessianDetector det;
      det.setVocabulary(vocabulary, k);
      hesaff_free(vocabulary);
      std::vector<char> query, rows;
      std::vector<int32_t> counts;
      for (int a = 5; a < argc; a++) {
         uint8_t *data = nullptr;
         int w = 0, h = 0, ch = 0;
         if (hesaff_read_image(argv[a], &data, &w, &h, &ch) != HESAFF_OK) {
            fprintf(stderr, "cannot read %s\n", argv[a]);
            return 1;
         }
         det.detectPyramidKeypoints(data, w, h, ch);
         hesaff_free(data);
         const std::string path = std::string(argv[4]) + "/" + std::to_string(a - 5) + ".hesaff.words";
         det.exportWords(path);
         void *p = nullptr;
         int n = 0, vs = 0;
         if (hesaff_read_words_rows(path.c_str(), &p, &n, &vs) != HESAFF_OK || vs != k || n != (int)det.keys.size()) {
            fprintf(stderr, "cannot read %s back\n", path.c_str());
            return 1;
         }
         std::vector<char> &to = a == 5 ? query : rows;
         to.insert(to.end(), (const char *)p, (const char *)p + (size_t)n * 24);
         hesaff_free(p);
         if (a > 5) counts.push_back(n);
      }
      std::vector<AffineHessianDetector::Verified> res;
      const std::vector<int32_t> order = det.verifyMatches(query.data(), (int)(query.size() / 24), counts, rows.data(), k, (float)atof(argv[2]), atoi(argv[3]), &res);
      for (size_t r = 0; r < order.size(); r++) {
         const AffineHessianDetector::Verified &v = res[(size_t)order[r]];
         printf("V %zu %d %d %d %d %d\n", r + 1, order[r], v.inliers, v.used, v.found, v.inertKeys);
      }
      bool refused = false;
      try { det.verifyMatches(query.data(), (int)(query.size() / 24), counts, rows.data(), k, 1.0f, 0); }
      catch (const std::invalid_argument &) { refused = true; }
      printf("C %s\n", refused ? "refused" : "answered");
   } catch (const std::exception &e) {
      fprintf(stderr, "verify_keys: %s\n", e.what());
      return 1;
   }
   return 0;
}
