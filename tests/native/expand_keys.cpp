// expand_keys.cpp -- AffineHessianDetector::expandQuery through hesaff_amd/csrc/hesaff.hpp: detect on the given images with a
// vocabulary set, export every image's words file, read the whole rows back, verify the images after the first against the first
// and expand the first with the verified ones (tests/test_query_expansion_host.py compiles it; tests/test_query_expansion.py runs it).
//
//   expand_keys <vocabulary file> <tolerance> <min inliers> <directory for the words files> <x0> <y0> <x1> <y1> <query image> <image> [<image> ...]
//
// Prints   N <rows of the expanded query>, per candidate   I <candidate> <rank> <live> <kept> <written>,   H <FNV-1a of the expanded
// rows' bytes>, W <the sum of the words>, B <the bounding box of the query's live rows> and then
//   C <a call with min inliers 0: refused>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../hesaff_amd/csrc/hesaff.hpp"

using namespace hesaff_amd;

int main(int argc, char **argv)
{
   if (argc < 11) {
      fprintf(stderr, "usage: expand_keys <vocabulary file> <tolerance> <min inliers> <directory> <x0> <y0> <x1> <y1> <query image> <image> [<image> ...]\n");
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
      for (int a = 9; a < argc; a++) {
         uint8_t *data = nullptr;
         int w = 0, h = 0, ch = 0;
         if (hesaff_read_image(argv[a], &data, &w, &h, &ch) != HESAFF_OK) {
            fprintf(stderr, "cannot read %s\n", argv[a]);
            return 1;
         }
         det.detectPyramidKeypoints(data, w, h, ch);
         hesaff_free(data);
         const std::string path = std::string(argv[4]) + "/" + std::to_string(a - 9) + ".hesaff.words";
         det.exportWords(path);
         void *p = nullptr;
         int n = 0, vs = 0;
         if (hesaff_read_words_rows(path.c_str(), &p, &n, &vs) != HESAFF_OK || vs != k || n != (int)det.keys.size()) {
            fprintf(stderr, "cannot read %s back\n", path.c_str());
            return 1;
         }
         std::vector<char> &to = a == 9 ? query : rows;
         to.insert(to.end(), (const char *)p, (const char *)p + (size_t)n * 24);
         hesaff_free(p);
         if (a > 9) counts.push_back(n);
      }
      const int nq = (int)(query.size() / 24);
      std::vector<AffineHessianDetector::Verified> res;
      det.verifyMatches(query.data(), nq, counts, rows.data(), k, (float)atof(argv[2]), 1, &res);
      const float roi[4] = {(float)atof(argv[5]), (float)atof(argv[6]), (float)atof(argv[7]), (float)atof(argv[8])};
      std::vector<int32_t> words;
      std::vector<AffineHessianDetector::Expanded> info;
      const std::vector<char> out = det.expandQuery(query.data(), nq, counts, rows.data(), res, k, atoi(argv[3]), roi, 1024, 1 << 18, &words, &info);
      printf("N %zu\n", out.size() / 24);
      for (size_t r = 0; r < info.size(); r++) printf("I %zu %d %d %d %d\n", r, info[r].rank, info[r].liveKeys, info[r].keptKeys, info[r].writtenKeys);
      unsigned long long hash = 1469598103934665603ull, sum = 0;
      for (char c : out) hash = (hash ^ (unsigned char)c) * 1099511628211ull;
      for (int32_t w : words) sum += (unsigned long long)w;
      printf("H %llu\nW %llu\n", hash, sum);
      float box[4];
      AffineHessianDetector::liveBounds(query.data(), nq, box);
      printf("B %.9g %.9g %.9g %.9g\n", (double)box[0], (double)box[1], (double)box[2], (double)box[3]);
      bool refused = false;
      try { det.expandQuery(query.data(), nq, counts, rows.data(), res, k, 0, roi); }
      catch (const std::invalid_argument &) { refused = true; }
      printf("C %s\n", refused ? "refused" : "answered");
   } catch (const std::exception &e) {
      fprintf(stderr, "expand_keys: %s\n", e.what());
      return 1;
   }
   return 0;
}
