// embedding_search_keys.cpp -- AffineHessianDetector::setEmbedding / signatures / trainEmbedding / embeddingProjection and the
// buildIndex / queryIndex overloads with signatures through hesaff_amd/csrc/hesaff.hpp: detect on the given images with a vocabulary
// set, train the thresholds on the detector's own descriptors and words, install them, detect again, build the embedded index from
// the detector's words and signatures, and query it with the first image's at a Hamming threshold (tests/test_embedding.py runs it).
//
//   embedding_search_keys <vocabulary file> <seed> <hamming> <top> <image> [<image> ...]
//
// Prints   T <FNV-1a of the trained thresholds' bytes>, per image   S <image index> <keys> <FNV-1a of its signatures' bytes>,
// per result   R <rank> <image index> <score as %.17g>   and then   P <a plain buildIndex followed by the embedded query: refused>
#include <cstdio>
#include <cstdlib>

#include "../../hesaff_amd/csrc/hesaff.hpp"

using namespace hesaff_amd;

static unsigned long long fnv(const void *p, size_t n)
{
   unsigned long long h = 0xcbf29ce484222325ull;
   for (size_t i = 0; i < n; i++) h = (h ^ ((const unsigned char *)p)[i]) * 0x100000001b3ull;
   return h;
}

int main(int argc, char **argv)
{
   if (argc < 6) {
      fprintf(stderr, "usage: embedding_search_keys <vocabulary file> <seed> <hamming> <top> <image> [<image> ...]\n");
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
      const std::vector<int8_t> P = AffineHessianDetector::embeddingProjection(strtoull(argv[2], nullptr, 10));
      std::vector<uint8_t> desc;
      std::vector<int32_t> words;
      auto detect = [&](const char *path) {
         uint8_t *data = nullptr;
         int w = 0, h = 0, ch = 0;
         if (hesaff_read_image(path, &data, &w, &h, &ch) != HESAFF_OK) throw std::runtime_error(std::string("cannot read ") + path);
         det.detectPyramidKeypoints(data, w, h, ch);
         hesaff_free(data);
      };
      for (int a = 5; a < argc; a++) {
         detect(argv[a]);
         if (det.signatures()) throw std::runtime_error("signatures without an embedding");
         const size_t n = det.keys.size();
         for (size_t i = 0; i < n; i++) desc.insert(desc.end(), det.keys[i].desc, det.keys[i].desc + 128);
         if (n) words.insert(words.end(), det.words(), det.words() + 2 * n);
      }
      const std::vector<int32_t> tau = det.trainEmbedding(desc.data(), words.data(), 2, (int)(desc.size() / 128), k, P.data());
      printf("T %llu\n", fnv(tau.data(), tau.size() * 4));
      det.setEmbedding(P.data(), tau.data());
      std::vector<int32_t> counts, first_words;
      std::vector<uint64_t> sigs, first_sigs;
      words.clear();
      for (int a = 5; a < argc; a++) {
         detect(argv[a]);
         const size_t n = det.keys.size();
         counts.push_back((int32_t)n);
         if (n) { words.insert(words.end(), det.words(), det.words() + 2 * n); sigs.insert(sigs.end(), det.signatures(), det.signatures() + n); }
         if (a == 5 && n) { first_words.assign(det.words(), det.words() + 2 * n); first_sigs.assign(det.signatures(), det.signatures() + n); }
         printf("S %d %zu %llu\n", a - 5, n, fnv(det.signatures(), n * 8));
      }
      det.buildIndex(counts, words.data(), 2, sigs.data(), k);
      const int nq = (int)first_sigs.size();
      const std::vector<std::pair<int32_t, double>> res = det.queryIndex(first_words.data(), nq, 2, first_sigs.data(), atoi(argv[3]), atoi(argv[4]));
      for (size_t r = 0; r < res.size(); r++) printf("R %zu %d %.17g\n", r + 1, res[r].first, res[r].second);
      det.buildIndex(counts, words.data(), 2, k);
      bool refused = false;
      try { det.queryIndex(first_words.data(), nq, 2, first_sigs.data(), atoi(argv[3]), 1); }
      catch (const std::invalid_argument &) { refused = true; }
      printf("P %s\n", refused ? "refused" : "answered");
      det.setEmbedding(nullptr, nullptr);
   } catch (const std::exception &e) {
      fprintf(stderr, "embedding_search_keys: %s\n", e.what());
      return 1;
   }
   return 0;
}
