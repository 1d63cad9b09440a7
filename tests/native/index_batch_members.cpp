// index_batch_members.cpp -- AffineHessianDetector::queryIndexBatch (both overloads), setIndexBatchBudget and indexBatchBudget through
// hesaff_amd/csrc/hesaff.hpp: detect on the given images with a vocabulary set, build the index from the detector's own (word, dist2)
// rows, and ask every image as one query of ONE batch (tests/test_index_batch_host.py compiles it; tests/test_index_batch.py runs it).
//
//   index_batch_members <vocabulary file> <top> <image> [<image> ...]
//
// Prints per query and result   B <query> <rank> <image index> <score as %.17g>,   then   S <the batch, at the default budget and at a
// budget of one byte, against queryIndex per query: equal>,   E <the same for the overload with signatures, on an index built with
// signatures: equal>   and   C <a batch after clearIndex: refused>
#include <cstdio>
#include <cstdlib>

#include "../../hesaff_amd/csrc/hesaff.hpp"

using namespace hesaff_amd;

typedef std::vector<std::pair<int32_t, double>> Ranked;

int main(int argc, char **argv)
{
   if (argc < 4) {
      fprintf(stderr, "usage: index_batch_members <vocabulary file> <top> <image> [<image> ...]\n");
      return 2;
   }
   try {
      uint8_t *rows = nullptr;
      int k = 0;
      if (hesaff_read_vocabulary(argv[1], &rows, &k) != HESAFF_OK) {
         fprintf(stderr, "cannot read %s\n", argv[1]);
         return 1;
      }
      const int top = atoi(argv[2]);
      AffineHessianDetector det;
      det.setVocabulary(rows, k);
      hesaff_free(rows);
      std::vector<int32_t> counts, words;
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
      }
      // a signature per key: its number, spread over the 64 bits (any values serve: the index takes them as given)
      std::vector<uint64_t> sigs(words.size() / 2);
      for (size_t j = 0; j < sigs.size(); j++) sigs[j] = (uint64_t)(j % 7) * 0x0101010101010101ull;
      det.buildIndex(counts, words.data(), 2, k);
      const size_t default_budget = det.indexBatchBudget();
      const std::vector<Ranked> batch = det.queryIndexBatch(counts, words.data(), 2, top);
      for (size_t q = 0; q < batch.size(); q++)
         for (size_t r = 0; r < batch[q].size(); r++) printf("B %zu %zu %d %.17g\n", q, r + 1, batch[q][r].first, batch[q][r].second);
      det.setIndexBatchBudget(1);
      bool same = det.indexBatchBudget() == 1 && det.queryIndexBatch(counts, words.data(), 2, top) == batch;
      det.setIndexBatchBudget(0);
      same = same && det.indexBatchBudget() == default_budget && batch.size() == counts.size();
      size_t at = 0;
      for (size_t q = 0; q < counts.size(); q++) {
         same = same && det.queryIndex(words.data() + 2 * at, counts[q], 2, top) == batch[q];
         at += (size_t)counts[q];
      }
      printf("S %s\n", same ? "equal" : "different");
      det.buildIndex(counts, words.data(), 2, sigs.data(), k);
      const std::vector<Ranked> embedded = det.queryIndexBatch(counts, words.data(), 2, sigs.data(), 20, top);
      same = embedded.size() == counts.size();
      at = 0;
      for (size_t q = 0; q < counts.size(); q++) {
         same = same && det.queryIndex(words.data() + 2 * at, counts[q], 2, sigs.data() + at, 20, top) == embedded[q];
         at += (size_t)counts[q];
      }
      printf("E %s\n", same ? "equal" : "different");
      det.clearIndex();
      bool refused = false;
      try { det.queryIndexBatch(counts, words.data(), 2, top); }
      catch (const std::invalid_argument &) { refused = true; }
      printf("C %s\n", refused ? "refused" : "answered");
   } catch (const std::exception &e) {
      fprintf(stderr, "index_batch_members: %s\n", e.what());
      return 1;
   }
   return 0;
}
