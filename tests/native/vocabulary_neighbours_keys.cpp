// vocabulary_neighbours_keys.cpp -- AffineHessianDetector::setVocabularyNeighbours, vocabularyNeighbours(), neighbours() and the
// expanded exportWords through hesaff_amd/csrc/hesaff.hpp (tests/test_vocabulary_neighbours.py builds and runs it; the host suite
// compiles it).
//
//   vocabulary_neighbours_keys <vocabulary file> <image> <words file to write> <R>
//
// Prints what the detector holds afterwards:
//   N <keys.size()> <neighboursRanks()> <1 when words() is rank 0 of neighbours() for every key, else 0>
//   B <word> <dist2> ... (R pairs)            per key
//   refused cells / refused 0 / refused 9     a cell layer beside R > 1, and the counts outside 1..8, throw
//   R <vocabularyNeighbours()>                the setting after the refusals
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../hesaff_amd/csrc/hesaff.hpp"

using namespace hesaff_amd;

int main(int argc, char **argv)
{
   if (argc != 5) {
      fprintf(stderr, "usage: vocabulary_neighbours_keys <vocabulary file> <image> <words file> <R>\n");
      return 2;
   }
   try {
      uint8_t *vocab = nullptr;
      int k = 0;
      if (hesaff_read_vocabulary(argv[1], &vocab, &k) != HESAFF_OK) {
         fprintf(stderr, "cannot read %s\n", argv[1]);
         return 1;
      }
      AffineHessianDetector det;
      if (det.vocabularyNeighbours() != 1 || det.neighbours() != nullptr) return 3;
      det.setVocabulary(vocab, k);
      det.setVocabularyNeighbours(atoi(argv[4]));
      uint8_t *data = nullptr;
      int w = 0, h = 0, ch = 0;
      if (hesaff_read_image(argv[2], &data, &w, &h, &ch) != HESAFF_OK) {
         fprintf(stderr, "cannot read %s\n", argv[2]);
         return 1;
      }
      det.detectPyramidKeypoints(data, w, h, ch);
      hesaff_free(data);
      const int32_t *nb = det.neighbours(), *words = det.words();
      const size_t R = (size_t)det.neighboursRanks();
      bool rank0 = nb != nullptr && words != nullptr;
      for (size_t i = 0; rank0 && i < det.keys.size(); i++) rank0 = nb[i * R * 2] == words[2 * i] && nb[i * R * 2 + 1] == words[2 * i + 1];
      printf("N %zu %zu %d\n", det.keys.size(), R, rank0 ? 1 : 0);
      for (size_t i = 0; i < det.keys.size(); i++) {
         printf("B");
         for (size_t j = 0; j < 2 * R; j++) printf(" %d", nb[i * R * 2 + j]);
         printf("\n");
      }
      det.exportWords(argv[3]);
      const uint32_t first[2] = {0, (uint32_t)k};
      try { det.setVocabularyCells(vocab, first, 1); } catch (const std::invalid_argument &) { printf("refused cells\n"); }
      try { det.setVocabularyNeighbours(0); } catch (const std::invalid_argument &) { printf("refused 0\n"); }
      try { det.setVocabularyNeighbours(9); } catch (const std::invalid_argument &) { printf("refused 9\n"); }
      printf("R %d\n", det.vocabularyNeighbours());
      hesaff_free(vocab);
   } catch (const std::exception &e) {
      fprintf(stderr, "vocabulary_neighbours_keys: %s\n", e.what());
      return 1;
   }
   return 0;
}
