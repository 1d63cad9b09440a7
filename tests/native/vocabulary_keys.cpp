// vocabulary_keys.cpp -- AffineHessianDetector::setVocabulary, words() and exportWords through hesaff_amd/csrc/hesaff.hpp
// (tests/test_vocabulary.py builds and runs it).
//
//   vocabulary_keys <vocabulary file> <image> <words file to write>
//
// Prints what the detector holds afterwards, every key's (word, dist2) row beside the hex of the key's bytes:
//   N <g_numberOfPoints> <keys.size()> <1 when words() is non-null, else 0>
//   W <word> <dist2> <328 hex digits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../hesaff_amd/csrc/hesaff.hpp"

using namespace hesaff_amd;

int main(int argc, char **argv)
{
   if (argc != 4) {
      fprintf(stderr, "usage: vocabulary_keys <vocabulary file> <image> <words file>\n");
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
      if (det.words() != nullptr) return 3;
      det.setVocabulary(vocab, k);
      hesaff_free(vocab);   // (copied)
      uint8_t *data = nullptr;
      int w = 0, h = 0, ch = 0;
      if (hesaff_read_image(argv[2], &data, &w, &h, &ch) != HESAFF_OK) {
         fprintf(stderr, "cannot read %s\n", argv[2]);
         return 1;
      }
      det.detectPyramidKeypoints(data, w, h, ch);
      hesaff_free(data);
      const int32_t *words = det.words();
      printf("N %d %zu %d\n", det.g_numberOfPoints, det.keys.size(), words ? 1 : 0);
      for (size_t i = 0; i < det.keys.size(); i++) {
         unsigned char b[164];
         memcpy(b, &det.keys[i], sizeof b);
         printf("W %d %d ", words[2 * i], words[2 * i + 1]);
         for (unsigned char v : b) printf("%02x", v);
         printf("\n");
      }
      det.exportWords(argv[3]);
   } catch (const std::exception &e) {
      fprintf(stderr, "vocabulary_keys: %s\n", e.what());
      return 1;
   }
   return 0;
}
