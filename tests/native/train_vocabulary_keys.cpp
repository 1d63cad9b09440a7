// train_vocabulary_keys.cpp -- AffineHessianDetector::trainVocabulary through hesaff_amd/csrc/hesaff.hpp: detect on an image, train K
// words on its own descriptors, install them (tests/test_vocabulary_training_host.py compiles it; tests/test_vocabulary_training.py runs it).
//
//   train_vocabulary_keys <image> <K> <iterations> <vocabulary file to write>
//
// Prints   T <iterations run>   and per iteration   I <distortion> <empty words>
#include <cstdio>
#include <cstdlib>

#include "../../hesaff_amd/csrc/hesaff.hpp"

using namespace hesaff_amd;

int main(int argc, char **argv)
{
   if (argc != 5) {
      fprintf(stderr, "usage: train_vocabulary_keys <image> <K> <iterations> <vocabulary file>\n");
      return 2;
   }
   try {
      uint8_t *data = nullptr;
      int w = 0, h = 0, ch = 0;
      if (hesaff_read_image(argv[1], &data, &w, &h, &ch) != HESAFF_OK) {
         fprintf(stderr, "cannot read %s\n", argv[1]);
         return 1;
      }
      AffineHessianDetector det;
      det.detectPyramidKeypoints(data, w, h, ch);
      hesaff_free(data);
      std::vector<uint8_t> desc(det.keys.size() * 128);
      for (size_t i = 0; i < det.keys.size(); i++)
         for (int j = 0; j < 128; j++) desc[i * 128 + j] = det.keys[i].desc[j];
      const int k = atoi(argv[2]);
      const std::vector<uint8_t> rows = det.trainVocabulary(desc.data(), (int)det.keys.size(), k, atoi(argv[3]));
      printf("T %zu\n", det.distortion().size());
      for (size_t t = 0; t < det.distortion().size(); t++) printf("I %lld %d\n", (long long)det.distortion()[t], det.emptyWords()[t]);
      if (hesaff_write_vocabulary(argv[4], rows.data(), k) != HESAFF_OK) return 1;
      det.setVocabulary(rows.data(), k);
   } catch (const std::exception &e) {
      fprintf(stderr, "train_vocabulary_keys: %s\n", e.what());
      return 1;
   }
   return 0;
}
