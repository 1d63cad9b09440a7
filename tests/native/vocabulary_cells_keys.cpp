// vocabulary_cells_keys.cpp -- the cell members of AffineHessianDetector through hesaff_amd/csrc/hesaff.hpp: detect on an image, train C
// coarse rows and K rows inside their cells on its own descriptors, install both, detect again through the layer
// (tests/test_vocabulary_cells_host.py compiles it; tests/test_vocabulary_cells.py runs it).
//
//   vocabulary_cells_keys <image> <K> <C> <iterations> <vocabulary file to write>      (the cells go to <vocabulary file>.cells)
//
// Prints   C <cells that hold rows>,   per iteration   I <distortion> <empty words>,   and per key   W <word> <dist2>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../hesaff_amd/csrc/hesaff.hpp"

using namespace hesaff_amd;

int main(int argc, char **argv)
{
   if (argc != 6) {
      fprintf(stderr, "usage: vocabulary_cells_keys <image> <K> <C> <iterations> <vocabulary file>\n");
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
      const int n = (int)det.keys.size(), k = atoi(argv[2]), c = atoi(argv[3]), iterations = atoi(argv[4]);
      std::vector<uint8_t> desc((size_t)n * 128);
      for (int i = 0; i < n; i++)
         for (int j = 0; j < 128; j++) desc[(size_t)i * 128 + j] = det.keys[(size_t)i].desc[j];
      const std::vector<uint8_t> coarse = det.trainVocabulary(desc.data(), n, c, iterations);
      std::vector<uint8_t> rows((size_t)k * 128);
      for (long long r = 0; r < k; r++)
         for (int j = 0; j < 128; j++) rows[(size_t)r * 128 + j] = desc[(size_t)(r * n / k) * 128 + j];
      const AffineHessianDetector::VocabularyCells cells = det.buildVocabularyCells(rows, coarse.data(), c);
      rows = det.trainVocabularyCells(desc.data(), n, rows, cells, iterations);
      printf("C %d\n", cells.cells());
      for (size_t t = 0; t < det.distortion().size(); t++) printf("I %lld %d\n", (long long)det.distortion()[t], det.emptyWords()[t]);
      if (hesaff_write_vocabulary(argv[5], rows.data(), k) != HESAFF_OK) return 1;
      if (hesaff_write_vocabulary_cells((std::string(argv[5]) + ".cells").c_str(), cells.cells(), cells.coarse.data(), cells.first.data()) != HESAFF_OK) return 1;
      det.setVocabulary(rows.data(), k);
      det.setVocabularyCells(cells.coarse.data(), cells.first.data(), cells.cells());
      det.detectPyramidKeypoints(data, w, h, ch);
      hesaff_free(data);
      for (size_t i = 0; i < det.keys.size(); i++) printf("W %d %d\n", det.words()[2 * i], det.words()[2 * i + 1]);
   } catch (const std::exception &e) {
      fprintf(stderr, "vocabulary_cells_keys: %s\n", e.what());
      return 1;
   }
   return 0;
}
