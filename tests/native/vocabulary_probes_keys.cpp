// vocabulary_probes_keys.cpp -- setVocabularyProbes of AffineHessianDetector through hesaff_amd/csrc/hesaff.hpp: install a vocabulary
// and its cell layer from their files, set the probe count, detect on an image through the layer
// (tests/test_vocabulary_probes_host.py compiles it; tests/test_vocabulary_probes.py runs it).
//
//   vocabulary_probes_keys <image> <vocabulary file> <cells file> <P>
//
// Prints   P <the probe count the detector reports>   and per key   W <word> <dist2>
#include <cstdio>
#include <cstdlib>

#include "../../hesaff_amd/csrc/hesaff.hpp"

using namespace hesaff_amd;

int main(int argc, char **argv)
{
   if (argc != 5) {
      fprintf(stderr, "usage: vocabulary_probes_keys <image> <vocabulary file> <cells file> <P>\n");
      return 2;
   }
   uint8_t *data = nullptr, *rows = nullptr, *coarse = nullptr;
   uint32_t *first = nullptr;
   int rc = 1;
   try {
      int w = 0, h = 0, ch = 0, k = 0, c = 0, cell_rows = 0;
      if (hesaff_read_image(argv[1], &data, &w, &h, &ch) != HESAFF_OK || hesaff_read_vocabulary(argv[2], &rows, &k) != HESAFF_OK ||
          hesaff_read_vocabulary_cells(argv[3], &coarse, &first, &c, &cell_rows) != HESAFF_OK || cell_rows != k) {
         fprintf(stderr, "cannot read %s, %s or %s\n", argv[1], argv[2], argv[3]);
      } else {
         AffineHessianDetector det;
         det.setVocabularyProbes(atoi(argv[4]));   // before a layer exists: kept
         det.setVocabulary(rows, k);
         det.setVocabularyCells(coarse, first, c);
         printf("P %d\n", det.vocabularyProbes());
         det.detectPyramidKeypoints(data, w, h, ch);
         for (size_t i = 0; i < det.keys.size(); i++) printf("W %d %d\n", det.words()[2 * i], det.words()[2 * i + 1]);
         rc = 0;
      }
   } catch (const std::exception &e) {
      fprintf(stderr, "vocabulary_probes_keys: %s\n", e.what());
   }
   hesaff_free(data); hesaff_free(rows); hesaff_free(coarse); hesaff_free(first);
   return rc;
}
