// describe_filter.cpp -- "detect, choose, describe the chosen" through hesaff_amd/csrc/hesaff.hpp, the way a subclass of the
// reference's detector that filters in its callbacks is ported (tests/test_describe_regions.py builds and runs it).
// Both callbacks (pyramid.h:43-47, affine.h:48-58) are subclassed and collect what they receive; the affine shapes whose response
// lies above the median are kept and handed to AffineHessianDetector::onAffineShapesFound, the batch form of calling
// onAffineShapeFound (hesaff.cpp:73-105) for each of them.
//
//   describe_filter <image>
//
// Output, one line each:
//   S <index>                          a kept shape: its number among the onHessianKeypointDetected calls
//   K <hex of the 164-byte record>     keys[i] after onAffineShapesFound
//   N <g_numberOfPoints> <g_numberOfAffinePoints> <keys.size()>
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../hesaff_amd/csrc/hesaff.hpp"

using namespace hesaff_amd;

struct Collector : HessianKeypointCallback, AffineShapeCallback {
   int n_hessian = 0;
   std::vector<hesaff_region> shapes;   // what onAffineShapeFound received
   std::vector<int> index;              // ... and the Hessian keypoint each belongs to
   void onHessianKeypointDetected(const BlurPlane &, float, float, float, float, int, float) override { n_hessian++; }
   void onAffineShapeFound(const BlurPlane &blur, float x, float y, float s, float, float a11, float a12, float a21, float a22, int type,
                           float response, int iters) override
   {
      shapes.push_back(AffineHessianDetector::region(blur, x, y, s, type, response, a11, a12, a21, a22, iters));
      index.push_back(n_hessian - 1);   // hesaff.cpp:66-105: called right after its keypoint's onHessianKeypointDetected
   }
};

int main(int argc, char **argv)
{
   if (argc != 2) {
      fprintf(stderr, "usage: describe_filter <image>\n");
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
      Collector c;
      det.setHessianKeypointCallback(&c);
      det.setAffineShapeCallback(&c);
      det.detectPyramidKeypoints(data, w, h, ch);
      std::vector<float> resp;
      for (const hesaff_region &g : c.shapes) resp.push_back(g.response);
      std::sort(resp.begin(), resp.end());
      const float median = resp.empty() ? 0.0f : resp[resp.size() / 2];
      std::vector<hesaff_region> kept;
      for (size_t i = 0; i < c.shapes.size(); i++)
         if (c.shapes[i].response > median) {
            kept.push_back(c.shapes[i]);
            printf("S %d\n", c.index[i]);
         }
      std::vector<hesaff_region> described;
      det.onAffineShapesFound(data, w, h, ch, kept, &described);
      hesaff_free(data);
      if (described.size() != kept.size()) {
         fprintf(stderr, "describe_filter: %zu records back for %zu\n", described.size(), kept.size());
         return 1;
      }
      for (const Keypoint &k : det.keys) {
         const unsigned char *b = reinterpret_cast<const unsigned char *>(&k);
         printf("K ");
         for (size_t j = 0; j < sizeof(Keypoint); j++) printf("%02x", b[j]);
         printf("\n");
      }
      printf("N %d %d %zu\n", det.g_numberOfPoints, det.g_numberOfAffinePoints, det.keys.size());
   } catch (const std::exception &e) {
      fprintf(stderr, "describe_filter: %s\n", e.what());
      return 1;
   }
   return 0;
}
