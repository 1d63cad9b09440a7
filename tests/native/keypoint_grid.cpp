// keypoint_grid.cpp -- AffineHessianDetector::setKeypointGrid (with setKeypointLimit) through hesaff_amd/csrc/hesaff.hpp with both of the reference's
// callbacks installed (tests/test_keypoint_grid.py builds and runs it).
//
//   keypoint_grid <limit> <rows> <cols> <image>
//
// Prints how often each callback fired and what the detector holds afterwards, and the response of every Hessian callback
// (hex of its bits, call order):
//   R <response>
//   C <onHessianKeypointDetected calls> <onAffineShapeFound calls>
//   N <g_numberOfPoints> <g_numberOfAffinePoints> <keys.size()>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../hesaff_amd/csrc/hesaff.hpp"

using namespace hesaff_amd;

struct Counter : HessianKeypointCallback, AffineShapeCallback {
   int hessian = 0, affine = 0;
   void onHessianKeypointDetected(const BlurPlane &, float, float, float, float, int, float response) override
   {
      unsigned u;
      memcpy(&u, &response, 4);
      printf("R %08x\n", u);
      hessian++;
   }
   void onAffineShapeFound(const BlurPlane &, float, float, float, float, float, float, float, float, int, float, int) override { affine++; }
};

int main(int argc, char **argv)
{
   if (argc != 5) {
      fprintf(stderr, "usage: keypoint_grid <limit> <rows> <cols> <image>\n");
      return 2;
   }
   try {
      AffineHessianDetector det;
      Counter c;
      det.setHessianKeypointCallback(&c);
      det.setAffineShapeCallback(&c);
      det.setKeypointLimit(atoi(argv[1]));
      det.setKeypointGrid(atoi(argv[2]), atoi(argv[3]));
      uint8_t *data = nullptr;
      int w = 0, h = 0, ch = 0;
      if (hesaff_read_image(argv[4], &data, &w, &h, &ch) != HESAFF_OK) {
         fprintf(stderr, "cannot read %s\n", argv[4]);
         return 1;
      }
      det.detectPyramidKeypoints(data, w, h, ch);
      hesaff_free(data);
      printf("C %d %d\n", c.hessian, c.affine);
      printf("N %d %d %zu\n", det.g_numberOfPoints, det.g_numberOfAffinePoints, det.keys.size());
   } catch (const std::exception &e) {
      fprintf(stderr, "keypoint_grid: %s\n", e.what());
      return 1;
   }
   return 0;
}
