// detection_mask.cpp -- AffineHessianDetector::setMask through hesaff_amd/csrc/hesaff.hpp with both of the reference's callbacks
// installed (tests/test_detection_mask.py builds and runs it).
//
//   detection_mask <image> <mask image>
//
// Runs detectPyramidKeypoints twice: with the mask set, then without calling setMask again (the mask is one-shot).  Prints, for the
// first run, the response of every Hessian callback (hex of its bits, call order), how often each callback fired and what the
// detector holds afterwards; for the second run the Hessian callbacks alone:
//   R <response>
//   C <onHessianKeypointDetected calls> <onAffineShapeFound calls>
//   N <g_numberOfPoints> <keys.size()>
//   U <onHessianKeypointDetected calls of the second, unmasked run> <g_numberOfPoints>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../hesaff_amd/csrc/hesaff.hpp"

using namespace hesaff_amd;

struct Counter : HessianKeypointCallback, AffineShapeCallback {
   int hessian = 0, affine = 0;
   bool print = true;
   void onHessianKeypointDetected(const BlurPlane &, float, float, float, float, int, float response) override
   {
      unsigned u;
      memcpy(&u, &response, 4);
      if (print) printf("R %08x\n", u);
      hessian++;
   }
   void onAffineShapeFound(const BlurPlane &, float, float, float, float, float, float, float, float, int, float, int) override { affine++; }
};

int main(int argc, char **argv)
{
   if (argc != 3) {
      fprintf(stderr, "usage: detection_mask <image> <mask image>\n");
      return 2;
   }
   try {
      uint8_t *data = nullptr, *mask = nullptr;
      int w = 0, h = 0, ch = 0, mw = 0, mh = 0, mch = 0;
      if (hesaff_read_image(argv[1], &data, &w, &h, &ch) != HESAFF_OK || hesaff_read_image(argv[2], &mask, &mw, &mh, &mch) != HESAFF_OK) {
         fprintf(stderr, "cannot read %s or %s\n", argv[1], argv[2]);
         return 1;
      }
      if (mch != 1 || mw != w || mh != h) {
         fprintf(stderr, "%s is not a one-channel mask of the image's size\n", argv[2]);
         return 1;
      }
      AffineHessianDetector det;
      Counter c;
      det.setHessianKeypointCallback(&c);
      det.setAffineShapeCallback(&c);
      det.setMask(mask, (size_t)mw);
      det.detectPyramidKeypoints(data, w, h, ch);
      printf("C %d %d\n", c.hessian, c.affine);
      printf("N %d %zu\n", det.g_numberOfPoints, det.keys.size());
      c.hessian = 0;
      c.print = false;
      det.detectPyramidKeypoints(data, w, h, ch);
      printf("U %d %d\n", c.hessian, det.g_numberOfPoints);
      hesaff_free(data);
      hesaff_free(mask);
   } catch (const std::exception &e) {
      fprintf(stderr, "detection_mask: %s\n", e.what());
      return 1;
   }
   return 0;
}
