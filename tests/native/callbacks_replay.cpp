// callbacks_replay.cpp -- the reference's two detector callbacks (pyramid.h:43-47, affine.h:48-58) subclassed through
// hesaff_amd/csrc/hesaff.hpp, as code written against the reference would do it (tests/test_regions.py builds and runs it).
//
//   callbacks_replay <image> [<image> ...]
//
// For every image: the callback stream in call order, then the keys, one line each; floats as the hex of their bits:
//   I <index> <width> <height>
//   H <x> <y> <s> <pixelDistance> <type> <response> <octave> <level>          onHessianKeypointDetected
//   A <x> <y> <s> <pixelDistance> <a11> <a12> <a21> <a22> <type> <response> <iters>   onAffineShapeFound
//   K <hex of the 164-byte record>                                          keys[i]
//   N <g_numberOfPoints> <g_numberOfAffinePoints> <keys.size()>
// With no callback set (argument "--plain" first) only the K and N lines are printed.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../hesaff_amd/csrc/hesaff.hpp"

using namespace hesaff_amd;

static unsigned bits(float v)
{
   unsigned u;
   memcpy(&u, &v, 4);
   return u;
}

struct Printer : HessianKeypointCallback, AffineShapeCallback {
   void onHessianKeypointDetected(const BlurPlane &blur, float x, float y, float s, float pixelDistance, int type, float response) override
   {
      printf("H %08x %08x %08x %08x %d %08x %d %d\n", bits(x), bits(y), bits(s), bits(pixelDistance), type, bits(response), blur.octave, blur.level);
   }
   void onAffineShapeFound(const BlurPlane &blur, float x, float y, float s, float pixelDistance, float a11, float a12, float a21, float a22,
                           int type, float response, int iters) override
   {
      if (bits(blur.pixelDistance) != bits(pixelDistance)) printf("E plane and argument disagree\n");
      printf("A %08x %08x %08x %08x %08x %08x %08x %08x %d %08x %d\n", bits(x), bits(y), bits(s), bits(pixelDistance), bits(a11), bits(a12),
             bits(a21), bits(a22), type, bits(response), iters);
   }
};

int main(int argc, char **argv)
{
   int first = 1;
   const bool plain = argc > 1 && strcmp(argv[1], "--plain") == 0;
   if (plain) first = 2;
   if (argc <= first) {
      fprintf(stderr, "usage: callbacks_replay [--plain] <image> [<image> ...]\n");
      return 2;
   }
   try {
      AffineHessianDetector det;
      Printer p;
      if (!plain) {
         det.setHessianKeypointCallback(&p);
         det.setAffineShapeCallback(&p);
      }
      int total_affine = 0;
      for (int i = first; i < argc; i++) {
         uint8_t *data = nullptr;
         int w = 0, h = 0, ch = 0;
         if (hesaff_read_image(argv[i], &data, &w, &h, &ch) != HESAFF_OK) {
            fprintf(stderr, "cannot read %s\n", argv[i]);
            return 1;
         }
         printf("I %d %d %d\n", i - first, w, h);
         det.detectPyramidKeypoints(data, w, h, ch);
         hesaff_free(data);
         for (const Keypoint &k : det.keys) {
            const unsigned char *b = reinterpret_cast<const unsigned char *>(&k);
            printf("K ");
            for (size_t j = 0; j < sizeof(Keypoint); j++) printf("%02x", b[j]);
            printf("\n");
         }
         total_affine = det.g_numberOfAffinePoints;
         printf("N %d %d %zu\n", det.g_numberOfPoints, total_affine, det.keys.size());
      }
   } catch (const std::exception &e) {
      fprintf(stderr, "callbacks_replay: %s\n", e.what());
      return 1;
   }
   return 0;
}
