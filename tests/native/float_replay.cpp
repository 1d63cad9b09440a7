// float_replay.cpp -- the reference's two detector callbacks (pyramid.h:43-47, affine.h:48-58) subclassed through
// hesaff_amd/csrc/hesaff.hpp on the reference's own input, a CV_32FC1 plane (detectPyramidKeypoints(const Mat &), pyramid.h:73);
// tests/test_float_input.py builds and runs it.
//
//   float_replay [--plain] <plane.f32> <width> <height> [<plane.f32> <width> <height> ...]
//
// A plane file is width x height little-endian float32 values, rows tightly packed.  Output as callbacks_replay.cpp prints it:
//   I <index> <width> <height> / H ... / A ... / K <hex of the record> / N <g_numberOfPoints> <g_numberOfAffinePoints> <keys.size()>
// The planes are handed over with padded rows (stride = 4 * width + 64 bytes), the way a cv::Mat ROI carries them.
#include <cstdio>
#include <cstdlib>
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
   if (argc <= first || (argc - first) % 3 != 0) {
      fprintf(stderr, "usage: float_replay [--plain] <plane.f32> <width> <height> [...]\n");
      return 2;
   }
   try {
      AffineHessianDetector det;
      Printer p;
      if (!plain) {
         det.setHessianKeypointCallback(&p);
         det.setAffineShapeCallback(&p);
      }
      for (int i = first, img = 0; i < argc; i += 3, img++) {
         const int w = atoi(argv[i + 1]), h = atoi(argv[i + 2]);
         const size_t stride = (size_t)w + 16;   // floats per row
         std::vector<float> plane(stride * (size_t)h, 0.0f);
         FILE *f = fopen(argv[i], "rb");
         if (!f) {
            fprintf(stderr, "cannot read %s\n", argv[i]);
            return 1;
         }
         bool ok = true;
         for (int y = 0; y < h && ok; y++) ok = fread(&plane[stride * (size_t)y], 4, (size_t)w, f) == (size_t)w;
         fclose(f);
         if (!ok) {
            fprintf(stderr, "%s is shorter than %d x %d floats\n", argv[i], w, h);
            return 1;
         }
         printf("I %d %d %d\n", img, w, h);
         det.detectPyramidKeypoints(plane.data(), w, h, stride * sizeof(float));
         for (const Keypoint &k : det.keys) {
            const unsigned char *b = reinterpret_cast<const unsigned char *>(&k);
            printf("K ");
            for (size_t j = 0; j < sizeof(Keypoint); j++) printf("%02x", b[j]);
            printf("\n");
         }
         printf("N %d %d %zu\n", det.g_numberOfPoints, det.g_numberOfAffinePoints, det.keys.size());
      }
   } catch (const std::exception &e) {
      fprintf(stderr, "float_replay: %s\n", e.what());
      return 1;
   }
   return 0;
}
