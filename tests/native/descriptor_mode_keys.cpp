// descriptor_mode_keys.cpp -- AffineHessianDetector::setDescriptor through hesaff_amd/csrc/hesaff.hpp (tests/test_rootsift.py builds
// and runs it).
//
//   descriptor_mode_keys <mode: 0 | 1> <image>
//
// Prints what the detector holds afterwards, every key as the hex of its bytes (x, y, s, a11, a12, a21, a22, response, type, desc):
//   N <g_numberOfPoints> <g_numberOfAffinePoints> <keys.size()>
//   K <328 hex digits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../hesaff_amd/csrc/hesaff.hpp"

using namespace hesaff_amd;

int main(int argc, char **argv)
{
   if (argc != 3) {
      fprintf(stderr, "usage: descriptor_mode_keys <mode> <image>\n");
      return 2;
   }
   try {
      AffineHessianDetector det;
      det.setDescriptor(atoi(argv[1]));
      uint8_t *data = nullptr;
      int w = 0, h = 0, ch = 0;
      if (hesaff_read_image(argv[2], &data, &w, &h, &ch) != HESAFF_OK) {
         fprintf(stderr, "cannot read %s\n", argv[2]);
         return 1;
      }
      det.detectPyramidKeypoints(data, w, h, ch);
      hesaff_free(data);
      printf("N %d %d %zu\n", det.g_numberOfPoints, det.g_numberOfAffinePoints, det.keys.size());
      static_assert(sizeof(det.keys[0]) == 164, "struct Keypoint of hesaff.cpp:41-48");
      for (const auto &k : det.keys) {
         unsigned char b[164];
         memcpy(b, &k, sizeof b);
         printf("K ");
         for (unsigned char v : b) printf("%02x", v);
         printf("\n");
      }
   } catch (const std::exception &e) {
      fprintf(stderr, "descriptor_mode_keys: %s\n", e.what());
      return 1;
   }
   return 0;
}
