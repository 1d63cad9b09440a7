// jpeg_plan.h -- the host arithmetic of the device JPEG stage (kernels_jpeg.h): the geometry k_jpeg_idct and k_jpeg_pixels work from,
// made from the hesaff_jpeg_layout a caller hands in - which layouts are refused, jdsample.c's up-sampling method per component, and
// where the components' coefficients and planes lie.  Plain structs and one pure function, no HIP: kernels_jpeg.h and pipeline.hip
// obtain their numbers here, and tests/native/jpeg_plan_check.cpp checks them on the CPU (tests/test_jpeg_constructed_host.py) - every
// bound on both sides, the method table, and that no sample index the kernels can form from an accepted layout leaves its plane.
#pragma once
#include <cstdint>
#include <cstring>

#include "../../include/hesaff_amd.h"   // hesaff_jpeg_layout, HESAFF_JPEG_BLOB_HEADER

struct JpegGeom {
   int W, H, nc;
   int bw[3], bh[3], cw[3], chgt[3], hx[3], vx[3], mode[3];
   unsigned long long coef_off[3];    // bytes from the start of an image's blob
   unsigned long long plane_off[3];   // bytes from the start of an image's planes
   unsigned long long blob_bytes, plane_bytes;
   unsigned int blocks[3], blocks_per_image;
};
enum { JPEG_UP_NONE = 0, JPEG_UP_H2V1 = 1, JPEG_UP_H2V2 = 2, JPEG_UP_H1V2 = 3, JPEG_UP_REPLICATE = 4 };

namespace hesaff_plan {

// hesaff_jpeg_layout (what the host's entropy stage reports; from a caller, so checked) -> the kernels' geometry; false: refused
inline bool make_jpeg_geom(const hesaff_jpeg_layout &L, JpegGeom &g)
{
   memset(&g, 0, sizeof g);
   if (L.width < 1 || L.height < 1 || L.width > 65535 || L.height > 65535 || (L.channels != 1 && L.channels != 3)) return false;
   g.W = L.width; g.H = L.height; g.nc = L.channels;
   unsigned long long coef = HESAFF_JPEG_BLOB_HEADER, plane = 0, blocks = 0;
   for (int i = 0; i < g.nc; i++) {
      const long long bw = L.bw[i], bh = L.bh[i], cw = L.cw[i], chgt = L.chgt[i], hx = L.hx[i], vx = L.vx[i];
      if (bw < 1 || bh < 1 || bw > 8192 || bh > 8192 || cw < 1 || chgt < 1 || cw > bw * 8 || chgt > bh * 8 || hx < 1 || hx > 4 || vx < 1 || vx > 4 ||
          cw * hx < L.width || chgt * vx < L.height || (g.nc == 1 && (hx != 1 || vx != 1)))
         return false;
      g.bw[i] = (int)bw; g.bh[i] = (int)bh; g.cw[i] = (int)cw; g.chgt[i] = (int)chgt; g.hx[i] = (int)hx; g.vx[i] = (int)vx;
      // jdsample.c's choice of method (jpeg_decode.cpp)
      g.mode[i] = (hx == 1 && vx == 1) ? JPEG_UP_NONE : (hx == 2 && vx == 1 && cw > 2) ? JPEG_UP_H2V1 : (hx == 2 && vx == 2 && cw > 2) ? JPEG_UP_H2V2
                  : (hx == 1 && vx == 2) ? JPEG_UP_H1V2 : JPEG_UP_REPLICATE;
      g.blocks[i] = (unsigned int)(bw * bh);
      g.coef_off[i] = coef; g.plane_off[i] = plane;
      coef += (unsigned long long)(bw * bh) * 128;
      plane += (unsigned long long)(bw * bh) * 64;
      blocks += (unsigned long long)(bw * bh);
   }
   if (blocks > 0x7fffffffull) return false;
   g.blob_bytes = coef; g.plane_bytes = plane; g.blocks_per_image = (unsigned int)blocks;
   return true;
}

} // namespace hesaff_plan
