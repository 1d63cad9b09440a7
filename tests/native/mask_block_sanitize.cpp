// mask_block_sanitize.cpp -- the host arithmetic of hesaff_set_next_masks under AddressSanitizer + UBSan, without a device
// (tests/test_detection_mask.py builds and runs it): ArrayIO deals a caller's masks out to chunks of one geometry
// (chunk_engine.h), fill_mask_block lays a chunk's masks out as the device reads them (batch_plan.h: mask_planes_offset,
// mask_block_bytes).  Every mask lives in a heap block that ends with the last pixel of its last row, so a copy that read the
// padding behind a row would read outside it, and every chunk's block is allocated at exactly mask_block_bytes.
//
//   mask_block_sanitize <max_batch>
//
// Prints "chunks=<n> masked_chunks=<n> planes=<n> ok" when every present flag and every plane byte is the caller's.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../hesaff_amd/csrc/chunk_engine.h"
#include "../../hesaff_amd/csrc/batch_plan.h"

using namespace hesaff_engine;
using namespace hesaff_plan;

static uint8_t mask_pixel(int j, int y, int x) { return (uint8_t)(((j * 131 + y * 17 + x * 7) % 5 == 0) ? 0 : 1 + (j + y + x) % 255); }

int main(int argc, char **argv)
{
   const int max_batch = argc > 1 ? atoi(argv[1]) : 2;
   const int sizes[3][2] = {{40, 30}, {31, 25}, {16, 12}};   // W, H
   const int n = 23;
   std::vector<int> widths(n), heights(n), strides(n), mstrides(n);
   std::vector<std::unique_ptr<uint8_t[]>> pix(n), mpix(n);
   std::vector<const uint8_t *> images(n), masks(n);
   for (int j = 0; j < n; j++) {
      const int W = sizes[(j * 7 + j / 3) % 3][0], H = sizes[(j * 7 + j / 3) % 3][1];
      widths[j] = W; heights[j] = H; strides[j] = W;
      pix[j].reset(new uint8_t[(size_t)W * H]());
      images[j] = pix[j].get();
      mstrides[j] = W + (j % 4) * 5;   // every fourth tightly packed
      masks[j] = nullptr;
      if (j % 3 == 1) continue;        // a third of the images have no mask
      const size_t bytes = (size_t)mstrides[j] * (H - 1) + W;
      mpix[j].reset(new uint8_t[bytes]);
      for (int y = 0; y < H; y++)
         for (int x = 0; x < (y == H - 1 ? W : mstrides[j]); x++) mpix[j][(size_t)y * mstrides[j] + x] = x < W ? mask_pixel(j, y, x) : 0xEE;
      masks[j] = mpix[j].get();
   }
   // images 18 .. 20 (one per geometry at most) lose their masks, so that some chunk of a small max_batch has none at all
   for (int j = 18; j < 21; j++) masks[j] = nullptr;
   BlockRing ring;
   MaskInput mi;
   mi.masks = masks.data(); mi.strides = mstrides.data();
   ArrayIO io(&ring, max_batch, n, images.data(), widths.data(), heights.data(), strides.data(), nullptr, false, nullptr, nullptr, 0, mi);
   int chunks = 0, masked = 0, planes = 0;
   std::vector<char> seen(n, 0);
   HostChunk q;
   while (io.next(q)) {
      chunks++;
      const int B = (int)q.data.size();
      bool any = false;
      for (int b = 0; b < B; b++) {
         seen[q.index[b]]++;
         any = any || masks[q.index[b]];
      }
      if (q.masks.empty() != !any) { fprintf(stderr, "chunk %d: masks present %d, expected %d\n", chunks, (int)!q.masks.empty(), (int)any); return 1; }
      if (!any) continue;
      masked++;
      if ((int)q.masks.size() != B || (int)q.mask_stride.size() != B) { fprintf(stderr, "chunk %d: %zu masks for %d images\n", chunks, q.masks.size(), B); return 1; }
      const size_t at = mask_planes_offset(B), bytes = mask_block_bytes(B, q.H, q.W);
      std::unique_ptr<uint8_t[]> blk(new uint8_t[bytes]);
      for (size_t i = 0; i < bytes; i++) blk[i] = 0xCC;
      fill_mask_block(blk.get(), at, q);
      for (int b = 0; b < B; b++) {
         const int j = q.index[b];
         if (blk[b] != (masks[j] ? 1 : 0)) { fprintf(stderr, "image %d: present flag %d\n", j, blk[b]); return 1; }
         if (!masks[j]) continue;
         planes++;
         for (int y = 0; y < q.H; y++)
            for (int x = 0; x < q.W; x++)
               if (blk[at + ((size_t)b * q.H + y) * q.W + x] != mask_pixel(j, y, x)) { fprintf(stderr, "image %d: pixel (%d, %d) is not its mask's\n", j, y, x); return 1; }
      }
   }
   for (int j = 0; j < n; j++)
      if (seen[j] != 1) { fprintf(stderr, "image %d dealt out %d times\n", j, seen[j]); return 1; }
   printf("chunks=%d masked_chunks=%d planes=%d ok\n", chunks, masked, planes);
   return 0;
}
