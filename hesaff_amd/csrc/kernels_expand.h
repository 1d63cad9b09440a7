// kernels_expand.h -- query expansion (hesaff_expand_query of include/hesaff_amd.h): the keys of the selected candidates of a verified
// shortlist, back-projected into the query's frame by each candidate's affinity, filtered by the query's region and appended to the
// query in a fixed order.  Only the rows of selected candidates are read.  A wavefront owns one tile of HS_EXPAND_TILE = 64
// consecutive rows of one selected candidate; the tiles lie in rank order (expand_plan.h: ExpandTiles), so the position of a kept
// row in the output is the kept rows of the tiles before its own plus the kept lanes below its own - no cursor, no atomic on the
// order, nothing sorted, and the same bytes for whichever schedule runs it.
//
// k_expand_flags: every lane computes expand_key (expand_plan.h) of its row; __ballot makes the tile's mask.  exclusive_scan
// (pipeline.hip) over the popcounts of the masks gives every tile's base and kept_total.  k_expand_scatter computes the same function
// once more - cheaper than keeping 24 bytes per row between the passes - and writes the kept rows whose position lies below max_rows.
// The per-candidate counts are integer atomics, one per tile and count: order-free.
//
// A block holds the prefix of the tile table (at most 1025 words) in LDS and each of its four waves walks HS_EXPAND_WAVE_TILES
// consecutive tiles, so the table is read once per 16 tiles; the owner of a tile is a binary search of that copy, the same address in
// every lane.  A row is 24 bytes at a 24-byte stride: a lane loads its own row with dword loads, and the 64 lanes of a wave cover
// 1536 consecutive bytes, twelve whole 128-byte lines, so every byte fetched is used.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "expand_plan.h"

using hesaff_plan::VerifyRow;
using hesaff_plan::ExpandCand;
using hesaff_plan::ExpandRoi;

#define HS_EXPAND_WAVE_TILES 4                               // consecutive tiles of a wave
#define HS_EXPAND_BLOCK_TILES (4 * HS_EXPAND_WAVE_TILES)     // of a block of 256 threads

__device__ __forceinline__ void hs_expand_load_prefix(uint32_t *s_prefix, const uint32_t *__restrict__ prefix, int n_selected)
{
   for (int i = (int)threadIdx.x; i <= n_selected; i += 256) s_prefix[i] = prefix[i];
   __syncthreads();
}

// mask[tile] = the kept rows of the tile; info[s][0] += its live rows (zero on entry).  Grid: ceil(tiles / HS_EXPAND_BLOCK_TILES).
__global__ __launch_bounds__(256) void k_expand_flags(const VerifyRow *__restrict__ rows, const ExpandCand *__restrict__ cand, const uint32_t *__restrict__ prefix,
                                                      int n_selected, uint32_t tiles, ExpandRoi roi, unsigned long long *__restrict__ mask, uint32_t *__restrict__ info)
{
   __shared__ uint32_t s_prefix[hesaff_plan::HS_EXPAND_MAX_IMAGES + 1];
   hs_expand_load_prefix(s_prefix, prefix, n_selected);
   const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
   const uint32_t first = (blockIdx.x * 4u + wv) * HS_EXPAND_WAVE_TILES;
   for (uint32_t t = 0; t < HS_EXPAND_WAVE_TILES; t++) {
      const uint32_t tile = first + t;
      if (tile >= tiles) return;   // (the whole wave)
      const uint32_t s = hesaff_plan::expand_tile_owner(s_prefix, (uint32_t)n_selected, tile);
      const ExpandCand c = cand[s];
      const uint32_t j = (tile - s_prefix[s]) * hesaff_plan::HS_EXPAND_TILE + lane;
      bool live = false, kept = false;
      if (j < c.count) {
         const hesaff_plan::ExpandKey e = hesaff_plan::expand_key(rows[(size_t)c.start + j], c.a, roi);
         live = e.live; kept = e.kept;
      }
      const unsigned long long m = __ballot(kept), l = __ballot(live);
      if (lane == 0u) {
         mask[tile] = m;
         if (l != 0ull) atomicAdd(&info[s * hesaff_plan::HS_EXPAND_INFO], (uint32_t)__popcll(l));
      }
   }
}

// The kept rows into rows_out / words_out / sigs_out at nq + base[tile] + (the kept lanes below), where that lies below max_rows;
// info[s][1] += the tile's kept rows, info[s][2] += the written ones.  sigs, sigs_out: both NULL or both given.
__global__ __launch_bounds__(256) void k_expand_scatter(const VerifyRow *__restrict__ rows, const unsigned long long *__restrict__ sigs, const ExpandCand *__restrict__ cand,
                                                        const uint32_t *__restrict__ prefix, int n_selected, uint32_t tiles, ExpandRoi roi,
                                                        const unsigned long long *__restrict__ mask, const uint32_t *__restrict__ base, uint32_t nq, uint32_t max_rows,
                                                        VerifyRow *__restrict__ rows_out, int32_t *__restrict__ words_out, unsigned long long *__restrict__ sigs_out,
                                                        uint32_t *__restrict__ info)
{
   __shared__ uint32_t s_prefix[hesaff_plan::HS_EXPAND_MAX_IMAGES + 1];
   hs_expand_load_prefix(s_prefix, prefix, n_selected);
   const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
   const uint32_t first = (blockIdx.x * 4u + wv) * HS_EXPAND_WAVE_TILES;
   for (uint32_t t = 0; t < HS_EXPAND_WAVE_TILES; t++) {
      const uint32_t tile = first + t;
      if (tile >= tiles) return;   // (the whole wave)
      const unsigned long long m = mask[tile];
      if (m == 0ull) continue;
      const uint32_t s = hesaff_plan::expand_tile_owner(s_prefix, (uint32_t)n_selected, tile);
      const uint32_t kept = (uint32_t)__popcll(m);
      const uint32_t at = nq + base[tile];   // (nq <= 2^18 and kept_total <= 2^28: no wrap)
      const uint32_t room = at < max_rows ? max_rows - at : 0u;
      const uint32_t written = kept < room ? kept : room;
      if (lane == 0u) {
         atomicAdd(&info[s * hesaff_plan::HS_EXPAND_INFO + 1], kept);
         if (written != 0u) atomicAdd(&info[s * hesaff_plan::HS_EXPAND_INFO + 2], written);
      }
      if (written == 0u) continue;   // (the cut: nothing of this tile is read again)
      const uint32_t below = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      if (((m >> lane) & 1ull) == 0ull || below >= written) continue;
      const ExpandCand c = cand[s];
      const size_t src = (size_t)c.start + (tile - s_prefix[s]) * hesaff_plan::HS_EXPAND_TILE + lane;
      const VerifyRow k = rows[src];
      const hesaff_plan::ExpandKey e = hesaff_plan::expand_key(k, c.a, roi);
      const size_t pos = (size_t)at + below;
      VerifyRow o;
      o.x = e.x; o.y = e.y; o.a = e.a; o.b = e.b; o.c = e.c; o.word = k.word;
      rows_out[pos] = o;
      words_out[pos] = (int32_t)k.word;
      if (sigs_out) sigs_out[pos] = sigs[src];
   }
}

// words_out[i] = the word of query row i.  Grid: ceil(nq / 256).
__global__ __launch_bounds__(256) void k_expand_query_words(const VerifyRow *__restrict__ rows, int nq, int32_t *__restrict__ words_out)
{
   const int i = (int)(blockIdx.x * 256u + threadIdx.x);
   if (i < nq) words_out[i] = (int32_t)rows[i].word;
}

// The anchor rows of the eligible candidates, for the host's check of a device-form call: anchors[r][0] = query row out[r][3],
// anchors[r][1] = row out[r][4] of candidate r, where the candidate is eligible and both keys lie inside their arrays; nothing is
// read or written otherwise (the host refuses such a candidate before it looks).  One block of 1024 threads.
__global__ __launch_bounds__(1024) void k_expand_anchors(const VerifyRow *__restrict__ qrows, const VerifyRow *__restrict__ crows, const uint32_t *__restrict__ starts,
                                                         const int32_t *__restrict__ out, int n_candidates, int nq, int min_inliers, VerifyRow *__restrict__ anchors)
{
   const int r = (int)threadIdx.x;
   if (r >= n_candidates) return;
   const int32_t *o = out + (size_t)r * 6;
   if (o[0] < min_inliers) return;
   const uint32_t count = starts[r + 1] - starts[r];
   if (o[3] < 0 || o[3] >= nq || o[4] < 0 || (uint32_t)o[4] >= count) return;
   anchors[(size_t)r * 2] = qrows[o[3]];
   anchors[(size_t)r * 2 + 1] = crows[(size_t)starts[r] + (uint32_t)o[4]];
}
