// kernels_cells.h -- visual-word assignment through vocabulary cells (hesaff_set_vocabulary_cells, include/hesaff_amd.h): a key is
// compared with the C coarse rows, then only with the rows of the cell it fell into - C + K / C exact distances instead of K.
//
// The steps (launch_assign_cells, pipeline.hip).  k_assign_words (kernels_words.h) runs unchanged against the packed coarse rows: (cell,
// dist2 to the coarse row) per key.  The keys are grouped by cell with the kernels of kernels_train.h as they are - k_word_histogram,
// exclusive_scan, k_word_scatter - into `perm`, a cell's keys neighbours, its range read off the cursor behind the scatter.  A cell with
// m keys makes ceil(m / 64) work items; a second scan (LoadCellItems) gives each cell's first item and the total.  The order of the keys
// inside a cell depends on which wave came first: no result below depends on it.
//
// k_assign_words_cells is the frame of kernels_words.h - keys, stream, running best - over one work item: up to 64 keys of ONE cell
// gathered through perm.  The grid is sized by the host's bound, floor(n / 64) + C (cells_plan.h); a wave beyond the device's total
// returns; a wave finds its cell by binary search in the item offsets (wave-uniform: scalar loads).  It streams tiles first[c] / 32 ..
// (first[c + 1] - 1) / 32 of the context's flat packed vocabulary - the layout on the device is the flat kernel's.  Only a cell's
// first and last tile can hold rows of other cells: there (a wave-uniform branch) the visit masks a row outside [first[c],
// first[c + 1]), and a cell has at least one real row, so the minimum is a row of the cell.  Each key's 8 bytes go to its own index.
// Plain loads and vector stores, no atomics: every result is a function of the key alone.
//
// With probes (hesaff_set_vocabulary_probes, P' = min(P, C) > 1; launch_assign_cells): k_probe_cells replaces the first step and gives
// every key P' cells, the grouping and k_assign_words_cells<true> run over the n P' entries (key, rank), and k_merge_probes takes each
// key's lexicographic minimum.  With P' = 1 none of the three is launched.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cells_plan.h"
#include "kernels_words.h"

// the work items of cell i from the cursor behind k_word_scatter (cursor[i][slots - 1]: the end of cell i's keys in perm): the load of
// the second scan (exclusive_scan).  p: the cursor (and the pointer k_scan_down tests for alignment).
struct LoadCellItems {
   const uint32_t *p;
   int slots;
   __device__ uint32_t operator()(long long i) const
   {
      const uint32_t end = p[(size_t)i * slots + slots - 1], begin = i > 0 ? p[(size_t)i * slots - 1] : 0u;
      return hesaff_plan::cells_items_of(end - begin);
   }
   __device__ void load16(long long base, uint32_t *v) const
   {
#pragma unroll
      for (int i = 0; i < 16; i++) v[i] = (*this)(base + i);
   }
};

// a value the lanes of a wave agree on, where the compiler cannot see that they do: kept in a scalar register
__device__ __forceinline__ uint32_t hs_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// desc, stride, offset, tiles, norms, out: as for k_assign_words (the keys of a slice: perm holds indices into it).  cursor[c][slots]
// behind k_word_scatter, item_first[c + 1] behind the second scan, first[c + 1]: the cells' rows.  Grid: ceil(item bound / 4) blocks.
// PROBES (hesaff_set_vocabulary_probes with P' = used > 1): perm holds entries, key * used + rank, a key at most once in a cell since
// its probes are distinct cells; the bytes are the key's, the 8 bytes of the result go to the ENTRY's slot of out, which k_merge_probes
// reduces.  Without PROBES `used` is not read and an entry is the key.
template <bool PROBES>
__global__ __launch_bounds__(HS_WORD_BLOCK_WAVES * 64) void k_assign_words_cells(const uint8_t *__restrict__ desc, long long stride, long long offset,
                                                                                const uint32_t *__restrict__ perm, const uint32_t *__restrict__ cursor, int slots,
                                                                                const uint32_t *__restrict__ item_first, const uint32_t *__restrict__ first, int c,
                                                                                const hs_v4i *__restrict__ tiles, const int32_t *__restrict__ norms,
                                                                                int32_t *__restrict__ out, int used)
{
   const int lane = (int)(threadIdx.x & 63u);
   const int r = lane & 31, h = lane >> 5;
   const uint32_t item = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * HS_WORD_BLOCK_WAVES + (threadIdx.x >> 6)));
   if (item >= item_first[c]) return;   // (wave-uniform)
   const int cell = (int)hs_uniform((uint32_t)hesaff_plan::cells_item_cell(item_first, c, item));
   // (all of these are the same for the 64 lanes)
   const uint32_t key_end = hs_uniform(cursor[(size_t)cell * slots + slots - 1]), key_begin = cell > 0 ? hs_uniform(cursor[(size_t)cell * slots - 1]) : 0u;
   const uint32_t pos0 = key_begin + (item - hs_uniform(item_first[cell])) * (uint32_t)HS_WORD_WAVE_KEYS;   // < key_end: the item exists
   const uint32_t lo = hs_uniform(first[cell]), hi = hs_uniform(first[cell + 1]);
   const int t0 = hesaff_plan::cells_first_tile(lo), t1 = hesaff_plan::cells_last_tile(hi);

   // a lane beyond the cell's last key reads that key again and stores nothing
   hs_v4i kf[2][4];
   int knorm[2];
   uint32_t kidx[2];
   hs_word_best best[2];
#pragma unroll
   for (int j = 0; j < 2; j++) {
      kidx[j] = perm[min(pos0 + 32u * j + (uint32_t)r, key_end - 1u)];
      const uint32_t key = PROBES ? hesaff_plan::cells_entry_key(kidx[j], (uint32_t)used) : kidx[j];
      hs_key_load(desc, (long long)key, stride, offset, h, kf[j]);
      knorm[j] = hs_key_norm(kf[j]);
      best[j].init(t0);
   }

   hs_word_stream(tiles, norms, t0, t1, lane, kf, [&](int t, int j, int (&score)[16]) {
      if (hesaff_plan::cells_tile_is_edge(t, lo, hi)) {   // (wave-uniform)
#pragma unroll
         for (int e = 0; e < 16; e++) {
            const uint32_t row = (uint32_t)t * HS_WORD_TILE + (uint32_t)hs_word_row(e, h);
            score[e] = hesaff_plan::cells_row_masked(row, lo, hi) ? 0x7fffffff : score[e];
         }
      }
      best[j].take(t, score);
   });

#pragma unroll
   for (int j = 0; j < 2; j++) {
      int bs, bk;
      best[j].reduce(h, bs, bk);
      if (h == 0 && pos0 + 32u * j + (uint32_t)r < key_end) {
         out[2 * (size_t)kidx[j]] = bk;
         out[2 * (size_t)kidx[j] + 1] = bs + knorm[j];
      }
   }
}

// The first step with probes (hesaff_set_vocabulary_probes): for every key its `probes` nearest coarse rows in the order (dist2, c)
// ascending - out[(key * probes + p)] = (cell, dist2) for rank p, the (word, dist2) rows the grouping reads, one per entry.  1 <= probes
// <= the real rows of the packed coarse layer (launch_probe_cells passes min(P, C)).
// The frame of kernels_words.h with the stream run `probes` times: the wave's 64 keys stay in registers, loaded once, and the coarse
// tiles are a few thousand rows: L2.  Sweep p is k_assign_words' search restricted to the rows whose (score, row) is lexicographically
// GREATER than the key's result of sweep p - 1: the visit masks a row at or below that threshold, so sweep p finds the least
// (score, row) above it - rank p of the order, ties included.  The threshold is per key, the key is the column, so it is per lane -
// two registers per key tile - and the same in lanes l and l ^ 32, which both keep the reduced result.  Before sweep 0 it is
// (INT_MIN, -1): every row is above it (|score| < 2^23, a pad row 2^30).  A pad row is above every threshold but never the least:
// p < probes <= C real rows remain above it, each below 2^23.  Plain loads and vector stores.
__global__ __launch_bounds__(HS_WORD_BLOCK_WAVES * 64) void k_probe_cells(const uint8_t *__restrict__ desc, long long n, long long stride, long long offset,
                                                                         const hs_v4i *__restrict__ tiles, const int32_t *__restrict__ norms, int n_tiles, int probes,
                                                                         int32_t *__restrict__ out)
{
   const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
   const int r = lane & 31, h = lane >> 5;
   const long long key0 = ((long long)blockIdx.x * HS_WORD_BLOCK_WAVES + wave) * HS_WORD_WAVE_KEYS;
   if (key0 >= n) return;   // (wave-uniform)

   // a lane beyond the last key reads the last key again and stores nothing
   hs_v4i kf[2][4];
   int knorm[2];
#pragma unroll
   for (int j = 0; j < 2; j++) {
      hs_key_load(desc, min(key0 + 32 * j + r, n - 1), stride, offset, h, kf[j]);
      knorm[j] = hs_key_norm(kf[j]);
   }

   int thr_s[2] = {(int)0x80000000, (int)0x80000000}, thr_k[2] = {-1, -1};   // the key's result of the sweep before
   for (int sweep = 0; sweep < probes; sweep++) {
      hs_word_best best[2];
#pragma unroll
      for (int j = 0; j < 2; j++) best[j].init(0);

      hs_word_stream(tiles, norms, 0, n_tiles - 1, lane, kf, [&](int t, int j, int (&score)[16]) {
#pragma unroll
         for (int e = 0; e < 16; e++) {
            const int row = t * HS_WORD_TILE + hs_word_row(e, h);
            // (score, row) > (thr_s, thr_k) lexicographically, without a branch: a row at or below thr_k has to beat thr_s by one.  No
            // overflow: thr_s is INT_MIN only beside thr_k = -1, which no row is at or below, and a sweep's result is below 2^23
            const bool above = score[e] >= thr_s[j] + (int)(row <= thr_k[j]);
            score[e] = above ? score[e] : 0x7fffffff;
         }
         best[j].take(t, score);
      });

#pragma unroll
      for (int j = 0; j < 2; j++) {
         best[j].reduce(h, thr_s[j], thr_k[j]);   // both halves keep the result as the next threshold
         const long long key = key0 + 32 * j + r;
         if (h == 0 && key < n) {
            const long long e = key * probes + sweep;
            out[2 * e] = thr_k[j];
            out[2 * e + 1] = thr_s[j] + knorm[j];
         }
      }
   }
}

// The last step with probes: a key's (word, dist2) is the lexicographic minimum of (dist2, row) over its `used` entries of fine[e][2] =
// (row, dist2), e = key * used + rank - a tie between rows of two probed cells goes to the lower row, whatever the ranks.
__global__ __launch_bounds__(256) void k_merge_probes(const int32_t *__restrict__ fine, int n, int used, int32_t *__restrict__ out)
{
   const int i = (int)(blockIdx.x * 256u + threadIdx.x);
   if (i >= n) return;
   const int2 *f = (const int2 *)fine + (size_t)i * (size_t)used;
   int2 b = f[0];
   for (int p = 1; p < used; p++) {
      const int2 v = f[p];
      if (v.y < b.y || (v.y == b.y && v.x < b.x)) b = v;
   }
   out[2 * (size_t)i] = b.x;   // (the caller's array: 4-byte aligned only)
   out[2 * (size_t)i + 1] = b.y;
}
