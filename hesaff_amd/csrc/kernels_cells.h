// kernels_cells.h -- visual-word assignment through vocabulary cells (hesaff_set_vocabulary_cells, include/hesaff_amd.h): a key is
// compared with the C coarse rows, then only with the rows of the cell it fell into - C + K / C exact distances instead of K.
//
// The steps (launch_assign_cells, pipeline.hip).  k_assign_words (kernels_words.h) runs unchanged against the packed coarse rows: (cell,
// dist2 to the coarse row) per key.  The keys are grouped by cell with the kernels of kernels_train.h as they are - k_word_histogram,
// exclusive_scan, k_word_scatter - into `perm`, a cell's keys neighbours, its range read off the cursor behind the scatter.  A cell with
// m keys makes ceil(m / 64) work items; a second scan (LoadCellItems) gives each cell's first item and the total.  The order of the keys
// inside a cell depends on which wave came first: no result below depends on it.
//
// k_assign_words_cells: a wavefront owns one work item, up to 64 keys of ONE cell gathered through perm, and keeps their bytes in
// registers by k_assign_words' fragment rule.  The grid is sized by the host's bound, floor(n / 64) + C (cells_plan.h); a wave beyond
// the device's total returns; a wave finds its cell by binary search in the item offsets (wave-uniform: scalar loads).  It streams
// tiles first[c] / 32 .. (first[c + 1] - 1) / 32 of the context's flat packed vocabulary - the layout on the device is the flat
// kernel's - with four v_mfma_i32_32x32x32_i8 per key tile and word tile and the same running (score, tile) on strict <.  Only a
// cell's first and last tile can hold rows of other cells: there (a wave-uniform branch) a row outside [first[c], first[c + 1]) scores
// 0x7fffffff, which cannot replace the initial best on strict <, and a cell has at least one real row, so the minimum is a row of the
// cell.  The final reduction is the flat kernel's lexicographic (score, k); each key's 8 bytes go to its own index.  Plain loads and
// vector stores, no atomics: every result is a function of the key alone.
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

   // the keys' fragments and the lane's half of |d'|^2; a lane beyond the cell's last key reads that key again and stores nothing
   hs_v4i kf[2][4];
   int knorm[2];
   uint32_t kidx[2];
#pragma unroll
   for (int j = 0; j < 2; j++) {
      kidx[j] = perm[min(pos0 + 32u * j + (uint32_t)r, key_end - 1u)];
      const uint32_t key = PROBES ? hesaff_plan::cells_entry_key(kidx[j], (uint32_t)used) : kidx[j];
      const uint32_t *p = (const uint32_t *)(desc + (long long)key * stride + offset + 16 * h);
      int sq = 0;
#pragma unroll
      for (int s = 0; s < 4; s++)
#pragma unroll
         for (int q = 0; q < 4; q++) {
            const uint32_t v = p[8 * s + q] ^ 0x80808080u;
            kf[j][s][q] = (int)v;
            sq += hs_sq4_i8(v);
         }
      knorm[j] = sq + __shfl_xor(sq, 32, 64);
   }

   int best[2][16], best_t[2][16];
#pragma unroll
   for (int j = 0; j < 2; j++)
#pragma unroll
      for (int e = 0; e < 16; e++) { best[j][e] = 0x7fffffff; best_t[j][e] = t0; }

   // tile t's operand fragments and the norms of the lane's 16 rows (rows 8 g + 4 h .. + 3 for g = 0..3), loaded one tile ahead
   hs_v4i a[4], nr[4];
#pragma unroll
   for (int s = 0; s < 4; s++) a[s] = tiles[((size_t)t0 * 4 + s) * 64 + lane];
#pragma unroll
   for (int g = 0; g < 4; g++) nr[g] = *(const hs_v4i *)(norms + (size_t)t0 * HS_WORD_TILE + 8 * g + 4 * h);
   for (int t = t0; t <= t1; t++) {
      hs_v4i a_next[4], nr_next[4];
      const int tn = min(t + 1, t1);
#pragma unroll
      for (int s = 0; s < 4; s++) a_next[s] = tiles[((size_t)tn * 4 + s) * 64 + lane];
#pragma unroll
      for (int g = 0; g < 4; g++) nr_next[g] = *(const hs_v4i *)(norms + (size_t)tn * HS_WORD_TILE + 8 * g + 4 * h);
      const bool edge = hesaff_plan::cells_tile_is_edge(t, lo, hi);   // (wave-uniform)
#pragma unroll
      for (int j = 0; j < 2; j++) {
         hs_v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
         for (int s = 0; s < 4; s++) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s], kf[j][s], acc, 0, 0, 0);
         int score[16];
#pragma unroll
         for (int e = 0; e < 16; e++) score[e] = nr[e >> 2][e & 3] - 2 * acc[e];
         if (edge) {
#pragma unroll
            for (int e = 0; e < 16; e++) {
               const uint32_t row = (uint32_t)t * HS_WORD_TILE + (uint32_t)((e & 3) + 8 * (e >> 2) + 4 * h);
               score[e] = hesaff_plan::cells_row_masked(row, lo, hi) ? 0x7fffffff : score[e];
            }
         }
#pragma unroll
         for (int e = 0; e < 16; e++) {
            const bool less = score[e] < best[j][e];
            best[j][e] = less ? score[e] : best[j][e];
            best_t[j][e] = less ? t : best_t[j][e];
         }
      }
#pragma unroll
      for (int s = 0; s < 4; s++) a[s] = a_next[s];
#pragma unroll
      for (int g = 0; g < 4; g++) nr[g] = nr_next[g];
   }

#pragma unroll
   for (int j = 0; j < 2; j++) {
      // the lane's 16 rows, then the other half's: (score, k) lexicographically
      int bs = 0x7fffffff, bk = 0x7fffffff;
#pragma unroll
      for (int e = 0; e < 16; e++) {
         const int k = best_t[j][e] * HS_WORD_TILE + (e & 3) + 8 * (e >> 2) + 4 * h;
         const bool less = best[j][e] < bs || (best[j][e] == bs && k < bk);
         bs = less ? best[j][e] : bs;
         bk = less ? k : bk;
      }
      const int os = __shfl_xor(bs, 32, 64), ok = __shfl_xor(bk, 32, 64);
      if (os < bs || (os == bs && ok < bk)) { bs = os; bk = ok; }
      if (h == 0 && pos0 + 32u * j + (uint32_t)r < key_end) {
         out[2 * (size_t)kidx[j]] = bk;
         out[2 * (size_t)kidx[j] + 1] = bs + knorm[j];
      }
   }
}

// The first step with probes (hesaff_set_vocabulary_probes): for every key its `probes` nearest coarse rows in the order (dist2, c)
// ascending - out[(key * probes + p)] = (cell, dist2) for rank p, the (word, dist2) rows the grouping reads, one per entry.  1 <= probes
// <= the real rows of the packed coarse layer (launch_probe_cells passes min(P, C)).
// k_assign_words' structure: the wave's 64 keys stay in registers, loaded once, and the coarse tiles (a few thousand rows: L2) are
// streamed `probes` times.  Sweep p is k_assign_words' search restricted to the rows whose (score, row) is lexicographically GREATER
// than the key's result of sweep p - 1: a row at or below that threshold scores 0x7fffffff, which cannot replace a running best on
// strict <, so sweep p finds the least (score, row) above the threshold - rank p of the order, ties included.  The threshold is per
// key, the key is the column, so it is per lane - two registers per key tile - and the same in lanes l and l ^ 32, which both keep the
// reduced result.  Before sweep 0 it is (INT_MIN, -1): every row is above it (|score| < 2^23, a pad row 2^30).  A pad row is above
// every threshold but never the least: p < probes <= C real rows remain above it, each below 2^23.  Plain loads and vector stores.
__global__ __launch_bounds__(HS_WORD_BLOCK_WAVES * 64) void k_probe_cells(const uint8_t *__restrict__ desc, long long n, long long stride, long long offset,
                                                                         const hs_v4i *__restrict__ tiles, const int32_t *__restrict__ norms, int n_tiles, int probes,
                                                                         int32_t *__restrict__ out)
{
   const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
   const int r = lane & 31, h = lane >> 5;
   const long long key0 = ((long long)blockIdx.x * HS_WORD_BLOCK_WAVES + wave) * HS_WORD_WAVE_KEYS;
   if (key0 >= n) return;   // (wave-uniform)

   // the keys' fragments and the lane's half of |d'|^2; a lane beyond the last key reads the last key again and stores nothing
   hs_v4i kf[2][4];
   int knorm[2];
#pragma unroll
   for (int j = 0; j < 2; j++) {
      const long long key = min(key0 + 32 * j + r, n - 1);
      const uint32_t *p = (const uint32_t *)(desc + key * stride + offset + 16 * h);
      int sq = 0;
#pragma unroll
      for (int s = 0; s < 4; s++)
#pragma unroll
         for (int q = 0; q < 4; q++) {
            const uint32_t v = p[8 * s + q] ^ 0x80808080u;
            kf[j][s][q] = (int)v;
            sq += hs_sq4_i8(v);
         }
      knorm[j] = sq + __shfl_xor(sq, 32, 64);
   }

   int thr_s[2] = {(int)0x80000000, (int)0x80000000}, thr_k[2] = {-1, -1};   // the key's result of the sweep before
   for (int sweep = 0; sweep < probes; sweep++) {
      int best[2][16], best_t[2][16];
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
         for (int e = 0; e < 16; e++) { best[j][e] = 0x7fffffff; best_t[j][e] = 0; }

      // tile t's operand fragments and the norms of the lane's 16 rows, loaded one tile ahead (as in k_assign_words)
      hs_v4i a[4], nr[4];
#pragma unroll
      for (int s = 0; s < 4; s++) a[s] = tiles[(size_t)s * 64 + lane];
#pragma unroll
      for (int g = 0; g < 4; g++) nr[g] = *(const hs_v4i *)(norms + 8 * g + 4 * h);
      for (int t = 0; t < n_tiles; t++) {
         hs_v4i a_next[4], nr_next[4];
         const int tn = min(t + 1, n_tiles - 1);
#pragma unroll
         for (int s = 0; s < 4; s++) a_next[s] = tiles[((size_t)tn * 4 + s) * 64 + lane];
#pragma unroll
         for (int g = 0; g < 4; g++) nr_next[g] = *(const hs_v4i *)(norms + (size_t)tn * HS_WORD_TILE + 8 * g + 4 * h);
#pragma unroll
         for (int j = 0; j < 2; j++) {
            hs_v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int s = 0; s < 4; s++) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s], kf[j][s], acc, 0, 0, 0);
#pragma unroll
            for (int e = 0; e < 16; e++) {
               const int row = t * HS_WORD_TILE + (e & 3) + 8 * (e >> 2) + 4 * h;
               const int raw = nr[e >> 2][e & 3] - 2 * acc[e];
               const bool above = raw > thr_s[j] || (raw == thr_s[j] && row > thr_k[j]);
               const int score = above ? raw : 0x7fffffff;
               const bool less = score < best[j][e];
               best[j][e] = less ? score : best[j][e];
               best_t[j][e] = less ? t : best_t[j][e];
            }
         }
#pragma unroll
         for (int s = 0; s < 4; s++) a[s] = a_next[s];
#pragma unroll
         for (int g = 0; g < 4; g++) nr[g] = nr_next[g];
      }

#pragma unroll
      for (int j = 0; j < 2; j++) {
         // the lane's 16 rows, then the other half's: (score, k) lexicographically; both halves keep the result as the next threshold
         int bs = 0x7fffffff, bk = 0x7fffffff;
#pragma unroll
         for (int e = 0; e < 16; e++) {
            const int k = best_t[j][e] * HS_WORD_TILE + (e & 3) + 8 * (e >> 2) + 4 * h;
            const bool less = best[j][e] < bs || (best[j][e] == bs && k < bk);
            bs = less ? best[j][e] : bs;
            bk = less ? k : bk;
         }
         const int os = __shfl_xor(bs, 32, 64), ok = __shfl_xor(bk, 32, 64);
         if (os < bs || (os == bs && ok < bk)) { bs = os; bk = ok; }
         thr_s[j] = bs; thr_k[j] = bk;
         const long long key = key0 + 32 * j + r;
         if (h == 0 && key < n) {
            const long long e = key * probes + sweep;
            out[2 * e] = bk;
            out[2 * e + 1] = bs + knorm[j];
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
