// kernels_words.h -- visual-word assignment (hesaff_set_vocabulary, include/hesaff_amd.h): for every key the LOWEST row k of the
// vocabulary that minimises dist2(k) = sum_j (d[j] - w_k[j])^2 over the 128 descriptor bytes, and that distance.  Integers only:
// with d' = d ^ 0x80 and w' = w ^ 0x80 read as signed bytes (the values minus 128), dist2(k) = |d'|^2 + |w'_k|^2 - 2 d'.w'_k, every
// term fits int32 (|d'.w'| <= 2^21), and the dot products are what the i8 matrix instruction computes without rounding.
//
// k_assign_words: a wavefront owns 64 keys (two 32-key column tiles) and keeps their bytes in registers - 2 x 16 VGPRs - for the
// whole vocabulary.  It streams the vocabulary in tiles of 32 rows in increasing k: four v_mfma_i32_32x32x32_i8 per key tile give the
// 32 x 32 dot products of a word tile (rows) with a key tile (columns), and per accumulator element a running (best score, best
// tile) is replaced on strict < only, so the lowest k survives inside an element; score = |w'_k|^2 - 2 d'.w'_k.  The key is the
// COLUMN of C (lane & 31), so a key's 32 rows of a tile live in the 16 registers of two lanes: the final reduction compares
// (score, k) lexicographically over the registers of a lane and once across lanes l and l ^ 32.
//
// Operand order: a dot product does not care in which order the 32 byte positions of a k-step are summed, as long as both operands
// of the step hold the same positions in the same lane group.  Both are loaded by ONE rule - lane l (r = l & 31, h = l >> 5) holds, for
// step s, bytes [32 s + 16 h, 32 s + 16 h + 16) of row / column r - so whatever the byte order inside an operand fragment is, the
// sums are right.  Which (word, key) pair an accumulator element is follows the C/D map that all gfx950 MFMA shapes share:
// column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
//
// The vocabulary as the device holds it (pack_vocabulary, host): XORed already, padded to whole tiles, and laid out in the order the
// lanes read it - tile t, step s, lane l: 16 bytes at ((t * 4 + s) * 64 + l) * 16 - so a step's operand is one coalesced 1 KB read; and
// one int32 |w'_k|^2 per row.  A pad row is all zero with norm 2^30: its score, 2^30, cannot overflow and cannot be the minimum
// while a real row exists (a real score is at most 128 * 128^2 + 2 * 2^21 < 2^23).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define HS_WORD_TILE 32                 // vocabulary rows per tile (the M of the MFMA)
#define HS_WORD_PAD_NORM (1 << 30)      // |w'|^2 of a pad row
#define HS_WORD_WAVE_KEYS 64            // keys of a wavefront: two column tiles
#define HS_WORD_BLOCK_WAVES 4
#define HS_WORD_BLOCK_KEYS (HS_WORD_WAVE_KEYS * HS_WORD_BLOCK_WAVES)
#define HS_WORD_TILE_BYTES (HS_WORD_TILE * 128)

typedef int hs_v4i __attribute__((ext_vector_type(4)));
typedef int hs_v16i __attribute__((ext_vector_type(16)));

// sum of the squares of the four signed bytes of v
__device__ __forceinline__ int hs_sq4_i8(uint32_t v)
{
   const int b0 = (int)(int8_t)(v & 0xffu), b1 = (int)(int8_t)((v >> 8) & 0xffu), b2 = (int)(int8_t)((v >> 16) & 0xffu), b3 = (int)(int8_t)(v >> 24);
   return b0 * b0 + b1 * b1 + b2 * b2 + b3 * b3;
}

// desc: key i's 128 descriptor bytes start at desc + i * stride + offset (stride, offset and desc multiples of 4: key records are
// 164 bytes apart with the descriptor 36 bytes in).  tiles / norms: the packed vocabulary of n_tiles tiles.  out: (word, dist2) per key.
__global__ __launch_bounds__(HS_WORD_BLOCK_WAVES * 64) void k_assign_words(const uint8_t *__restrict__ desc, long long n, long long stride, long long offset,
                                                                          const hs_v4i *__restrict__ tiles, const int32_t *__restrict__ norms, int n_tiles,
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

   int best[2][16], best_t[2][16];
#pragma unroll
   for (int j = 0; j < 2; j++)
#pragma unroll
      for (int e = 0; e < 16; e++) { best[j][e] = 0x7fffffff; best_t[j][e] = 0; }

   // tile t's operand fragments and the norms of the lane's 16 rows (rows 8 g + 4 h .. + 3 for g = 0..3), loaded one tile ahead
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
            const int score = nr[e >> 2][e & 3] - 2 * acc[e];
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
      const long long key = key0 + 32 * j + r;
      if (h == 0 && key < n) {
         out[2 * key] = bk;
         out[2 * key + 1] = bs + knorm[j];
      }
   }
}
