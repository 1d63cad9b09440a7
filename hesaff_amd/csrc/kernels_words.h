// kernels_words.h -- visual-word assignment (hesaff_set_vocabulary, include/hesaff_amd.h): for every key the LOWEST row k of the
// vocabulary that minimises dist2(k) = sum_j (d[j] - w_k[j])^2 over the 128 descriptor bytes, and that distance.  Integers only:
// with d' = d ^ 0x80 and w' = w ^ 0x80 read as signed bytes (the values minus 128), dist2(k) = |d'|^2 + |w'_k|^2 - 2 d'.w'_k, every
// term fits int32 (|d'.w'| <= 2^21), and the dot products are what the i8 matrix instruction computes without rounding.
//
// THE FRAME, which k_assign_words, k_assign_words_cells, k_probe_cells (kernels_cells.h) and k_assign_neighbours
// (kernels_neighbours.h) share; each of them adds its indexing, a visit and its stores.
//
// Keys (hs_key_load, hs_key_norm): a wavefront owns 64 keys (two 32-key column tiles) and keeps their bytes in registers - 2 x 16
// VGPRs - while the vocabulary goes by.  The key is the COLUMN of C (lane & 31).
//
// Stream (hs_word_stream): tiles t0 .. t1 of 32 rows in increasing k, loaded one tile ahead: four v_mfma_i32_32x32x32_i8 per key tile
// give the 32 x 32 dot products of a word tile (rows) with a key tile (columns), and the lane's 16 scores, score = |w'_k|^2 -
// 2 d'.w'_k, go to the caller's visit(t, j, score).
//
// Running best (hs_word_best): per accumulator element a (best score, best tile) replaced on strict < only, so the lowest k survives
// inside an element.  A key's 32 rows of a tile live in the 16 registers of two lanes: the final reduction compares (score, k)
// lexicographically over the registers of a lane and once across lanes l and l ^ 32.
//
// Operand order: a dot product does not care in which order the 32 byte positions of a k-step are summed, as long as both operands
// of the step hold the same positions in the same lane group.  Both are loaded by ONE rule - lane l (r = l & 31, h = l >> 5) holds, for
// step s, bytes [32 s + 16 h, 32 s + 16 h + 16) of row / column r - so whatever the byte order inside an operand fragment is, the
// sums are right.  Which (word, key) pair an accumulator element is follows the C/D map that all gfx950 MFMA shapes share:
// column = lane & 31, row = hs_word_row(reg, lane >> 5).
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
#define HS_WORD_TILE_BYTES (HS_WORD_TILE * 128)

typedef int hs_v4i __attribute__((ext_vector_type(4)));
typedef int hs_v16i __attribute__((ext_vector_type(16)));

// sum of the squares of the four signed bytes of v
__device__ __forceinline__ int hs_sq4_i8(uint32_t v)
{
   const int b0 = (int)(int8_t)(v & 0xffu), b1 = (int)(int8_t)((v >> 8) & 0xffu), b2 = (int)(int8_t)((v >> 16) & 0xffu), b3 = (int)(int8_t)(v >> 24);
   return b0 * b0 + b1 * b1 + b2 * b2 + b3 * b3;
}

// the row, inside its tile, of accumulator element e in a lane of half h; elements 4 g .. 4 g + 3 are four rows in a run
__device__ __forceinline__ int hs_word_row(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

// the lane's fragments of one key, XORed: the key's 128 descriptor bytes start at desc + key * stride + offset (stride, offset and desc
// multiples of 4: key records are 164 bytes apart with the descriptor 36 bytes in).  key: clamped or gathered by the caller.
__device__ __forceinline__ void hs_key_load(const uint8_t *__restrict__ desc, long long key, long long stride, long long offset, int h, hs_v4i (&kf)[4])
{
   const uint32_t *p = (const uint32_t *)(desc + key * stride + offset + 16 * h);
#pragma unroll
   for (int s = 0; s < 4; s++)
#pragma unroll
      for (int q = 0; q < 4; q++) kf[s][q] = (int)(p[8 * s + q] ^ 0x80808080u);
}

// |d'|^2 of the key whose fragments the lane and lane l ^ 32 hold (all lanes take part in the exchange)
__device__ __forceinline__ int hs_key_norm(const hs_v4i (&kf)[4])
{
   int sq = 0;
#pragma unroll
   for (int s = 0; s < 4; s++)
#pragma unroll
      for (int q = 0; q < 4; q++) sq += hs_sq4_i8((uint32_t)kf[s][q]);
   return sq + __shfl_xor(sq, 32, 64);
}

// Tiles t0 <= t1 of a packed vocabulary (tiles / norms) against the wave's two key tiles kf: visit(t, j, score) receives, for tile t
// and key tile j, the lane's 16 scores - element e is row t * HS_WORD_TILE + hs_word_row(e, h) - and may overwrite them.
template <class Visit>
__device__ __forceinline__ void hs_word_stream(const hs_v4i *__restrict__ tiles, const int32_t *__restrict__ norms, int t0, int t1, int lane,
                                               const hs_v4i (&kf)[2][4], Visit visit)
{
   // tile t's operand, fragment s in elements 4 s .. 4 s + 3, and the norms of the lane's 16 rows, four runs of four.  The operand is
   // ONE value: as four separate fragments the compiler folds the load of a single-block loop (k_assign_words') back into the
   // iteration that uses it, and the prefetch is gone - 13 % of that kernel's time (the frame).  The norms it may move: they
   // are needed behind the MFMAs only
   const auto load = [&](int t, hs_v16i &a, hs_v4i (&nr)[4]) {
#pragma unroll
      for (int s = 0; s < 4; s++) {
         const hs_v4i f = tiles[((size_t)t * 4 + s) * 64 + lane], g = *(const hs_v4i *)(norms + (size_t)t * HS_WORD_TILE + hs_word_row(4 * s, lane >> 5));
#pragma unroll
         for (int q = 0; q < 4; q++) a[4 * s + q] = f[q];
         nr[s] = g;
      }
   };
   hs_v16i a;
   hs_v4i nr[4];
   load(t0, a, nr);
   for (int t = t0; t <= t1; t++) {
      hs_v16i a_next;
      hs_v4i nr_next[4];
      load(min(t + 1, t1), a_next, nr_next);   // one tile ahead; the last tile again behind the last
#pragma unroll
      for (int j = 0; j < 2; j++) {
         hs_v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
         for (int s = 0; s < 4; s++) {
            const hs_v4i f = {a[4 * s], a[4 * s + 1], a[4 * s + 2], a[4 * s + 3]};
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(f, kf[j][s], acc, 0, 0, 0);
         }
         int score[16];
#pragma unroll
         for (int e = 0; e < 16; e++) score[e] = nr[e >> 2][e & 3] - 2 * acc[e];
         visit(t, j, score);
      }
      a = a_next;
#pragma unroll
      for (int g = 0; g < 4; g++) nr[g] = nr_next[g];
   }
}

// The running best of one key tile: a lane's 16 x (score, tile).  A score of 0x7fffffff never replaces one: that is how a visit masks.
struct hs_word_best {
   int s[16], t[16];
   // t0: a tile of the stream (its first: every k the reduction can form is then a row the stream covers)
   __device__ __forceinline__ void init(int t0)
   {
#pragma unroll
      for (int e = 0; e < 16; e++) { s[e] = 0x7fffffff; t[e] = t0; }
   }
   __device__ __forceinline__ void take(int tile, const int (&score)[16])
   {
#pragma unroll
      for (int e = 0; e < 16; e++) {
         const bool less = score[e] < s[e];
         s[e] = less ? score[e] : s[e];
         t[e] = less ? tile : t[e];
      }
   }
   // the lane's 16 rows, then the other half's: the least (score, k) lexicographically, in both lanes of the key
   __device__ __forceinline__ void reduce(int h, int &bs, int &bk) const
   {
      bs = 0x7fffffff; bk = 0x7fffffff;
#pragma unroll
      for (int e = 0; e < 16; e++) {
         const int k = t[e] * HS_WORD_TILE + hs_word_row(e, h);
         const bool less = s[e] < bs || (s[e] == bs && k < bk);
         bs = less ? s[e] : bs;
         bk = less ? k : bk;
      }
      const int os = __shfl_xor(bs, 32, 64), ok = __shfl_xor(bk, 32, 64);
      if (os < bs || (os == bs && ok < bk)) { bs = os; bk = ok; }
   }
};

// desc, stride, offset: as for hs_key_load.  tiles / norms: the packed vocabulary of n_tiles tiles.  out: (word, dist2) per key.
// Grid: one wavefront per 64 keys, HS_WORD_BLOCK_WAVES to a block.
__global__ __launch_bounds__(HS_WORD_BLOCK_WAVES * 64) void k_assign_words(const uint8_t *__restrict__ desc, long long n, long long stride, long long offset,
                                                                          const hs_v4i *__restrict__ tiles, const int32_t *__restrict__ norms, int n_tiles,
                                                                          int32_t *__restrict__ out)
{
   const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
   const int r = lane & 31, h = lane >> 5;
   const long long key0 = ((long long)blockIdx.x * HS_WORD_BLOCK_WAVES + wave) * HS_WORD_WAVE_KEYS;
   if (key0 >= n) return;   // (wave-uniform)

   // a lane beyond the last key reads the last key again and stores nothing
   hs_v4i kf[2][4];
   int knorm[2];
   hs_word_best best[2];
#pragma unroll
   for (int j = 0; j < 2; j++) {
      hs_key_load(desc, min(key0 + 32 * j + r, n - 1), stride, offset, h, kf[j]);
      knorm[j] = hs_key_norm(kf[j]);
      best[j].init(0);
   }

   hs_word_stream(tiles, norms, 0, n_tiles - 1, lane, kf, [&](int t, int j, int (&score)[16]) { best[j].take(t, score); });

#pragma unroll
   for (int j = 0; j < 2; j++) {
      int bs, bk;
      best[j].reduce(h, bs, bk);
      const long long key = key0 + 32 * j + r;
      if (h == 0 && key < n) {
         out[2 * key] = bk;
         out[2 * key + 1] = bs + knorm[j];
      }
   }
}
