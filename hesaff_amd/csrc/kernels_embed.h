// kernels_embed.h -- Hamming embedding (hesaff_set_embedding, hesaff_train_embedding, hesaff_index_build_embedded and
// hesaff_index_query_embedded of include/hesaff_amd.h): a 64-bit signature per key that places the key inside its word's cell, and
// a word match that counts only where two signatures lie within a Hamming threshold.  Integers only: z = P.d is what the i8 matrix
// instruction computes without rounding, a signature bit is a strict integer compare, the thresholds are exact lower medians, and the
// query adds with integer atomics - no result depends on the launch geometry or on which wave ran first.
//
// k_embed_keys: a wavefront owns 64 keys (two 32-key column tiles) under k_assign_words' fragment rules (kernels_words.h): lane l
// (r = l & 31, h = l >> 5) holds, for step s, bytes [32 s + 16 h, + 16) of key r, XORed with 0x80 (d' = d - 128 as signed bytes).  P
// is packed once (embed_pack_projection, embed_plan.h) as two 32-row tiles in the same lane order, not XORed: it is signed already.
// Eight v_mfma_i32_32x32x32_i8 per key tile give P.d' for the 64 rows and 32 keys; z = P.d' + bias[row], bias = 128 * rowsum(P), and
// every term stays inside int32 (|P.d'|, |bias| < 2^21).  Accumulator element e of lane l is row hs_word_row(e, h) of the
// tile and key r: a lane holds 16 rows per tile of its key, in four runs of four, so it reads its key's thresholds tau[word][..] - 256
// contiguous bytes per key - as four 16-byte loads per tile, folds its compares into a 64-bit mask, ORs it with lane l ^ 32's (the
// other 32 rows) and the lower lane writes the key's 8 bytes.  RAW: the test seam, z itself instead of the bits.
//
// Threshold training.  k_embed_keys<true> writes z[n][64]; the keys are grouped by word with k_word_histogram, exclusive_scan and
// k_word_scatter (kernels_train.h); k_embed_medians then runs one block per word, lane = bit: a wave walks every fourth key of the word
// and reads its 256-byte row of z as one coalesced load.  The lower median - element (m - 1) / 2 in ascending order - is found by a
// most-significant-bit-first radix select over u = z + 2^22 (23 bits, embed_plan.h) with one-bit digits: a pass counts, per bit column,
// the values that match the prefix found so far and have a 0 in the pass's bit; the counts of the four waves meet in LDS; if the rank
// lies below the count the bit is 0, otherwise the rank drops by the count and the bit is 1.  Counting is exact and commutative, so
// neither the order of the keys inside a word (which depends on which wave came first) nor the block's shape shows in the result.
//
// Key lists of an embedded index: the count of every word's keys (k_word_histogram, one counter per word), exclusive_scan, and
// k_keylist_scatter writes (image, signature) to the next free place of the word's list - structure of arrays, so that a signature is
// an aligned 8-byte load.  The order inside a list depends on which wave came first; only sums over a list are ever output.
//
// k_query_score_embedded: one wavefront per query key, as k_query_score (kernels_index.h).  The tfq exchange still decides which wave
// of a word adds (t idf)^2 to nq2 and still leaves tfq zero for the next query; but EVERY wave walks its word's key list (unless idf
// is 0), its lanes striding it, and each entry within the Hamming threshold adds idf^2 to dot[image].
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "embed_plan.h"
#include "kernels_index.h"
#include "kernels_train.h"
#include "kernels_words.h"

#define HS_EMBED_BLOCK_WAVES 4
#define HS_EMBED_WAVE_KEYS 64

// desc: key i's 128 descriptor bytes at desc + i * stride + offset (multiples of 4).  words: key i's word at words[i * word_stride],
// inside 0 .. K - 1 (checked by the caller).  tiles / bias: the packed projection.  tau [K][64].  out: a uint64 per key, or with RAW
// int32 z[n][64] (words and tau are not read).  Grid: ceil(n / 256) blocks of 256.
template <bool RAW>
__global__ __launch_bounds__(HS_EMBED_BLOCK_WAVES * 64) void k_embed_keys(const uint8_t *__restrict__ desc, long long n, long long stride, long long offset,
                                                                         const int32_t *__restrict__ words, int word_stride,
                                                                         const hs_v4i *__restrict__ tiles, const int32_t *__restrict__ bias,
                                                                         const int32_t *__restrict__ tau, void *__restrict__ out)
{
   const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
   const int r = lane & 31, h = lane >> 5;
   const long long key0 = ((long long)blockIdx.x * HS_EMBED_BLOCK_WAVES + wave) * HS_EMBED_WAVE_KEYS;
   if (key0 >= n) return;   // (wave-uniform)

   // P's fragments: tile t, step s
   hs_v4i a[2][4];
#pragma unroll
   for (int t = 0; t < 2; t++)
#pragma unroll
      for (int s = 0; s < 4; s++) a[t][s] = tiles[(size_t)(t * 4 + s) * 64 + lane];
   // the bias of the lane's 16 rows of a tile: four runs of four
   hs_v4i bs[2][4];
#pragma unroll
   for (int t = 0; t < 2; t++)
#pragma unroll
      for (int g = 0; g < 4; g++) bs[t][g] = *(const hs_v4i *)(bias + 32 * t + hs_word_row(4 * g, h));

#pragma unroll
   for (int j = 0; j < 2; j++) {
      // a lane beyond the last key reads the last key again and stores nothing
      const long long key = key0 + 32 * j + r;
      const long long src = min(key, n - 1);
      hs_v4i kf[4];
      hs_key_load(desc, src, stride, offset, h, kf);
      const int32_t *th = RAW ? nullptr : tau + (size_t)words[(size_t)src * word_stride] * 64;
      unsigned long long bits = 0ull;
#pragma unroll
      for (int t = 0; t < 2; t++) {
         hs_v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
         for (int s = 0; s < 4; s++) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[t][s], kf[s], acc, 0, 0, 0);
#pragma unroll
         for (int g = 0; g < 4; g++) {
            const int row0 = 32 * t + hs_word_row(4 * g, h);   // the lane's rows row0 .. row0 + 3: accumulator elements 4 g .. 4 g + 3
            if (RAW) {
               if (key < n) {
                  hs_v4i z;
#pragma unroll
                  for (int q = 0; q < 4; q++) z[q] = acc[4 * g + q] + bs[t][g][q];
                  *(hs_v4i *)((int32_t *)out + (size_t)key * 64 + row0) = z;
               }
            } else {
               const hs_v4i tv = *(const hs_v4i *)(th + row0);
#pragma unroll
               for (int q = 0; q < 4; q++)
                  if (acc[4 * g + q] + bs[t][g][q] > tv[q]) bits |= 1ull << (row0 + q);
            }
         }
      }
      if (!RAW) {
         // the other half of the key's rows lives in lane l ^ 32
         const uint32_t lo = (uint32_t)bits, hi = (uint32_t)(bits >> 32);
         const uint32_t olo = (uint32_t)__shfl_xor((int)lo, 32, 64), ohi = (uint32_t)__shfl_xor((int)hi, 32, 64);
         if (h == 0 && key < n) ((unsigned long long *)out)[key] = bits | (unsigned long long)olo | ((unsigned long long)ohi << 32);
      }
   }
}

#define HS_EMBED_MEDIAN_WAVES 4

// One block per word, lane = bit.  cursor [K][slots]: the ends of the word's entries behind k_word_scatter, so word w's keys are
// perm[end of word w - 1 .. end of word w).  z [n][64].  tau[w][bit]: the lower median of the word's z[.][bit], 0 for a word
// without keys; counts[w] = its keys.  Grid: K blocks of 256.
__global__ __launch_bounds__(HS_EMBED_MEDIAN_WAVES * 64) void k_embed_medians(const int32_t *__restrict__ z, const uint32_t *__restrict__ perm,
                                                                             const uint32_t *__restrict__ cursor, int slots, int32_t *__restrict__ tau,
                                                                             uint32_t *__restrict__ counts)
{
   __shared__ uint32_t s_cnt[HS_EMBED_MEDIAN_WAVES][64];
   const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
   const size_t w = blockIdx.x;
   const uint32_t begin = w > 0 ? cursor[w * (size_t)slots - 1] : 0u, end = cursor[w * (size_t)slots + (size_t)slots - 1];
   const uint32_t m = end - begin;
   if (threadIdx.x == 0) counts[w] = m;
   if (m == 0u) {   // (block-uniform)
      if (wave == 0) tau[w * 64 + lane] = 0;
      return;
   }
   uint32_t rank = hesaff_plan::embed_median_rank(m), prefix = 0u;
   for (int b = hesaff_plan::HS_EMBED_Z_BITS - 1; b >= 0; b--) {
      // the wave's keys: every fourth of the word.  A value counts where its bits above b equal the prefix's and its bit b is 0.
      uint32_t c0 = 0u;
      for (uint32_t p = begin + (uint32_t)wave; p < end; p += HS_EMBED_MEDIAN_WAVES) {
         const uint32_t u = (uint32_t)(z[(size_t)perm[p] * 64 + lane] + hesaff_plan::HS_EMBED_Z_BIAS);
         c0 += (((u ^ prefix) >> b) == 0u) ? 1u : 0u;   // (prefix's bits b and below are still 0: the shift keeps bit b of u)
      }
      s_cnt[wave][lane] = c0;
      __syncthreads();
      uint32_t zeros = 0u;
#pragma unroll
      for (int v = 0; v < HS_EMBED_MEDIAN_WAVES; v++) zeros += s_cnt[v][lane];
      __syncthreads();
      if (rank >= zeros) { rank -= zeros; prefix |= 1u << b; }
   }
   if (wave == 0) tau[w * 64 + lane] = (int32_t)prefix - hesaff_plan::HS_EMBED_Z_BIAS;
}

// Key j (of image base + hs_index_image_of: a build numbers its images from 0, an add from the images of the index so far) goes to
// its word's list.  cursor[k]: each list's next free position on entry - a copy of the offsets, or behind the old keys
// (k_keylist_merge, kernels_index_grow.h) - its end afterwards.  Grid: ceil(total / 256) blocks of 256.
__global__ __launch_bounds__(256) void k_keylist_scatter(const int32_t *__restrict__ words, int word_stride, const unsigned long long *__restrict__ sigs,
                                                         const uint32_t *__restrict__ starts, int n_images, uint32_t total, uint32_t base,
                                                         uint32_t *__restrict__ cursor, unsigned long long *__restrict__ list_sig, uint32_t *__restrict__ list_image)
{
   const uint32_t j = blockIdx.x * 256u + threadIdx.x;
   const bool live = j < total;
   const int w = live ? words[(size_t)j * word_stride] : -1;
   const uint32_t pos = hs_claim_per_word(cursor, w, live);
   if (live) {
      list_sig[pos] = sigs[j];
      list_image[pos] = base + hs_index_image_of(starts, n_images, j);
   }
}

// A wave's walk of one word's keys, entries first .. end - 1 of the lists, its lanes striding them: every entry whose signature lies
// within `threshold` bits of sig adds ff = idf^2 to row[image] (the dot of the query, or the query's row of a chunk's)
__device__ __forceinline__ void hs_keylist_walk(int lane, uint32_t first, uint32_t end, const unsigned long long *__restrict__ list_sig,
                                                const uint32_t *__restrict__ list_image, unsigned long long sig, int threshold, unsigned long long ff,
                                                unsigned long long *__restrict__ row)
{
   for (uint32_t p = first + (uint32_t)lane; p < end; p += 64u)
      if (__popcll(sig ^ list_sig[p]) <= threshold) atomicAdd(&row[list_image[p]], ff);
}

// One wavefront per query key; dot zeroed, head->nq2 zero on entry, tfq filled by k_query_count.  Grid: ceil(n / 4) blocks of 256.
__global__ __launch_bounds__(256) void k_query_score_embedded(const int32_t *__restrict__ words, int word_stride, const unsigned long long *__restrict__ sigs,
                                                              int n, int threshold, uint32_t *__restrict__ tfq, const uint32_t *__restrict__ idf,
                                                              const uint32_t *__restrict__ offsets, const unsigned long long *__restrict__ list_sig,
                                                              const uint32_t *__restrict__ list_image, unsigned long long *__restrict__ dot,
                                                              IndexResultHead *__restrict__ head)
{
   const int lane = (int)(threadIdx.x & 63u);
   const int j = (int)(blockIdx.x * 4u + (threadIdx.x >> 6));
   if (j >= n) return;   // (the whole wave)
   const int w = words[(size_t)j * word_stride];
   // the word's query count goes to exactly one of the waves that hold the word, and the table is zero again for the next query
   uint32_t t = 0;
   if (lane == 0) t = atomicExch(&tfq[w], 0u);
   const unsigned long long f = idf[w];
   if (lane == 0 && t != 0u) hs_query_norm_add(&head->nq2, t, f);
   if (f == 0ull) return;   // a word of every image weighs nothing: its list, one of the longest, is not walked
   const unsigned long long sig = sigs[j];
   const uint32_t end = offsets[w + 1];
   hs_keylist_walk(lane, offsets[w], end, list_sig, list_image, sig, threshold, f * f, dot);   // idf^2 < 2^26
}
