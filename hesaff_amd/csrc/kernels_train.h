// kernels_train.h -- the other half of a Lloyd iteration (hesaff_train_vocabulary, include/hesaff_amd.h): behind k_assign_words
// (kernels_words.h), the count and the byte sums of every word over the n keys, and the new vocabulary.  Integers only, and every
// sum is made of atomic integer additions or of a fixed order, so no result depends on the launch geometry or on which wave ran first.
//
// Accumulation.  The keys are grouped by word first - k_word_histogram counts, exclusive_scan (pipeline.hip) turns the counts into
// each word's first position, k_word_scatter writes the key indices there - so that a word's keys are neighbours in `perm`.  Both
// kernels add to a word's counter ONCE per wave and word: the lanes of a wave that hold the same word are found with ballots, one of
// them adds their number, and every lane takes its rank among them; with few words (K = 1: all keys) the counter sees n / 64
// additions, not n.  With some tens of words every wave still holds every word, and the counters are neighbours in one or two cache
// lines: so a word has `slots` sub-counters (accumulate_slots, train_plan.h: 64 for small K, 1 from K = 4097 on), wave v adds to slot
// v % slots, the scan runs over [K][slots], a word's entries are neighbours and so are its keys; k_word_counts reads count[k] off the
// cursor afterwards.  The order of the keys inside a word depends on which wave came first, but it is never output: sums do not care.
// k_accumulate_words: a half-wave walks 32 x chunks consecutive positions of `perm` (accumulate_chunks: 1 .. 8); its 32 lanes hold
// four byte columns each, as uint32 sums in registers, so one load of the wave reads two 128-byte rows.  The sums go to sum[word] with
// atomicAdd only where the word changes and at the end of the walk: (n / (32 chunks) + K) x 128 atomics at most.  (Adding every key's
// bytes straight to sum[word] is n x 128 atomics, all on one row when K is small.)
//
// k_update_words: per row the mean rounded half up (train_rounded_mean, train_plan.h), or the old row where the word has no key; the
// row is written three times - plain, as the caller reads it; XORed in the lane order k_assign_words reads (pack_vocabulary,
// capi_impl.h, is the same layout on the host); and its |w'|^2 - and rows that changed and words without keys are counted.  With all
// counts zero it is the packer of the initial vocabulary: every row is kept and laid out.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_words.h"
#include "train_plan.h"

using hesaff_plan::TrainStats;

// For the live lanes of a wave, each with a word w: counter[w] grows by the number of lanes that hold w - one atomicAdd per distinct
// word of the wave - and a lane receives the counter's value before that, plus its rank among those lanes.  Every lane of the wave
// must call (the loop is wave-uniform: `todo` is a ballot).
__device__ __forceinline__ uint32_t hs_claim_per_word(uint32_t *__restrict__ counter, int w, bool live)
{
   const int lane = (int)(threadIdx.x & 63u);
   uint32_t pos = 0;
   unsigned long long todo = __ballot(live);
   while (todo) {
      const int lead = __ffsll((long long)todo) - 1;
      const int w0 = __shfl(w, lead, 64);
      const bool mine = live && w == w0;
      const unsigned long long same = __ballot(mine);
      uint32_t base = 0;
      if (lane == lead) base = atomicAdd(&counter[w0], (uint32_t)__popcll(same));
      base = __shfl(base, lead, 64);
      if (mine) pos = base + (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
      todo &= ~same;
   }
   return pos;
}

// the sub-counter of word w that this wave adds to: slot = wave index % slots (slots: a power of two, accumulate_slots of train_plan.h)
__device__ __forceinline__ int hs_word_entry(int w, int slots) { return w * slots + (int)((blockIdx.x * 4u + (threadIdx.x >> 6)) & (uint32_t)(slots - 1)); }

// words: key i's word at words[i * word_stride] (2: the (word, dist2) rows of k_assign_words, whose dist2 are then summed into
// *distortion; 1: bare words, distortion == nullptr).  sub[K][slots] zeroed by the caller.  Grid: ceil(n / 256) blocks.
__global__ __launch_bounds__(256) void k_word_histogram(const int32_t *__restrict__ words, int word_stride, int n, uint32_t *__restrict__ sub, int slots,
                                                        unsigned long long *__restrict__ distortion)
{
   __shared__ uint32_t s_wave[4];
   const int i = (int)(blockIdx.x * 256u + threadIdx.x);
   const bool live = i < n;
   const int w = live ? hs_word_entry(words[(size_t)i * word_stride], slots) : -1;
   hs_claim_per_word(sub, w, live);
   if (!distortion) return;   // (uniform)
   // a block's dist2 fit uint32: 256 * 128 * 255^2 < 2^31
   uint32_t d = live ? (uint32_t)words[(size_t)i * word_stride + 1] : 0u;
#pragma unroll
   for (int m = 32; m >= 1; m >>= 1) d += __shfl_xor(d, m, 64);
   if ((threadIdx.x & 63u) == 0) s_wave[threadIdx.x >> 6] = d;
   __syncthreads();
   if (threadIdx.x == 0) atomicAdd(distortion, (unsigned long long)(s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3]));
}

// cursor[K][slots]: each entry's first position (the exclusive scan of sub, launched with the same grid) on entry, its end afterwards.
// perm[n]: the key indices by word (a word's entries are neighbours, so its keys are).
__global__ __launch_bounds__(256) void k_word_scatter(const int32_t *__restrict__ words, int word_stride, int n, uint32_t *__restrict__ cursor, int slots,
                                                      uint32_t *__restrict__ perm)
{
   const int i = (int)(blockIdx.x * 256u + threadIdx.x);
   const bool live = i < n;
   const int w = live ? hs_word_entry(words[(size_t)i * word_stride], slots) : -1;
   const uint32_t pos = hs_claim_per_word(cursor, w, live);
   if (live) perm[pos] = (uint32_t)i;
}

// counts[k] from the cursor behind k_word_scatter: the end of word k's last entry less the end of word k - 1's.  Grid: ceil(k / 256).
__global__ __launch_bounds__(256) void k_word_counts(const uint32_t *__restrict__ cursor, int slots, int k, uint32_t *__restrict__ counts)
{
   const int w = (int)(blockIdx.x * 256u + threadIdx.x);
   if (w >= k) return;
   counts[w] = cursor[(size_t)w * slots + slots - 1] - (w > 0 ? cursor[(size_t)w * slots - 1] : 0u);
}

#define HS_ACC_CHUNK 32   // positions of perm a half-wave fetches at a time; it walks `chunks` of them (accumulate_chunks, train_plan.h)

// desc: key i's bytes at desc + i * stride + offset (multiples of 4, as for k_assign_words).  sums[K][128] zeroed by the caller.
// Grid: ceil(n / (8 * HS_ACC_CHUNK * chunks)) blocks of 256.
__global__ __launch_bounds__(256) void k_accumulate_words(const uint8_t *__restrict__ desc, long long stride, long long offset,
                                                          const int32_t *__restrict__ words, int word_stride, const uint32_t *__restrict__ perm, int n,
                                                          int chunks, uint32_t *__restrict__ sums)
{
   const int lane = (int)(threadIdx.x & 63u), r = lane & 31, h = lane >> 5;
   // the half-wave's first position: the wave's 2 * 32 * chunks positions, half h the h-th half of them
   const long long first = (((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 2 + h) * HS_ACC_CHUNK * chunks;
   uint32_t acc[4] = {0, 0, 0, 0};
   int cur = -1;
   for (int c = 0; c < chunks; c++) {
      // lane r's position of this chunk: key index and word, handed round the half-wave one position at a time (-1: beyond the last key)
      const long long p = first + (long long)c * HS_ACC_CHUNK + r;
      uint32_t idx = 0;
      int w = -1;
      if (p < n) {
         idx = perm[p];
         w = words[(size_t)idx * word_stride];
      }
      for (int it = 0; it < HS_ACC_CHUNK; it++) {
         const uint32_t ki = __shfl(idx, HS_ACC_CHUNK * h + it, 64);
         const int kw = __shfl(w, HS_ACC_CHUNK * h + it, 64);
         if (kw != cur) {   // (the same for the 32 lanes of a half)
            if (cur >= 0) {
               uint32_t *s = sums + (size_t)cur * 128 + 4 * r;
#pragma unroll
               for (int q = 0; q < 4; q++) atomicAdd(s + q, acc[q]);
            }
            cur = kw;
            acc[0] = acc[1] = acc[2] = acc[3] = 0;
         }
         if (kw >= 0) {
            const uint32_t v = *(const uint32_t *)(desc + (long long)ki * stride + offset + 4 * r);
            acc[0] += v & 0xffu; acc[1] += (v >> 8) & 0xffu; acc[2] += (v >> 16) & 0xffu; acc[3] += v >> 24;
         }
      }
   }
   if (cur >= 0) {
      uint32_t *s = sums + (size_t)cur * 128 + 4 * r;
#pragma unroll
      for (int q = 0; q < 4; q++) atomicAdd(s + q, acc[q]);
   }
}

// Rows 0 .. k - 1: the update; rows k .. rows_padded - 1 (the pad rows of the last tile): zero bytes and HS_WORD_PAD_NORM.  A half-wave
// per row, four byte columns per lane.  rows [k][128], tiles / norms as k_assign_words reads them.  Grid: ceil(rows_padded / 8) blocks of 256.
__global__ __launch_bounds__(256) void k_update_words(const uint32_t *__restrict__ sums, const uint32_t *__restrict__ counts, int k, int rows_padded,
                                                      uint8_t *__restrict__ rows, uint8_t *__restrict__ tiles, int32_t *__restrict__ norms,
                                                      TrainStats *__restrict__ stats)
{
   const int lane = (int)(threadIdx.x & 63u), r = lane & 31, h = lane >> 5;
   const long long row = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 2 + h;
   const bool real = row < k, pad = !real && row < rows_padded;
   uint32_t old = 0x80808080u, nv = 0x80808080u, cnt = 0;   // (a pad row: XORed to zero below)
   if (real) {
      old = *(const uint32_t *)(rows + (size_t)row * 128 + 4 * r);
      cnt = counts[row];
      nv = old;
      if (cnt) {
         const uint4 s = *(const uint4 *)(sums + (size_t)row * 128 + 4 * r);
         nv = hesaff_plan::train_rounded_mean(s.x, cnt) | (hesaff_plan::train_rounded_mean(s.y, cnt) << 8) |
              (hesaff_plan::train_rounded_mean(s.z, cnt) << 16) | (hesaff_plan::train_rounded_mean(s.w, cnt) << 24);
      }
   }
   const uint32_t x = nv ^ 0x80808080u;
   int sq = hs_sq4_i8(x);
#pragma unroll
   for (int m = 16; m >= 1; m >>= 1) sq += __shfl_xor(sq, m, 64);   // (inside the half-wave)
   if (real || pad) {
      // bytes [4 r, 4 r + 4) of the row: step s = r / 8, half (r / 4) & 1 of the step, dword r & 3 of the lane's 16 bytes
      const size_t t = (size_t)row / HS_WORD_TILE, rr = (size_t)row % HS_WORD_TILE;
      *(uint32_t *)(tiles + ((t * 4 + (size_t)(r >> 3)) * 64 + rr + 32 * (size_t)((r >> 2) & 1)) * 16 + 4 * (r & 3)) = x;
      if (r == 0) norms[row] = real ? sq : HS_WORD_PAD_NORM;
   }
   if (real && nv != old) *(uint32_t *)(rows + (size_t)row * 128 + 4 * r) = nv;
   const unsigned long long ch = __ballot(real && nv != old), em = __ballot(real && cnt == 0 && r == 0);
   if (lane == 0) {
      const uint32_t changed = ((ch & 0xffffffffull) != 0 ? 1u : 0u) + ((ch >> 32) != 0 ? 1u : 0u);
      if (changed) atomicAdd(&stats->changed, changed);
      if (em) atomicAdd(&stats->empty, (uint32_t)__popcll(em));
   }
}

// rows[row] = key train_sample_index(row, n, k): the initial vocabulary of a call without one.  A thread per dword; grid: ceil(k * 32 / 256).
__global__ __launch_bounds__(256) void k_sample_words(const uint8_t *__restrict__ desc, long long stride, long long offset, int n, int k,
                                                      uint8_t *__restrict__ rows)
{
   const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
   const long long row = g >> 5;
   const int r = (int)(g & 31);
   if (row >= k) return;
   const long long key = hesaff_plan::train_sample_index(row, n, k);
   *(uint32_t *)(rows + (size_t)row * 128 + 4 * r) = *(const uint32_t *)(desc + key * stride + offset + 4 * r);
}
