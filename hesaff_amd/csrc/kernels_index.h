// kernels_index.h -- the image index (hesaff_index_build, hesaff_index_query of include/hesaff_amd.h): an inverted file over visual
// words with tf-idf scoring.  Integers up to the last step, and every sum is made of atomic integer additions, so no result depends
// on the launch geometry or on which wave ran first; the score is three IEEE binary64 operations on those integers.
//
// Build.  k_index_insert puts every key's (image, word) into an open-addressing hash table of 64-bit keys (index_plan.h: at least
// twice as many slots as keys, all-ones = empty): atomicCAS on the key, linear probing, atomicAdd on the slot's count.  The set of
// (image, word, tf) that results does not depend on the order of arrival; the slot layout does and is never output.  k_index_df adds
// one to df[word] per occupied slot, k_index_idf turns df into idf (ilog2_q8), exclusive_scan (pipeline.hip) turns df into the list
// offsets, and k_index_postings - the second pass over the table - writes every slot's (image, tf) to the next free place of its
// word's list and adds (tf idf)^2 to norm2[image]; an add (kernels_index_grow.h) runs the same kernel behind the old postings.  The order of the postings inside a list depends on which wave came first; only
// sums over a list are ever output.
//
// Query.  k_query_count adds the query's keys into tfq[word].  k_query_score runs one wavefront per query KEY: lane 0 exchanges
// tfq[word] for 0 - exactly one wave per distinct word sees t > 0, and the same exchange leaves the table zero for the next query -
// that wave adds (t idf)^2 to nq2 and, unless idf is 0 (a word of every image: exactly the longest lists), its lanes stride the
// word's list and add t tf idf^2 to dot[image].  k_query_finish writes score[i]; k_index_select finds the `top` winners.
//
// Selection.  The bit pattern of a non-negative double orders as the value does, so the order (score descending, image ascending)
// is the descending order of the 96-bit key (score bits, ~image), in which no two images are equal.  One block: MSB-first radix
// select with 8-bit digits (at most 12 passes over the scores, in the manner of kernels_select.h) until the chosen bin holds exactly
// what is still wanted; the survivors - exactly `top` of them - go to LDS in any order and are ranked by counting (1024 x 1024
// comparisons at most), which needs no stable sort because the keys are distinct.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "index_plan.h"

using hesaff_plan::IndexPosting;
using hesaff_plan::IndexResultHead;

// key j's word is words[j * word_stride]; *bad becomes 1 where one lies outside 0 .. k - 1.  Reads only.  Grid-stride.
__global__ __launch_bounds__(256) void k_index_check_words(const int32_t *__restrict__ words, int word_stride, long long n, int k, uint32_t *__restrict__ bad)
{
   bool wrong = false;
   for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < n; j += (long long)gridDim.x * 256) {
      const int32_t w = words[j * word_stride];
      wrong |= w < 0 || w >= k;
   }
   if (__ballot(wrong) != 0ull && (threadIdx.x & 63u) == 0u) atomicOr(bad, 1u);
}

// the image of key j: the i with starts[i] <= j < starts[i + 1] (images without keys repeat a start and are never found)
__device__ __forceinline__ uint32_t hs_index_image_of(const uint32_t *__restrict__ starts, int n_images, uint32_t j)
{
   uint32_t lo = 0, hi = (uint32_t)n_images;   // starts[lo] <= j < starts[hi]
   while (hi - lo > 1u) {
      const uint32_t mid = (lo + hi) >> 1;
      if (starts[mid] <= j) lo = mid; else hi = mid;
   }
   return lo;
}

// Every key into the table (hash_keys all-ones, hash_tf zero on entry).  The table has an empty slot on every probe path: slots >= 2 T.
// Grid: ceil(total / 256) blocks.
__global__ __launch_bounds__(256) void k_index_insert(const int32_t *__restrict__ words, int word_stride, const uint32_t *__restrict__ starts, int n_images,
                                                      uint32_t total, int bits, unsigned long long *__restrict__ hash_keys, uint32_t *__restrict__ hash_tf)
{
   const uint32_t j = blockIdx.x * 256u + threadIdx.x;
   if (j >= total) return;
   const uint32_t image = hs_index_image_of(starts, n_images, j);
   const unsigned long long key = hesaff_plan::index_key(image, (uint32_t)words[(size_t)j * word_stride]);
   const unsigned long long mask = (1ull << bits) - 1ull;
   unsigned long long slot = hesaff_plan::index_hash_slot(key, bits);
   for (;;) {
      const unsigned long long seen = atomicCAS(&hash_keys[slot], (unsigned long long)hesaff_plan::HS_INDEX_EMPTY, key);
      if (seen == hesaff_plan::HS_INDEX_EMPTY || seen == key) break;
      slot = (slot + 1ull) & mask;
   }
   atomicAdd(&hash_tf[slot], 1u);
}

// df[word] += 1 per occupied slot (df zeroed by the caller).  Grid-stride over the slots.
__global__ __launch_bounds__(256) void k_index_df(const unsigned long long *__restrict__ hash_keys, unsigned long long slots, uint32_t *__restrict__ df)
{
   for (unsigned long long s = (unsigned long long)blockIdx.x * 256 + threadIdx.x; s < slots; s += (unsigned long long)gridDim.x * 256) {
      const unsigned long long key = hash_keys[s];
      if (key != hesaff_plan::HS_INDEX_EMPTY) atomicAdd(&df[hesaff_plan::index_key_word(key)], 1u);
   }
}

// Grid: ceil(k / 256).
__global__ __launch_bounds__(256) void k_index_idf(const uint32_t *__restrict__ df, int k, int n_images, uint32_t *__restrict__ idf)
{
   const int w = (int)(blockIdx.x * 256u + threadIdx.x);
   if (w < k) idf[w] = hesaff_plan::index_idf((uint64_t)n_images, df[w]);
}

// (tf idf)^2 into norm2[image]: the one spelling of a posting's weight in its image's norm (the scatter below, and the merge and the
// load of kernels_index_grow.h)
__device__ __forceinline__ void hs_index_norm_add(unsigned long long *__restrict__ norm2, uint32_t image, uint32_t tf, uint32_t idf)
{
   const unsigned long long wt = (unsigned long long)tf * idf;   // < 2^31
   if (wt) atomicAdd(&norm2[image], wt * wt);
}

// Every slot's (image, tf) to the next free place of its word's list, the table's images numbered from `base` (a build: 0, an add:
// the images of the index so far).  cursor[k]: each list's next free position on entry - a copy of the offsets, or behind the old
// postings (k_index_merge) - its end afterwards.  norm2 is added to.  Grid-stride over the slots.
__global__ __launch_bounds__(256) void k_index_postings(const unsigned long long *__restrict__ hash_keys, const uint32_t *__restrict__ hash_tf,
                                                        unsigned long long slots, uint32_t base, const uint32_t *__restrict__ idf,
                                                        uint32_t *__restrict__ cursor, IndexPosting *__restrict__ lists, unsigned long long *__restrict__ norm2)
{
   for (unsigned long long s = (unsigned long long)blockIdx.x * 256 + threadIdx.x; s < slots; s += (unsigned long long)gridDim.x * 256) {
      const unsigned long long key = hash_keys[s];
      if (key == hesaff_plan::HS_INDEX_EMPTY) continue;
      const uint32_t word = hesaff_plan::index_key_word(key), image = base + hesaff_plan::index_key_image(key), tf = hash_tf[s];
      const uint32_t pos = atomicAdd(&cursor[word], 1u);
      IndexPosting p;
      p.image = image; p.tf = tf;
      lists[pos] = p;
      hs_index_norm_add(norm2, image, tf, idf[word]);
   }
}

// tfq[word] += 1 per query key.  Grid: ceil(n / 256).
__global__ __launch_bounds__(256) void k_query_count(const int32_t *__restrict__ words, int word_stride, int n, uint32_t *__restrict__ tfq)
{
   const int j = (int)(blockIdx.x * 256u + threadIdx.x);
   if (j < n) atomicAdd(&tfq[words[(size_t)j * word_stride]], 1u);
}

// (t idf)^2 into a query's squared norm, by one lane of the one wave that holds the word's count t (k_query_score* here, in
// kernels_embed.h and in kernels_index_batch.h)
__device__ __forceinline__ void hs_query_norm_add(unsigned long long *__restrict__ nq2, uint32_t t, unsigned long long f)
{
   atomicAdd(nq2, ((unsigned long long)t * f) * ((unsigned long long)t * f));   // (t idf)^2 < 2^62
}

// A wave's walk of one word's postings lists[first .. end), its lanes striding them: tff tf = t tf idf^2 into row[image] (the dot
// of the query, or the query's row of a chunk's)
__device__ __forceinline__ void hs_posting_walk(int lane, uint32_t first, uint32_t end, const IndexPosting *__restrict__ lists, unsigned long long tff,
                                                unsigned long long *__restrict__ row)
{
   for (uint32_t p = first + (uint32_t)lane; p < end; p += 64u) {
      const IndexPosting e = lists[p];
      atomicAdd(&row[e.image], tff * e.tf);   // < 2^62
   }
}

// One wavefront per query key; dot zeroed, head->nq2 zero on entry.  Grid: ceil(n / 4) blocks of 256.
__global__ __launch_bounds__(256) void k_query_score(const int32_t *__restrict__ words, int word_stride, int n, uint32_t *__restrict__ tfq,
                                                     const uint32_t *__restrict__ idf, const uint32_t *__restrict__ offsets,
                                                     const IndexPosting *__restrict__ lists, unsigned long long *__restrict__ dot,
                                                     IndexResultHead *__restrict__ head)
{
   const int lane = (int)(threadIdx.x & 63u);
   const int j = (int)(blockIdx.x * 4u + (threadIdx.x >> 6));
   if (j >= n) return;   // (the whole wave)
   const int w = words[(size_t)j * word_stride];
   // the word's query count goes to exactly one of the waves that hold the word, and the table is zero again for the next query
   uint32_t t = 0;
   if (lane == 0) t = atomicExch(&tfq[w], 0u);
   t = (uint32_t)__shfl((int)t, 0, 64);
   if (t == 0u) return;
   const unsigned long long f = idf[w];
   if (lane == 0) hs_query_norm_add(&head->nq2, t, f);
   if (f == 0ull) return;   // a word of every image weighs nothing: its list, one of the longest, is not walked
   const uint32_t end = offsets[w + 1];
   hs_posting_walk(lane, offsets[w], end, lists, (unsigned long long)t * f * f, dot);   // t idf^2 < 2^44
}

// the score of one image: the three binary64 operations of the definition (k_query_finish, and k_query_finish_batch of
// kernels_index_batch.h)
__device__ __forceinline__ double hs_index_score(unsigned long long d, unsigned long long nq2, unsigned long long n2)
{
   return d ? __ddiv_rn(__ull2double_rn(d), __dsqrt_rn(__dmul_rn(__ull2double_rn(nq2), __ull2double_rn(n2)))) : 0.0;
}

// score[i] = dot / sqrt(nq2 * norm2) in binary64 - the conversions, the product, the root and the quotient each rounded to nearest
// even - or 0.0 where dot is 0.  Grid: ceil(n_images / 256).
__global__ __launch_bounds__(256) void k_query_finish(const unsigned long long *__restrict__ dot, const unsigned long long *__restrict__ norm2,
                                                      const IndexResultHead *__restrict__ head, int n_images, double *__restrict__ score)
{
   const int i = (int)(blockIdx.x * 256u + threadIdx.x);
   if (i >= n_images) return;
   score[i] = hs_index_score(dot[i], head->nq2, norm2[i]);
}

#define HS_ISEL_THREADS 1024

// digit `pass` (0: the most significant) of the 96-bit key (hi = score bits, lo = ~image)
__device__ __forceinline__ uint32_t hs_isel_digit(unsigned long long hi, uint32_t lo, int pass)
{
   return pass < 8 ? (uint32_t)(hi >> (56 - 8 * pass)) & 255u : (lo >> (24 - 8 * (pass - 8))) & 255u;
}

// The selection of one block of HS_ISEL_THREADS threads over one row of scores (k_index_select, and one block per query in
// k_index_select_batch of kernels_index_batch.h).  top_images / top_scores [min(top, n_images)]: the images in the order (score
// descending, image ascending); head->count.
__device__ __forceinline__ void hs_index_select_block(const double *__restrict__ score, int n_images, int top, int32_t *__restrict__ top_images,
                                                      double *__restrict__ top_scores, IndexResultHead *__restrict__ head)
{
   __shared__ uint32_t s_hist[256];
   __shared__ uint32_t s_wsum[4];
   __shared__ uint32_t s_sel[3];   // the pass's digit, what is still wanted inside its bin, and the bin's size
   __shared__ unsigned long long s_hi[hesaff_plan::HS_INDEX_MAX_TOP];
   __shared__ uint32_t s_lo[hesaff_plan::HS_INDEX_MAX_TOP];
   __shared__ uint32_t s_n;
   const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
   const uint32_t n = (uint32_t)n_images;
   const uint32_t keep = min((uint32_t)top, n);
   // ---- the threshold: the keep-th largest key.  Invariant: exactly `want` of the keys that match the prefix are kept, with every
   // key above the prefix.  Ends when the chosen bin holds exactly what is wanted: then everything from the prefix up is kept. ----
   unsigned long long p_hi = 0ull, m_hi = 0ull;
   uint32_t p_lo = 0u, m_lo = 0u, want = keep;
   if (keep < n) {
      for (int pass = 0; pass < 12; pass++) {
         if (tid < 256u) s_hist[tid] = 0u;
         __syncthreads();
         for (uint32_t i = tid; i < n; i += HS_ISEL_THREADS) {
            const unsigned long long hi = (unsigned long long)__double_as_longlong(score[i]);
            const uint32_t lo = ~i;
            if ((hi & m_hi) == p_hi && (lo & m_lo) == p_lo) atomicAdd(&s_hist[hs_isel_digit(hi, lo, pass)], 1u);
         }
         __syncthreads();
         // bins from the top: thread t owns bin 255 - t; `above` = matching keys in higher bins (a scan over the first four waves)
         uint32_t h = 0u, inc = 0u;
         if (tid < 256u) {
            h = s_hist[255u - tid];
            inc = h;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
               const uint32_t t = __shfl_up(inc, d, 64);
               if (lane >= (uint32_t)d) inc += t;
            }
            if (lane == 63u) s_wsum[w] = inc;
         }
         __syncthreads();
         if (tid < 256u) {
            uint32_t above = inc - h;
            for (uint32_t v = 0; v < w; v++) above += s_wsum[v];
            // exactly one bin holds the want-th largest: the intervals (above, above + h] are disjoint
            if (above < want && want <= above + h) { s_sel[0] = 255u - tid; s_sel[1] = want - above; s_sel[2] = h; }
         }
         __syncthreads();
         const uint32_t digit = s_sel[0];
         if (pass < 8) { p_hi |= (unsigned long long)digit << (56 - 8 * pass); m_hi |= 255ull << (56 - 8 * pass); }
         else { p_lo |= digit << (24 - 8 * (pass - 8)); m_lo |= 255u << (24 - 8 * (pass - 8)); }
         want = s_sel[1];
         if (want == s_sel[2]) break;   // (block-uniform) the bin is kept whole; with distinct keys at the latest when it holds one key
      }
   }
   // ---- the survivors: every key whose masked bits are at least the prefix - exactly `keep` of them - in any order ----
   if (tid == 0u) s_n = 0u;
   __syncthreads();
   for (uint32_t i = tid; i < n; i += HS_ISEL_THREADS) {
      const unsigned long long hi = (unsigned long long)__double_as_longlong(score[i]);
      const uint32_t lo = ~i;
      const unsigned long long a = hi & m_hi;
      if (a > p_hi || (a == p_hi && (lo & m_lo) >= p_lo)) {
         const uint32_t at = atomicAdd(&s_n, 1u);
         if (at < (uint32_t)hesaff_plan::HS_INDEX_MAX_TOP) { s_hi[at] = hi; s_lo[at] = lo; }
      }
   }
   __syncthreads();
   const uint32_t got = min(s_n, (uint32_t)hesaff_plan::HS_INDEX_MAX_TOP);   // (== keep)
   // ---- rank by counting: the keys are distinct, so the ranks are 0 .. got - 1 ----
   if (tid < got) {
      const unsigned long long hi = s_hi[tid];
      const uint32_t lo = s_lo[tid];
      uint32_t rank = 0u;
      for (uint32_t v = 0; v < got; v++) {
         const unsigned long long h2 = s_hi[v];
         rank += (h2 > hi || (h2 == hi && s_lo[v] > lo)) ? 1u : 0u;
      }
      top_images[rank] = (int32_t)~lo;
      top_scores[rank] = __longlong_as_double((long long)hi);
   }
   if (tid == 0u) head->count = got;
}

// One block.
__global__ __launch_bounds__(HS_ISEL_THREADS) void k_index_select(const double *__restrict__ score, int n_images, int top, int32_t *__restrict__ top_images,
                                                                  double *__restrict__ top_scores, IndexResultHead *__restrict__ head)
{
   hs_index_select_block(score, n_images, top, top_images, top_scores, head);
}
