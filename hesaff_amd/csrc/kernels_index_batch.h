// kernels_index_batch.h -- a chunk of index queries in one pass (hesaff_index_query_batch* of include/hesaff_amd.h): B consecutive
// queries of a batch, each with a row of dot and score over the N images and a head of its own (index_batch_plan.h).  The rules are
// the single query's (kernels_index.h, kernels_embed.h): integers up to the last step, every sum an atomic integer addition, so no
// result depends on the chunking, on the launch geometry or on which wave ran first.
//
// Counts.  B dense tfq tables would be B x K x 4 bytes; the chunk's words go through the build's scheme instead: k_index_insert
// (kernels_index.h) as it is, with the chunk's query starts in the place of the image starts, leaves one slot per distinct
// (query in chunk, word) with its count.
//
// Scoring.  One wavefront per query key of the chunk, as k_query_score.  The wave finds its query (the starts), lane 0 walks the
// key's probe sequence to its slot - the key is there: the insert put it - and exchanges the slot's count for 0, so exactly one wave
// per distinct (query, word) sees t > 0.  That wave adds (t idf)^2 to the query's nq2 and, unless idf is 0, its lanes stride the word's
// list and add t tf idf^2 to dot[query][image].  The embedded form mirrors k_query_score_embedded: EVERY wave walks its word's key list
// with its own signature, and the exchange serves nq2 alone.
//
// Finish and selection.  k_query_finish_batch runs over (query, image); k_index_select_batch is one block per query over the body of
// k_index_select.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "index_batch_plan.h"
#include "kernels_index.h"   // hs_index_image_of, hs_query_norm_add, hs_posting_walk, the score and the selection
#include "kernels_embed.h"   // hs_keylist_walk

// the slot of a key that the insert has put into the table, or `slots` where the probe meets an empty slot first (never, behind
// k_index_insert over the same words; the walk ends either way)
__device__ __forceinline__ unsigned long long hs_batch_find_slot(const unsigned long long *__restrict__ hash_keys, int bits, unsigned long long key)
{
   const unsigned long long mask = (1ull << bits) - 1ull;
   unsigned long long slot = hesaff_plan::index_hash_slot(key, bits);
   for (unsigned long long step = 0; step <= mask; step++) {
      const unsigned long long seen = hash_keys[slot];
      if (seen == key) return slot;
      if (seen == hesaff_plan::HS_INDEX_EMPTY) break;
      slot = (slot + 1ull) & mask;
   }
   return mask + 1ull;
}

// One wavefront per key of the chunk; dot and the heads zero on entry, the table filled by k_index_insert over the same words and
// starts.  starts [b + 1]: query q's keys are words[starts[q] .. starts[q + 1]).  dot [b][n_images].  Grid: ceil(total / 4) blocks of 256.
__global__ __launch_bounds__(256) void k_query_score_batch(const int32_t *__restrict__ words, int word_stride, const uint32_t *__restrict__ starts, int b,
                                                           uint32_t total, int bits, const unsigned long long *__restrict__ hash_keys,
                                                           uint32_t *__restrict__ hash_tf, const uint32_t *__restrict__ idf,
                                                           const uint32_t *__restrict__ offsets, const IndexPosting *__restrict__ lists, int n_images,
                                                           unsigned long long *__restrict__ dot, IndexResultHead *__restrict__ heads)
{
   const int lane = (int)(threadIdx.x & 63u);
   const uint32_t j = blockIdx.x * 4u + (threadIdx.x >> 6);
   if (j >= total) return;   // (the whole wave)
   const int w = words[(size_t)j * word_stride];
   const uint32_t q = hs_index_image_of(starts, b, j);
   // the (query, word)'s count goes to exactly one of the waves that hold the pair
   uint32_t t = 0;
   if (lane == 0) {
      const unsigned long long slot = hs_batch_find_slot(hash_keys, bits, hesaff_plan::index_key(q, (uint32_t)w));
      if (slot < (1ull << bits)) t = atomicExch(&hash_tf[slot], 0u);
   }
   t = (uint32_t)__shfl((int)t, 0, 64);
   if (t == 0u) return;
   const unsigned long long f = idf[w];
   if (lane == 0) hs_query_norm_add(&heads[q].nq2, t, f);
   if (f == 0ull) return;   // a word of every image weighs nothing: its list is not walked
   const uint32_t end = offsets[w + 1];
   hs_posting_walk(lane, offsets[w], end, lists, (unsigned long long)t * f * f, dot + (size_t)q * (size_t)n_images);   // t idf^2 < 2^44
}

// The same over the key lists of an embedded index: sigs[j] is key j's signature.  Grid: ceil(total / 4) blocks of 256.
__global__ __launch_bounds__(256) void k_query_score_embedded_batch(const int32_t *__restrict__ words, int word_stride, const unsigned long long *__restrict__ sigs,
                                                                    const uint32_t *__restrict__ starts, int b, uint32_t total, int threshold, int bits,
                                                                    const unsigned long long *__restrict__ hash_keys, uint32_t *__restrict__ hash_tf,
                                                                    const uint32_t *__restrict__ idf, const uint32_t *__restrict__ offsets,
                                                                    const unsigned long long *__restrict__ list_sig, const uint32_t *__restrict__ list_image,
                                                                    int n_images, unsigned long long *__restrict__ dot, IndexResultHead *__restrict__ heads)
{
   const int lane = (int)(threadIdx.x & 63u);
   const uint32_t j = blockIdx.x * 4u + (threadIdx.x >> 6);
   if (j >= total) return;   // (the whole wave)
   const int w = words[(size_t)j * word_stride];
   const uint32_t q = hs_index_image_of(starts, b, j);
   const unsigned long long f = idf[w];
   if (lane == 0) {
      uint32_t t = 0;
      const unsigned long long slot = hs_batch_find_slot(hash_keys, bits, hesaff_plan::index_key(q, (uint32_t)w));
      if (slot < (1ull << bits)) t = atomicExch(&hash_tf[slot], 0u);
      if (t != 0u) hs_query_norm_add(&heads[q].nq2, t, f);
   }
   if (f == 0ull) return;
   const unsigned long long sig = sigs[j];
   const uint32_t end = offsets[w + 1];
   hs_keylist_walk(lane, offsets[w], end, list_sig, list_image, sig, threshold, f * f, dot + (size_t)q * (size_t)n_images);   // idf^2 < 2^26
}

// score[q][i] over the b x n_images pairs of the chunk.  Grid-stride.
__global__ __launch_bounds__(256) void k_query_finish_batch(const unsigned long long *__restrict__ dot, const unsigned long long *__restrict__ norm2,
                                                            const IndexResultHead *__restrict__ heads, int n_images, unsigned long long pairs,
                                                            double *__restrict__ score)
{
   for (unsigned long long x = (unsigned long long)blockIdx.x * 256 + threadIdx.x; x < pairs; x += (unsigned long long)gridDim.x * 256) {
      const unsigned long long q = x / (unsigned long long)n_images, i = x - q * (unsigned long long)n_images;
      score[x] = hs_index_score(dot[x], heads[q].nq2, norm2[i]);
   }
}

// One block per query of the chunk.  ranked_scores / ranked_images [b][keep], keep = min(top, n_images).  Grid: b blocks.
__global__ __launch_bounds__(HS_ISEL_THREADS) void k_index_select_batch(const double *__restrict__ score, int n_images, int top, int keep,
                                                                        int32_t *__restrict__ ranked_images, double *__restrict__ ranked_scores,
                                                                        IndexResultHead *__restrict__ heads)
{
   const size_t q = blockIdx.x;
   hs_index_select_block(score + q * (size_t)n_images, n_images, top, ranked_images + q * (size_t)keep, ranked_scores + q * (size_t)keep, heads + q);
}
