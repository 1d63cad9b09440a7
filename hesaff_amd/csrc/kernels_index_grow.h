// kernels_index_grow.h -- growing and reloading the image index (hesaff_index_add*, hesaff_index_load of include/hesaff_amd.h), beside
// the build's kernels in kernels_index.h and kernels_embed.h, which run here unchanged wherever their contract fits: k_index_insert
// and k_index_df over a hash table sized for the NEW keys alone, k_index_idf, exclusive_scan, k_word_histogram, and the two scatters
// with the old images as their base.  What is here is what only a grown or a loaded index needs: the merges, the lengths, the load.
//
// Add.  df_new = df_old + (one per new distinct (image, word)); idf and the offsets follow from df_new and N + m.  Every list keeps
// its old entries in front: k_index_merge moves old posting r of word w from old_off[w] + r to new_off[w] + r.  The shift
// new_off[w] - old_off[w] is the sum of the NEW df of the words below w, so it never decreases with w: a flat grid over the old
// positions reads and writes runs that are contiguous but for a step at a word boundary - 8 bytes per lane, coalesced.  A block finds
// the words of its tile's first and last position with two binary searches of the old offsets (hs_index_image_of: a run of empty
// words repeats an offset and is never the answer, the word that owns the position is), and every thread then searches only between
// them - a tile of 1024 positions spans few words unless the lists are short, and then the range is what it has to be.  The flat grid
// was chosen over a wave per word because the list lengths are Zipf-distributed: most words hold fewer postings than a wave has
// lanes, and the few that hold millions would each be one wave's work.  The same pass adds (tf idf_new)^2 to norm2[image] - every idf
// changes with N, so every old norm is summed again, with the integer atomic of the build - and its first K threads leave
// cursor[w] = new_off[w] + df_old[w].  The build's k_index_postings (kernels_index.h) then scatters the new table's slots behind the
// cursors, its images numbered from the base N.  k_keylist_merge and the build's k_keylist_scatter (kernels_embed.h) do the same for
// the (image, signature) lists of an embedded index.  As everywhere in the index, sums are integers and the order inside a list is no
// part of any result.
//
// Load.  k_index_load_postings is the one pass over the postings of an index file: it finds each position's word as the merge does,
// checks the entry, and sums norm2 (hs_index_norm_add of kernels_index.h: the build's arithmetic), tf per image and tf per word.
// k_index_load_sums then checks the sums.  A violated rule sets its bit in *flags (index_plan.h: HS_LOAD_*); nothing is written outside the arrays of
// the index under construction: an image or a key image outside 0 .. N - 1 is flagged and not used as an address.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "index_plan.h"
#include "kernels_index.h"

#define HS_GROW_TILE 1024   // positions per block of 256: four per thread

// the word w with off[w] <= p < off[w + 1], searched between lo and hi where off[lo] <= p < off[hi]
__device__ __forceinline__ uint32_t hs_word_between(const uint32_t *__restrict__ off, uint32_t lo, uint32_t hi, uint32_t p)
{
   while (hi - lo > 1u) {
      const uint32_t mid = (lo + hi) >> 1;
      if (off[mid] <= p) lo = mid; else hi = mid;
   }
   return lo;
}

// The words of a block's tile [first, last] of positions (last < n = off[k]): s_range[0] owns `first`, s_range[1] - 1 owns `last`.
// Every thread of the block must call; ends with a barrier.
__device__ __forceinline__ void hs_tile_words(const uint32_t *__restrict__ off, int k, uint32_t first, uint32_t last, uint32_t *s_range)
{
   if (threadIdx.x < 2u) s_range[threadIdx.x] = hs_index_image_of(off, k, threadIdx.x == 0u ? first : last) + threadIdx.x;
   __syncthreads();
}

// Old postings to their new places, the old images' norms under the new idf, and each word's cursor behind its old postings.
// Grid: ceil(max(n_old, k) / HS_GROW_TILE) blocks of 256.  norm2 zeroed by the caller.  old_off[k] == n_old.
__global__ __launch_bounds__(256) void k_index_merge(const uint32_t *__restrict__ old_off, const uint32_t *__restrict__ new_off, int k, uint32_t n_old,
                                                     const IndexPosting *__restrict__ old_lists, IndexPosting *__restrict__ new_lists,
                                                     const uint32_t *__restrict__ idf, unsigned long long *__restrict__ norm2, uint32_t *__restrict__ cursor)
{
   __shared__ uint32_t s_range[2];
   const uint32_t first = blockIdx.x * (uint32_t)HS_GROW_TILE;
   for (uint32_t w = first + threadIdx.x; w < min(first + (uint32_t)HS_GROW_TILE, (uint32_t)k); w += 256u) cursor[w] = new_off[w] + (old_off[w + 1] - old_off[w]);
   if (first >= n_old) return;   // (the whole block)
   hs_tile_words(old_off, k, first, min(first + (uint32_t)HS_GROW_TILE, n_old) - 1u, s_range);
   for (uint32_t p = first + threadIdx.x; p < min(first + (uint32_t)HS_GROW_TILE, n_old); p += 256u) {
      const uint32_t w = hs_word_between(old_off, s_range[0], s_range[1], p);
      const IndexPosting e = old_lists[p];
      new_lists[new_off[w] + (p - old_off[w])] = e;
      hs_index_norm_add(norm2, e.image, e.tf, idf[w]);
   }
}

// The same move for the key lists of an embedded index (structure of arrays: signature and image).  Grid and cursor as k_index_merge.
__global__ __launch_bounds__(256) void k_keylist_merge(const uint32_t *__restrict__ old_off, const uint32_t *__restrict__ new_off, int k, uint32_t n_old,
                                                       const unsigned long long *__restrict__ old_sig, const uint32_t *__restrict__ old_image,
                                                       unsigned long long *__restrict__ new_sig, uint32_t *__restrict__ new_image, uint32_t *__restrict__ cursor)
{
   __shared__ uint32_t s_range[2];
   const uint32_t first = blockIdx.x * (uint32_t)HS_GROW_TILE;
   for (uint32_t w = first + threadIdx.x; w < min(first + (uint32_t)HS_GROW_TILE, (uint32_t)k); w += 256u) cursor[w] = new_off[w] + (old_off[w + 1] - old_off[w]);
   if (first >= n_old) return;
   hs_tile_words(old_off, k, first, min(first + (uint32_t)HS_GROW_TILE, n_old) - 1u, s_range);
   for (uint32_t p = first + threadIdx.x; p < min(first + (uint32_t)HS_GROW_TILE, n_old); p += 256u) {
      const uint32_t w = hs_word_between(old_off, s_range[0], s_range[1], p);
      const uint32_t to = new_off[w] + (p - old_off[w]);
      new_sig[to] = old_sig[p];
      new_image[to] = old_image[p];
   }
}

// len[w] = off[w + 1] - off[w].  Grid: ceil(k / 256).
__global__ __launch_bounds__(256) void k_list_lengths(const uint32_t *__restrict__ off, int k, uint32_t *__restrict__ len)
{
   const int w = (int)(blockIdx.x * 256u + threadIdx.x);
   if (w < k) len[w] = off[w + 1] - off[w];
}

// The pass over the postings of an index file, lists[n] word-major with off[k] == n.  image_tf[n_images], word_tf[k] (embedded files
// only, else NULL) and norm2 zeroed by the caller.  Grid: ceil(n / HS_GROW_TILE) blocks of 256.
__global__ __launch_bounds__(256) void k_index_load_postings(const uint32_t *__restrict__ off, int k, uint32_t n, const IndexPosting *__restrict__ lists,
                                                             int n_images, const uint32_t *__restrict__ idf, unsigned long long *__restrict__ norm2,
                                                             unsigned long long *__restrict__ image_tf, unsigned long long *__restrict__ word_tf,
                                                             uint32_t *__restrict__ flags)
{
   __shared__ uint32_t s_range[2];
   const uint32_t first = blockIdx.x * (uint32_t)HS_GROW_TILE;
   if (first >= n) return;
   hs_tile_words(off, k, first, min(first + (uint32_t)HS_GROW_TILE, n) - 1u, s_range);
   uint32_t bad = 0u;
   for (uint32_t p = first + threadIdx.x; p < min(first + (uint32_t)HS_GROW_TILE, n); p += 256u) {
      const uint32_t w = hs_word_between(off, s_range[0], s_range[1], p);
      const IndexPosting e = lists[p];
      const bool image_ok = e.image < (uint32_t)n_images;
      const bool tf_ok = e.tf >= 1u && e.tf <= (uint32_t)hesaff_plan::HS_INDEX_MAX_IMAGE_KEYS;
      if (!image_ok) bad |= hesaff_plan::HS_LOAD_IMAGE;
      if (!tf_ok) bad |= hesaff_plan::HS_LOAD_TF;
      if (!image_ok || !tf_ok) continue;
      hs_index_norm_add(norm2, e.image, e.tf, idf[w]);
      atomicAdd(&image_tf[e.image], (unsigned long long)e.tf);   // <= 2^28 postings of <= 2^18: < 2^46
      if (word_tf) atomicAdd(&word_tf[w], (unsigned long long)e.tf);
   }
   if (bad) atomicOr(flags, bad);
}

// The sums of the load: every image's tf <= 2^18, their total == n_keys (added into *total, zeroed by the caller, and compared on
// the host), and for an embedded file every word's key count == its tf.  Grid: ceil(max(n_images, k) / 256).
__global__ __launch_bounds__(256) void k_index_load_sums(const unsigned long long *__restrict__ image_tf, int n_images, const unsigned long long *__restrict__ word_tf,
                                                         const uint32_t *__restrict__ key_count, int k, unsigned long long *__restrict__ total,
                                                         uint32_t *__restrict__ flags)
{
   const uint32_t t = blockIdx.x * 256u + threadIdx.x;
   uint32_t bad = 0u;
   if (t < (uint32_t)n_images) {
      const unsigned long long s = image_tf[t];
      if (s > (unsigned long long)hesaff_plan::HS_INDEX_MAX_IMAGE_KEYS) bad |= hesaff_plan::HS_LOAD_IMAGE_SUM;
      if (s) atomicAdd(total, s);
   }
   if (word_tf && t < (uint32_t)k && word_tf[t] != (unsigned long long)key_count[t]) bad |= hesaff_plan::HS_LOAD_KEY_COUNT;
   if (bad) atomicOr(flags, bad);
}

// every key image of an embedded file lies below n_images.  Reads only.  Grid-stride.
__global__ __launch_bounds__(256) void k_index_load_key_images(const uint32_t *__restrict__ key_image, unsigned long long n, int n_images, uint32_t *__restrict__ flags)
{
   bool wrong = false;
   for (unsigned long long j = (unsigned long long)blockIdx.x * 256 + threadIdx.x; j < n; j += (unsigned long long)gridDim.x * 256) wrong |= key_image[j] >= (uint32_t)n_images;
   if (__ballot(wrong) != 0ull && (threadIdx.x & 63u) == 0u) atomicOr(flags, (uint32_t)hesaff_plan::HS_LOAD_KEY_IMAGE);
}
