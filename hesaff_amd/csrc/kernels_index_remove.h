// kernels_index_remove.h -- removing images from the image index (hesaff_index_remove of include/hesaff_amd.h), beside the build's and
// the add's kernels, which run here unchanged wherever their contract fits: k_index_idf, exclusive_scan, hs_index_norm_add, and the
// tile search of kernels_index_grow.h (hs_tile_words, hs_word_between).  What is here is what only a removal needs: the renumbering,
// the counting pass and the compaction of the word-major lists.
//
// The index keeps no image-major copy of its postings, so the postings of a removed image are found by a pass over all lists, and
// since every idf changes with N every norm is summed again: a removal is two passes over the old postings.  The first counts, per
// word, the postings whose image stays (df_new) and sums the tf of those whose image goes (the keys removed); idf over N - m and a
// scan of df_new give the new offsets; the second moves every survivor to new_off[w] + (a slot drawn from cursor[w]) under its new
// number remap[image] and adds (tf idf_new)^2 to that image's norm, with the build's arithmetic.  An embedded index makes the same two
// passes over its key lists.  remap is the exclusive scan of the keep-flags over the N old images, HS_REMOVE_GONE for one that goes.
//
// The grid is the merge's flat grid over the old positions (HS_GROW_TILE per block of 256), for the merge's reason: the list lengths
// are Zipf-distributed, most words hold fewer postings than a wave has lanes, and the few that hold millions would each be one wave's
// work under a wave per word.  Unlike the merge a removal cannot compute a survivor's place from its old one - the survivors below it
// are not known - so places are drawn from a per-word counter.  One atomic per posting on that counter would serialise exactly the
// long lists: millions of additions to one address.  The positions of a wavefront are consecutive, so the words of its 64 lanes
// form runs, and hs_word_run aggregates per run: a lane is a run's head where its word differs from the lane below; the ballots of
// the heads and of the survivors give every lane its run's mask, the population count of the survivors in it the run's count, and of
// those below the lane its rank; the head makes ONE atomicAdd for the run and the base is shuffled from it.  A list of L postings
// costs about L / 64 atomics on its word in either pass, a wave of 64 different words 64 atomics on 64 addresses - what a counter per
// word has to cost.  The removed keys are one 64-bit atomic per wavefront and tile, behind a wave reduction, on one of 64 counters
// a line apart (one counter serialised 426 000 of them where a tenth of the images went).  What was not chosen: a
// block-level scan of the survivors per word (the tile's words are few where lists are long, but then a word's count crosses blocks
// anyway and needs the atomic), and sorting.  The norm atomics stay: they are inherent to word-major lists (one address per image,
// spread over all images).  As everywhere in the index, sums are integers and the order inside a list - which slot a survivor draws -
// is no part of any result.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "index_remove_plan.h"
#include "kernels_index_grow.h"

// the scan's load (exclusive_scan) of the keep-flags: 1 where gone[i] is 0.  p: the gone-flags (and the pointer k_scan_down tests for
// alignment)
struct LoadKeepU32 {
   const uint32_t *p;
   __device__ uint32_t operator()(long long i) const { return p[i] == 0u ? 1u : 0u; }
   __device__ void load16(long long base, uint32_t *v) const
   {
      const uint4 *q = reinterpret_cast<const uint4 *>(p + base);
#pragma unroll
      for (int i = 0; i < 4; i++) { const uint4 w = q[i]; v[4 * i] = w.x == 0u; v[4 * i + 1] = w.y == 0u; v[4 * i + 2] = w.z == 0u; v[4 * i + 3] = w.w == 0u; }
   }
};

// remap[i]: the scan of the keep-flags on entry; a removed image gets HS_REMOVE_GONE, so that one load tells a pass both whether an
// image stays and what it becomes.  Grid: ceil(n / 256).
__global__ __launch_bounds__(256) void k_remove_mark(const uint32_t *__restrict__ gone, int n, uint32_t *__restrict__ remap)
{
   const int i = (int)(blockIdx.x * 256u + threadIdx.x);
   if (i < n && gone[i] != 0u) remap[i] = hesaff_plan::HS_REMOVE_GONE;
}

// A lane's place in the run of its word among the 64 consecutive positions of its wavefront.  Every lane of the wave calls, a lane
// without a position with a word no position has and survive false.
struct HsWordRun {
   bool head;        // the lowest lane of the run
   int first;        // that lane
   uint32_t count;   // survivors in the run
   uint32_t rank;    // survivors in the run below this lane
};
__device__ __forceinline__ HsWordRun hs_word_run(uint32_t word, bool survive)
{
   const int lane = (int)(threadIdx.x & 63u);
   const uint32_t below = (uint32_t)__shfl_up((int)word, 1, 64);
   HsWordRun r;
   r.head = lane == 0 || below != word;
   const unsigned long long heads = __ballot(r.head), alive = __ballot(survive);
   const unsigned long long upto = (2ull << lane) - 1ull;   // lanes 0 .. lane (lane 63: all)
   r.first = 63 - __clzll((long long)(heads & upto));       // (lane 0 is a head: never empty)
   const unsigned long long above = heads & ~upto;          // the heads of the runs behind this one
   const unsigned long long to_end = above ? ((above & (0ull - above)) - 1ull) : ~0ull;   // lanes below the next head
   const unsigned long long run = to_end & ~((1ull << r.first) - 1ull);
   r.count = (uint32_t)__popcll(alive & run);
   r.rank = (uint32_t)__popcll(alive & run & (upto >> 1));
   return r;
}

// The counting pass over the old postings, lists[n_old] word-major with off[k] == n_old: df_new[w] += the postings of w whose image
// stays, removed += the tf of those whose image goes, in the striped counters of index_remove_plan.h (both zeroed by the caller).
// Grid: ceil(n_old / HS_GROW_TILE) blocks of 256.
__global__ __launch_bounds__(256) void k_remove_count(const uint32_t *__restrict__ off, int k, uint32_t n_old, const IndexPosting *__restrict__ lists,
                                                      const uint32_t *__restrict__ remap, uint32_t *__restrict__ df_new, unsigned long long *__restrict__ removed)
{
   __shared__ uint32_t s_range[2];
   const uint32_t first = blockIdx.x * (uint32_t)HS_GROW_TILE;
   if (first >= n_old) return;   // (the whole block)
   const uint32_t end = min(first + (uint32_t)HS_GROW_TILE, n_old);
   hs_tile_words(off, k, first, end - 1u, s_range);
   uint32_t lost = 0u;   // <= 4 x 2^18
   for (uint32_t base = first; base < end; base += 256u) {   // (block-uniform: every lane of a wave takes part in the run's ballots)
      const uint32_t p = base + threadIdx.x;
      const bool valid = p < end;
      uint32_t w = 0xFFFFFFFFu;
      bool survive = false;
      if (valid) {
         w = hs_word_between(off, s_range[0], s_range[1], p);
         const IndexPosting e = lists[p];
         survive = remap[e.image] != hesaff_plan::HS_REMOVE_GONE;
         if (!survive) lost += e.tf;
      }
      const HsWordRun r = hs_word_run(w, survive);
      if (r.head && r.count) atomicAdd(&df_new[w], r.count);
   }
   // the wave's lost keys: < 2^26
#pragma unroll
   for (int d = 32; d >= 1; d >>= 1) lost += (uint32_t)__shfl_xor((int)lost, d, 64);
   if ((threadIdx.x & 63u) == 0u && lost)
      atomicAdd(&removed[(blockIdx.x % (uint32_t)hesaff_plan::HS_REMOVE_STRIPES) * (uint32_t)hesaff_plan::HS_REMOVE_STRIPE_WORDS], (unsigned long long)lost);
}

// The same count over the key-image array of an embedded index: count_new[w] += the keys of w whose image stays.  Grid as above.
__global__ __launch_bounds__(256) void k_remove_count_keys(const uint32_t *__restrict__ off, int k, uint32_t n_old, const uint32_t *__restrict__ key_image,
                                                           const uint32_t *__restrict__ remap, uint32_t *__restrict__ count_new)
{
   __shared__ uint32_t s_range[2];
   const uint32_t first = blockIdx.x * (uint32_t)HS_GROW_TILE;
   if (first >= n_old) return;
   const uint32_t end = min(first + (uint32_t)HS_GROW_TILE, n_old);
   hs_tile_words(off, k, first, end - 1u, s_range);
   for (uint32_t base = first; base < end; base += 256u) {
      const uint32_t p = base + threadIdx.x;
      const bool valid = p < end;
      uint32_t w = 0xFFFFFFFFu;
      bool survive = false;
      if (valid) {
         w = hs_word_between(off, s_range[0], s_range[1], p);
         survive = remap[key_image[p]] != hesaff_plan::HS_REMOVE_GONE;
      }
      const HsWordRun r = hs_word_run(w, survive);
      if (r.head && r.count) atomicAdd(&count_new[w], r.count);
   }
}

// the run's survivors draw consecutive slots from cursor[w]: one atomic by the head, the base shuffled from it -> this lane's slot
// (of use to a survivor alone).  Every lane of the wave calls.
__device__ __forceinline__ uint32_t hs_run_slot(const HsWordRun &r, uint32_t w, uint32_t *__restrict__ cursor)
{
   uint32_t base = 0u;
   if (r.head && r.count) base = atomicAdd(&cursor[w], r.count);
   return (uint32_t)__shfl((int)base, r.first, 64) + r.rank;
}

// The compaction: every old posting whose image stays to new_off[w] + (a slot drawn from cursor[w], zeroed by the caller) under its
// new number, and (tf idf)^2 to that image's norm (norm2 zeroed by the caller; idf: the new one).  Afterwards cursor[w] == df_new[w].
// Grid as k_remove_count.
__global__ __launch_bounds__(256) void k_remove_compact(const uint32_t *__restrict__ old_off, const uint32_t *__restrict__ new_off, int k, uint32_t n_old,
                                                        const IndexPosting *__restrict__ old_lists, IndexPosting *__restrict__ new_lists,
                                                        const uint32_t *__restrict__ remap, const uint32_t *__restrict__ idf,
                                                        unsigned long long *__restrict__ norm2, uint32_t *__restrict__ cursor)
{
   __shared__ uint32_t s_range[2];
   const uint32_t first = blockIdx.x * (uint32_t)HS_GROW_TILE;
   if (first >= n_old) return;
   const uint32_t end = min(first + (uint32_t)HS_GROW_TILE, n_old);
   hs_tile_words(old_off, k, first, end - 1u, s_range);
   for (uint32_t base = first; base < end; base += 256u) {
      const uint32_t p = base + threadIdx.x;
      const bool valid = p < end;
      uint32_t w = 0xFFFFFFFFu;
      IndexPosting e;
      e.image = hesaff_plan::HS_REMOVE_GONE; e.tf = 0u;
      if (valid) {
         w = hs_word_between(old_off, s_range[0], s_range[1], p);
         e = old_lists[p];
         e.image = remap[e.image];
      }
      const bool survive = e.image != hesaff_plan::HS_REMOVE_GONE;
      const HsWordRun r = hs_word_run(w, survive);
      const uint32_t slot = hs_run_slot(r, w, cursor);
      if (survive) {
         new_lists[new_off[w] + slot] = e;
         hs_index_norm_add(norm2, e.image, e.tf, idf[w]);
      }
   }
}

// The same compaction for the key lists of an embedded index (structure of arrays: signature and image).  Grid as k_remove_count_keys.
__global__ __launch_bounds__(256) void k_remove_compact_keys(const uint32_t *__restrict__ old_off, const uint32_t *__restrict__ new_off, int k, uint32_t n_old,
                                                             const unsigned long long *__restrict__ old_sig, const uint32_t *__restrict__ old_image,
                                                             unsigned long long *__restrict__ new_sig, uint32_t *__restrict__ new_image,
                                                             const uint32_t *__restrict__ remap, uint32_t *__restrict__ cursor)
{
   __shared__ uint32_t s_range[2];
   const uint32_t first = blockIdx.x * (uint32_t)HS_GROW_TILE;
   if (first >= n_old) return;
   const uint32_t end = min(first + (uint32_t)HS_GROW_TILE, n_old);
   hs_tile_words(old_off, k, first, end - 1u, s_range);
   for (uint32_t base = first; base < end; base += 256u) {
      const uint32_t p = base + threadIdx.x;
      const bool valid = p < end;
      uint32_t w = 0xFFFFFFFFu, image = hesaff_plan::HS_REMOVE_GONE;
      if (valid) {
         w = hs_word_between(old_off, s_range[0], s_range[1], p);
         image = remap[old_image[p]];
      }
      const bool survive = image != hesaff_plan::HS_REMOVE_GONE;
      const HsWordRun r = hs_word_run(w, survive);
      const uint32_t slot = hs_run_slot(r, w, cursor);
      if (survive) {
         const uint32_t to = new_off[w] + slot;
         new_sig[to] = old_sig[p];
         new_image[to] = image;
      }
   }
}
