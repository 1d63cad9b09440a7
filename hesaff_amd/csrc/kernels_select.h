// kernels_select.h -- hesaff_set_keypoint_limit: keep the N strongest Hessian keypoints of every image, on the device, between the
// ordering step of detection and k_affine.  No counterpart in the reference: a caller of it filters inside
// onHessianKeypointDetected (pyramid.h:43-47), after the whole list is known.
//
// Strength of keypoint i = |response_i|.  Responses passed the threshold, so they are finite and non-zero, and the uint32 bit
// patterns of fabsf(response) order exactly as the floats do.  With i the keypoint's position in the reference's detection order
// within its image, i is kept iff
//    #{j : |r_j| > |r_i|} + #{j < i : |r_j| == |r_i|} < N
// (ties at the cut go to the earlier keypoint).  The kept keypoints stay in the reference's order.
//
//   k_select_image     one block per image: MSB-first radix select over the image's segment of the ordered list (4 passes of 8 bits,
//                      256-bin LDS histogram) gives the threshold key T and the quota q = how many keys equal to T are kept; a fifth,
//                      ordered pass gives every keypoint its rank among the image's kept ones (or "dropped").
//   k_select_starts    one block: the per-image starts of the kept list (exclusive scan of min(N, count_b)) and its length.
//   k_hess_deal_kept   k_hess_deal's compacting twin: the kept 32-byte items to their new places in the Hessian list.
//
// The integer histogram is filled with LDS atomics, whose sums do not depend on arrival order; everything that depends on order
// (ties, ranks) comes from wave ballots and counts carried along the segment, so the result is the same for every launch geometry and
// from run to run.  The host does not know the list's length before its one round trip, so nothing here takes it as an argument.
#pragma once
#include "kernels_pyramid.h"

#define HS_SEL_THREADS 1024
#define HS_SEL_WAVES (HS_SEL_THREADS / 64)
#define HS_SEL_DROPPED 0xffffffffu

__device__ __forceinline__ uint32_t hs_strength_key(float response) { return __float_as_uint(response) & 0x7fffffffu; }   // bits of fabsf(response)

// keep_rank[i] for every keypoint i of image blockIdx.x: its rank among the image's kept keypoints, HS_SEL_DROPPED when it is not kept.
// starts: the nimg + 1 Hessian starts of k_image_counts; n_ptr: the list's length (clamped to cap, as every reader of the list does).
__global__ __launch_bounds__(HS_SEL_THREADS) void k_select_image(const float *__restrict__ response, const int32_t *__restrict__ starts,
                                                                 const uint32_t *__restrict__ n_ptr, uint32_t cap, uint32_t limit,
                                                                 uint32_t *__restrict__ keep_rank)
{
   __shared__ uint32_t s_hist[256];
   __shared__ uint32_t s_wsum[4];
   __shared__ uint32_t s_sel[2];                       // the pass's digit, and what is still wanted inside its bin
   __shared__ uint32_t s_cnt[2][2][HS_SEL_WAVES];      // [chunk parity][greater | equal][wave]
   const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
   const uint32_t n = min(*n_ptr, cap);
   const uint32_t lo = min((uint32_t)starts[blockIdx.x], n), hi = max(min((uint32_t)starts[blockIdx.x + 1], n), lo);
   if (hi - lo <= limit) {   // nothing to drop
      for (uint32_t i = lo + tid; i < hi; i += HS_SEL_THREADS) keep_rank[i] = i - lo;
      return;
   }
   // ---- threshold: the limit-th largest key.  Invariant: at least `want` keys match (key & mask) == prefix. ----
   uint32_t prefix = 0u, mask = 0u, want = limit;
   for (int shift = 24; shift >= 0; shift -= 8) {
      if (tid < 256u) s_hist[tid] = 0u;
      __syncthreads();
      for (uint32_t i = lo + tid; i < hi; i += HS_SEL_THREADS) {
         const uint32_t key = hs_strength_key(response[i]);
         if ((key & mask) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
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
         if (above < want && want <= above + h) { s_sel[0] = 255u - tid; s_sel[1] = want - above; }
      }
      __syncthreads();
      prefix |= s_sel[0] << shift;
      mask |= 255u << shift;
      want = s_sel[1];
   }
   const uint32_t T = prefix, q = want;   // keys above T are kept, and the first q keys equal to T (1 <= q)
   // ---- ordered pass: keypoint i has gt_before + min(eq_before, q) kept keypoints before it ----
   uint32_t c_gt = 0u, c_eq = 0u;   // counts of the chunks before this one
   int par = 0;
   for (uint32_t base = lo; base < hi; base += HS_SEL_THREADS, par ^= 1) {
      const uint32_t i = base + tid;
      const bool valid = i < hi;
      const uint32_t key = valid ? hs_strength_key(response[i]) : 0u;
      const bool gt = valid && key > T, eq = valid && key == T;
      const unsigned long long m_gt = __ballot(gt), m_eq = __ballot(eq);
      if (lane == 0u) { s_cnt[par][0][w] = (uint32_t)__popcll(m_gt); s_cnt[par][1][w] = (uint32_t)__popcll(m_eq); }
      __syncthreads();   // (one per chunk: the next chunk writes the other half of s_cnt)
      uint32_t gt_before = c_gt, eq_before = c_eq;
#pragma unroll
      for (uint32_t v = 0; v < HS_SEL_WAVES; v++) {
         const uint32_t a = s_cnt[par][0][v], e = s_cnt[par][1][v];
         if (v < w) { gt_before += a; eq_before += e; }
         c_gt += a; c_eq += e;
      }
      const unsigned long long below = (1ull << lane) - 1ull;
      gt_before += (uint32_t)__popcll(m_gt & below);
      eq_before += (uint32_t)__popcll(m_eq & below);
      if (valid) keep_rank[i] = (gt || (eq && eq_before < q)) ? gt_before + min(eq_before, q) : HS_SEL_DROPPED;
   }
}

// One block.  starts[b] (in place): where image b's kept keypoints begin; *hess_total: how many are kept in all; *detected: the length
// of the list detection made, for k_hess_deal_kept.  A list that overflowed the capacity is left as it is (*detected = 0: nothing is
// moved), so that the host meets the count it refuses.
__global__ __launch_bounds__(256) void k_select_starts(int32_t *__restrict__ starts, int nimg, uint32_t limit, uint32_t cap,
                                                       uint32_t *__restrict__ hess_total, uint32_t *__restrict__ detected)
{
   __shared__ uint32_t s_wave[4];
   const uint32_t total = *hess_total;
   if (threadIdx.x == 0) *detected = total <= cap ? total : 0u;
   if (total > cap) return;
   uint32_t carry = 0u;
   for (int base = 0; base < nimg; base += 256) {
      const int b = base + (int)threadIdx.x;
      uint32_t v = 0u;
      if (b < nimg) {
         const uint32_t lo = min((uint32_t)starts[b], total), hi = max(min((uint32_t)starts[b + 1], total), lo);
         v = min(hi - lo, limit);
      }
      uint32_t tot;
      const uint32_t ex = hs_block_exclusive_scan(v, s_wave, tot);   // (synchronises: every read of this chunk precedes its writes)
      if (b < nimg) starts[b] = (int32_t)(carry + ex);
      carry += tot;
   }
   __syncthreads();   // every thread has read *hess_total
   if (threadIdx.x == 0) { starts[nimg] = (int32_t)carry; *hess_total = carry; }
}

// k_hess_deal over the kept items only: item r of the ordered list goes to starts[its image] + keep_rank[r], which is never behind r
__global__ __launch_bounds__(256) void k_hess_deal_kept(const HessItem *__restrict__ items, const uint32_t *__restrict__ detected,
                                                        const uint32_t *__restrict__ keep_rank, const int32_t *__restrict__ starts, HessList hl)
{
   const uint32_t n = min(*detected, hl.cap);
   for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
      const uint32_t kr = keep_rank[r];
      if (kr == HS_SEL_DROPPED) continue;
      const float4 a = reinterpret_cast<const float4 *>(items + r)[0], b = reinterpret_cast<const float4 *>(items + r)[1];
      const int32_t meta = __float_as_int(b.x);
      const uint32_t dst = (uint32_t)starts[meta >> 8] + kr;
      if (dst > r) continue;   // (cannot happen: a compaction only moves items forward)
      hl.x[dst] = a.x; hl.y[dst] = a.y; hl.s[dst] = a.z; hl.response[dst] = a.w;
      hl.meta[dst] = meta; hl.r0c0[dst] = __float_as_int(b.y);
   }
}
