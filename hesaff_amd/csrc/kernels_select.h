// kernels_select.h -- which Hessian keypoints of every image go on to k_affine, chosen on the device between the ordering step of
// detection and k_affine: hesaff_set_keypoint_limit (the N strongest) and hesaff_set_next_masks (those on a non-zero mask pixel).
// No counterpart in the reference: a caller of it filters inside onHessianKeypointDetected (pyramid.h:43-47), after the whole list
// is known.
//
// Eligible: an image without a mask has every keypoint eligible; with a mask (height x width bytes at the caller's image size),
// keypoint i is eligible iff mask[row][col] != 0, col = clamp((int)(x + 0.5f), 0, width - 1), row = clamp((int)(y + 0.5f), 0,
// height - 1) - the add in binary32, the conversion truncating - with x, y the floats onHessianKeypointDetected receives.
//
// Strength of keypoint i = |response_i|.  Responses passed the threshold, so they are finite and non-zero, and the uint32 bit
// patterns of fabsf(response) order exactly as the floats do.  With i the keypoint's position in the reference's detection order
// within its image and j ranging over the image's eligible keypoints, an eligible i is kept iff
//    #{j : |r_j| > |r_i|} + #{j < i : |r_j| == |r_i|} < N
// (ties at the cut go to the earlier keypoint; no limit: every eligible keypoint).  The kept keypoints stay in the reference's order.
//
//   k_select_image     one block per image: MSB-first radix select over the eligible keypoints of the image's segment of the ordered
//                      list (4 passes of 8 bits, 256-bin LDS histogram) gives the threshold key T and the quota q = how many keys
//                      equal to T are kept; a fifth, ordered pass gives every keypoint its rank among the image's kept ones (or
//                      "dropped") and the image its kept count.  A mask without a limit is the ordered pass alone.
//   k_select_starts    one block: the per-image starts of the kept list (exclusive scan of the kept counts) and its length.
//   k_hess_deal_kept   k_hess_deal's compacting twin: the kept 32-byte items to their new places in the Hessian list.
//
// The integer histogram is filled with LDS atomics, whose sums do not depend on arrival order; everything that depends on order
// (ties, ranks) comes from wave ballots and counts carried along the segment, so the result is the same for every launch geometry and
// from run to run.  The host does not know the list's length before its one round trip, so nothing here takes it as an argument.
// The mask costs one scattered byte per keypoint and pass: a few thousand bytes per image, which no staging would repay.
#pragma once
#include "kernels_pyramid.h"

#define HS_SEL_THREADS 1024
#define HS_SEL_WAVES (HS_SEL_THREADS / 64)
#define HS_SEL_DROPPED 0xffffffffu

__device__ __forceinline__ uint32_t hs_strength_key(float response) { return __float_as_uint(response) & 0x7fffffffu; }   // bits of fabsf(response)

// The detection masks of a batch (hesaff_set_next_masks*): plane b starts img_stride bytes after plane b-1, its rows are row_stride
// bytes apart, W x H is the images' size as the caller passed them.  present: one byte per image, 0 = image b has no mask (null: every
// image has one).  base null: the batch has no masks.
struct SelMasks {
   const uint8_t *base = nullptr;
   const uint8_t *present = nullptr;
   long long img_stride = 0;
   int row_stride = 0, W = 0, H = 0;
};
#define HS_SEL_NO_LIMIT 0xffffffffu

// (the clamps keep every read inside the plane whatever x and y hold)
__device__ __forceinline__ bool hs_mask_eligible(const uint8_t *__restrict__ plane, int row_stride, int W, int H, float x, float y)
{
   const int col = min(max((int)(x + 0.5f), 0), W - 1), row = min(max((int)(y + 0.5f), 0), H - 1);
   return plane[(long long)row * row_stride + col] != 0;
}

// keep_rank[i] for every keypoint i of image blockIdx.x: its rank among the image's kept keypoints, HS_SEL_DROPPED when it is not kept;
// kept[blockIdx.x]: how many are.  starts: the nimg + 1 Hessian starts of k_image_counts; n_ptr: the list's length (clamped to cap, as
// every reader of the list does); limit: HS_SEL_NO_LIMIT when only the masks select.
__global__ __launch_bounds__(HS_SEL_THREADS) void k_select_image(const float *__restrict__ response, const float *__restrict__ kx,
                                                                 const float *__restrict__ ky, const int32_t *__restrict__ starts,
                                                                 const uint32_t *__restrict__ n_ptr, uint32_t cap, uint32_t limit, SelMasks mk,
                                                                 uint32_t *__restrict__ keep_rank, uint32_t *__restrict__ kept)
{
   __shared__ uint32_t s_hist[256];
   __shared__ uint32_t s_wsum[4];
   __shared__ uint32_t s_sel[2];                       // the pass's digit, and what is still wanted inside its bin
   __shared__ uint32_t s_cnt[2][2][HS_SEL_WAVES];      // [chunk parity][greater | equal][wave]
   const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
   const uint32_t n = min(*n_ptr, cap);
   const uint32_t lo = min((uint32_t)starts[blockIdx.x], n), hi = max(min((uint32_t)starts[blockIdx.x + 1], n), lo);
   const uint8_t *plane = (mk.base && (!mk.present || mk.present[blockIdx.x])) ? mk.base + (long long)blockIdx.x * mk.img_stride : nullptr;
   if (!plane && hi - lo <= limit) {   // nothing to drop
      for (uint32_t i = lo + tid; i < hi; i += HS_SEL_THREADS) keep_rank[i] = i - lo;
      if (tid == 0u) kept[blockIdx.x] = hi - lo;
      return;
   }
   auto eligible = [&](uint32_t i) { return !plane || hs_mask_eligible(plane, mk.row_stride, mk.W, mk.H, kx[i], ky[i]); };
   // ---- threshold: the limit-th largest eligible key.  Invariant: at least `want` eligible keys match (key & mask) == prefix. ----
   uint32_t prefix = 0u, mask = 0u, want = limit;
   bool all = limit == HS_SEL_NO_LIMIT;   // every eligible keypoint is kept: no threshold (block-uniform)
   for (int shift = 24; shift >= 0 && !all; shift -= 8) {
      if (tid < 256u) s_hist[tid] = 0u;
      __syncthreads();
      for (uint32_t i = lo + tid; i < hi; i += HS_SEL_THREADS) {
         const uint32_t key = hs_strength_key(response[i]);
         if ((key & mask) == prefix && eligible(i)) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
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
      // the first pass counts every eligible keypoint: when the limit holds them all there is no cut (read by every thread alike)
      if (shift == 24 && s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3] <= want) { all = true; break; }
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
   const uint32_t T = prefix, q = all ? 0u : want;   // eligible keys above T are kept, and the first q equal to T (1 <= q unless all)
   // ---- ordered pass: keypoint i has gt_before + min(eq_before, q) kept keypoints before it ----
   uint32_t c_gt = 0u, c_eq = 0u;   // counts of the chunks before this one
   int par = 0;
   for (uint32_t base = lo; base < hi; base += HS_SEL_THREADS, par ^= 1) {
      const uint32_t i = base + tid;
      const bool valid = i < hi && eligible(i);
      const uint32_t key = valid ? hs_strength_key(response[i]) : 0u;
      const bool gt = valid && (all || key > T), eq = valid && !all && key == T;
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
      if (i < hi) keep_rank[i] = (gt || (eq && eq_before < q)) ? gt_before + min(eq_before, q) : HS_SEL_DROPPED;
   }
   if (tid == 0u) kept[blockIdx.x] = c_gt + min(c_eq, q);
}

// One block.  starts[b] (in place): where image b's kept keypoints begin; *hess_total: how many are kept in all; *detected: the length
// of the list detection made, for k_hess_deal_kept.  A list that overflowed the capacity is left as it is (*detected = 0: nothing is
// moved), so that the host meets the count it refuses.
__global__ __launch_bounds__(256) void k_select_starts(int32_t *__restrict__ starts, int nimg, const uint32_t *__restrict__ kept, uint32_t cap,
                                                       uint32_t *__restrict__ hess_total, uint32_t *__restrict__ detected)
{
   __shared__ uint32_t s_wave[4];
   const uint32_t total = *hess_total;
   if (threadIdx.x == 0) *detected = total <= cap ? total : 0u;
   if (total > cap) return;
   uint32_t carry = 0u;
   for (int base = 0; base < nimg; base += 256) {
      const int b = base + (int)threadIdx.x;
      const uint32_t v = b < nimg ? kept[b] : 0u;   // (k_select_image: never more than the image's segment of the list)
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
