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
//   k_select_image_grid  hesaff_set_keypoint_grid's twin of it (R x C cells, R * C > 1, with a limit): the Q = N / (R * C) strongest
//                      eligible keypoints of every cell; a threshold and a quota per cell (below, at the kernel).
//   k_select_starts    one block: the per-image starts of the kept list (exclusive scan of the kept counts) and its length.
//   k_hess_deal_kept   k_hess_deal's compacting twin: the kept 32-byte items to their new places in the Hessian list.
//
// The integer histogram is filled with LDS atomics, whose sums do not depend on arrival order; everything that depends on order
// (ties, ranks) comes from wave ballots and counts carried along the segment, so the result is the same for every launch geometry and
// from run to run.  The host does not know the list's length before its one round trip, so nothing here takes it as an argument.
// The mask costs one scattered byte per keypoint and pass: a few thousand bytes per image, which no staging would repay.
#pragma once
#include "kernels_pyramid.h"
#include "select_grid.h"

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
   const int col = hs_sel_pixel(x, W), row = hs_sel_pixel(y, H);
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

// ---- hesaff_set_keypoint_grid: the Q strongest eligible keypoints of every cell of an R x C grid over the image ----
// Keypoint i lies in cell hs_grid_cell(row, col) of its pixel (hs_sel_pixel of y and x: the masks' pixel); an eligible i of cell k is
// kept iff  #{j eligible in k : |r_j| > |r_i|} + #{j < i, eligible in k : |r_j| == |r_i|} < Q.  A sparse cell's unused quota is nobody's.
//
// One block per image, like k_select_image, and the same two phases, per cell:
//   thresholds   MSB-first radix select with one integer histogram per cell: 4-bit digits, eight passes, 64 cells x 16 bins x 4 B =
//                4 KiB of LDS, one bin per thread when it is cleared.  (8-bit digits would halve the passes with 64 KiB of dynamic
//                LDS - two blocks per CU - and a 16384-bin scan per pass; the passes after the first touch few keys, so the short
//                digit costs little.)  The first pass counts every cell's eligible keypoints: a cell with at most Q keeps them all
//                and takes no further part; when every cell does, the passes end.  It also leaves every keypoint's cell (or "not
//                eligible") in keep_rank[i], where the later passes and the ordered pass read it back: x, y, the mask byte and the
//                two divisions are paid once.  Thread t reads and writes only its own i = lo + t (mod the block), so that needs no
//                fence.  Afterwards cell k has its threshold key T_k and the quota q_k of keys equal to T_k that are kept.
//   ordered pass over chunks of the block's size: keypoint i is kept iff its key is above T_k, or equals T_k with fewer than q_k equal
//                keys of cell k before it.  A chunk without a key on its cell's threshold - nearly every chunk - is k_select_image's
//                chunk: one ballot, one barrier.  Otherwise every wave splits its threshold lanes by cell (a loop over the distinct
//                cells among them, one ballot each), leaves each cell's count in s_eqw[wave][cell] stamped with the chunk's number
//                (so that nothing has to be cleared), and after the barrier a threshold lane adds the counts carried from earlier
//                chunks (s_eqc), those of the waves before it and the lanes before it; a second ballot and barrier rank the kept.
// LDS: 4 KiB histogram + 4 KiB s_eqw + 1.5 KiB of per-cell state and wave counts = 9792 B static.  That would allow 16 blocks per
// CU of 160 KiB; the CU's 32 wave slots hold two blocks of 16 waves (48 VGPRs), so waves limit, not LDS - and with one block per
// image a batch rarely puts two on a CU at all.
// The histograms are filled with LDS atomics (integer sums); every order-dependent count comes from ballots and carried counts.
#define HS_SEL_ALL 0xffffffffu   // s_want of a cell that keeps every eligible keypoint
__global__ __launch_bounds__(HS_SEL_THREADS) void k_select_image_grid(const float *__restrict__ response, const float *__restrict__ kx,
                                                                      const float *__restrict__ ky, const int32_t *__restrict__ starts,
                                                                      const uint32_t *__restrict__ n_ptr, uint32_t cap, uint32_t quota, int R, int C,
                                                                      int W, int H, SelMasks mk, uint32_t *keep_rank, uint32_t *__restrict__ kept)
{
   __shared__ uint32_t s_hist[HS_GRID_MAX_CELLS * 16];
   __shared__ uint32_t s_prefix[HS_GRID_MAX_CELLS];           // the digits chosen so far; in the end T_k
   __shared__ uint32_t s_want[HS_GRID_MAX_CELLS];             // what is still wanted inside the prefix; in the end q_k, or HS_SEL_ALL
   __shared__ uint32_t s_eqw[HS_SEL_WAVES][HS_GRID_MAX_CELLS];   // (chunk number << 7) | threshold keys of the cell in the wave's lanes
   __shared__ uint32_t s_eqc[2][HS_GRID_MAX_CELLS];           // threshold keys of the cell in the chunks before this one
   __shared__ uint32_t s_cnt[2][2][HS_SEL_WAVES];             // [chunk parity][above the threshold | on it][wave]
   __shared__ uint32_t s_cnt2[HS_SEL_WAVES];                  // kept per wave, in a chunk with threshold keys
   const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
   const uint32_t ncell = (uint32_t)(R * C);   // 2 .. HS_GRID_MAX_CELLS (hesaff_set_keypoint_grid)
   const uint32_t n = min(*n_ptr, cap);
   const uint32_t lo = min((uint32_t)starts[blockIdx.x], n), hi = max(min((uint32_t)starts[blockIdx.x + 1], n), lo);
   const uint8_t *plane = (mk.base && (!mk.present || mk.present[blockIdx.x])) ? mk.base + (long long)blockIdx.x * mk.img_stride : nullptr;
   if (!plane && hi - lo <= quota) {   // no cell can hold more than its quota
      for (uint32_t i = lo + tid; i < hi; i += HS_SEL_THREADS) keep_rank[i] = i - lo;
      if (tid == 0u) kept[blockIdx.x] = hi - lo;
      return;
   }
   if (tid < HS_GRID_MAX_CELLS) { s_prefix[tid] = 0u; s_want[tid] = quota; s_eqc[0][tid] = 0u; }
   s_eqw[w][lane] = 0xffffffffu;   // a stamp no chunk has
   // ---- thresholds.  Invariant per cell: at least s_want eligible keys of the cell match (key & mask) == s_prefix. ----
   uint32_t mask = 0u;
   for (int shift = 28; shift >= 0; shift -= 4) {
      s_hist[tid] = 0u;   // (HS_SEL_THREADS == HS_GRID_MAX_CELLS * 16)
      __syncthreads();
      for (uint32_t i = lo + tid; i < hi; i += HS_SEL_THREADS) {
         uint32_t cell;
         if (shift == 28) {
            const float x = kx[i], y = ky[i];
            cell = (!plane || hs_mask_eligible(plane, mk.row_stride, mk.W, mk.H, x, y))
                      ? (uint32_t)hs_grid_cell(hs_sel_pixel(y, H), hs_sel_pixel(x, W), R, C, W, H) : HS_SEL_DROPPED;
            keep_rank[i] = cell;
         } else {
            cell = keep_rank[i];
         }
         if (cell == HS_SEL_DROPPED) continue;
         const uint32_t key = hs_strength_key(response[i]);
         if (s_want[cell] != HS_SEL_ALL && (key & mask) == s_prefix[cell]) atomicAdd(&s_hist[cell * 16u + ((key >> shift) & 15u)], 1u);
      }
      __syncthreads();
      // thread k < ncell walks cell k's bins from the top: exactly one holds the want-th largest (the intervals (above, above + h]
      // are disjoint)
      bool active = false;
      if (tid < ncell && s_want[tid] != HS_SEL_ALL) {
         const uint32_t want = s_want[tid];
         uint32_t above = 0u, digit = 0u, rest = want;
         for (int b = 15; b >= 0; b--) {
            const uint32_t h = s_hist[tid * 16u + (uint32_t)b];
            if (above < want && want <= above + h) { digit = (uint32_t)b; rest = want - above; }
            above += h;
         }
         if (shift == 28 && above <= want) {
            s_want[tid] = HS_SEL_ALL;   // the first pass counted every eligible keypoint of the cell: no cut
         } else {
            s_prefix[tid] |= digit << shift;
            s_want[tid] = rest;
            active = true;
         }
      }
      if (!__syncthreads_or(active ? 1 : 0)) break;   // (block-uniform) every cell keeps all it has
      mask |= 15u << shift;
   }
   // ---- ordered pass: keypoint i has as many kept keypoints before it as its rank says ----
   uint32_t c_kept = 0u;   // kept in the chunks before this one
   uint32_t chunk = 0u;
   int par = 0, epar = 0;
   for (uint32_t base = lo; base < hi; base += HS_SEL_THREADS, par ^= 1, chunk++) {
      const uint32_t i = base + tid;
      const uint32_t code = i < hi ? keep_rank[i] : HS_SEL_DROPPED;
      const bool valid = code != HS_SEL_DROPPED;
      const uint32_t cell = valid ? code : 0u;
      const uint32_t key = valid ? hs_strength_key(response[i]) : 0u;
      const uint32_t q = s_want[cell], T = s_prefix[cell];
      const bool gt = valid && (q == HS_SEL_ALL || key > T), eq = valid && q != HS_SEL_ALL && key == T;
      const unsigned long long below = (1ull << lane) - 1ull;
      const unsigned long long m_gt = __ballot(gt), m_eq = __ballot(eq);
      uint32_t eq_before = 0u;   // of a threshold lane: threshold keys of its cell in the lanes before it
      for (unsigned long long rest = m_eq; rest != 0ull;) {   // (wave-uniform) one turn per distinct cell among the threshold lanes
         const int first = __ffsll((long long)rest) - 1;
         const uint32_t cell_f = (uint32_t)__shfl((int)cell, first, 64);
         const bool mine = eq && cell == cell_f;
         const unsigned long long g = __ballot(mine);
         if (mine) eq_before = (uint32_t)__popcll(g & below);
         if ((int)lane == first) s_eqw[w][cell_f] = (chunk << 7) | (uint32_t)__popcll(g);
         rest &= ~g;
      }
      if (lane == 0u) { s_cnt[par][0][w] = (uint32_t)__popcll(m_gt); s_cnt[par][1][w] = (uint32_t)__popcll(m_eq); }
      __syncthreads();   // (the next chunk writes the other half of s_cnt)
      uint32_t gt_before = 0u, n_gt = 0u, n_eq = 0u;
#pragma unroll
      for (uint32_t v = 0; v < HS_SEL_WAVES; v++) {
         const uint32_t a = s_cnt[par][0][v];
         if (v < w) gt_before += a;
         n_gt += a; n_eq += s_cnt[par][1][v];
      }
      if (n_eq == 0u) {   // (block-uniform) nothing on a threshold: above it is kept
         if (i < hi) keep_rank[i] = gt ? c_kept + gt_before + (uint32_t)__popcll(m_gt & below) : HS_SEL_DROPPED;
         c_kept += n_gt;
         continue;
      }
      // counts of s_eqw that carry this chunk's stamp; the others are of earlier chunks
      auto stamped = [&](uint32_t v) { return (v >> 7) == chunk ? (v & 127u) : 0u; };
      bool keep = gt;
      if (eq) {
         eq_before += s_eqc[epar][cell];
         for (uint32_t v = 0; v < w; v++) eq_before += stamped(s_eqw[v][cell]);
         keep = eq_before < q;
      }
      const unsigned long long m_keep = __ballot(keep);
      if (lane == 0u) s_cnt2[w] = (uint32_t)__popcll(m_keep);
      if (tid < ncell) {
         uint32_t sum = s_eqc[epar][tid];
         for (uint32_t v = 0; v < HS_SEL_WAVES; v++) sum += stamped(s_eqw[v][tid]);
         s_eqc[epar ^ 1][tid] = sum;
      }
      __syncthreads();   // (every read of s_eqw and s_eqc[epar] precedes the next chunk's writes)
      epar ^= 1;
      uint32_t keep_before = 0u, n_keep = 0u;
#pragma unroll
      for (uint32_t v = 0; v < HS_SEL_WAVES; v++) {
         const uint32_t a = s_cnt2[v];
         if (v < w) keep_before += a;
         n_keep += a;
      }
      if (i < hi) keep_rank[i] = keep ? c_kept + keep_before + (uint32_t)__popcll(m_keep & below) : HS_SEL_DROPPED;
      c_kept += n_keep;
   }
   if (tid == 0u) kept[blockIdx.x] = c_kept;
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
