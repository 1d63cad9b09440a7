// kernels_keypoint.h -- per-keypoint kernels: Baumberg affine iteration, up-is-up
// rectification + border test, affine patch normalisation, SIFT descriptor, result packing.
// Reference: affine.cpp, helpers.cpp, siftdesc.cpp, hesaff.cpp:72-105.
//
// Float sums that the reference accumulates sequentially (SMM sums affine.cpp:57-68,
// photometric mean/variance helpers.cpp:253-266, histogram cells siftdesc.cpp:75-78, norms
// siftdesc.cpp:86-90) are accumulated in the SAME order here: one lane per sum, or one
// thread per histogram cell walking its pixels in raster order.  No shuffle trees, no
// float atomics (both would change the rounding and flip descriptor bytes).
#pragma once
#include <type_traits>
#include "device_common.h"
#include "kernels_pyramid.h"

struct PlaneTab {   // prevBlur planes of the batch: L[octave][level], level 0..2
   DPlane L[HS_MAX_OCTAVES][HS_NSCALES];
};

struct KpTables {   // device tables built on the host once per context
   const float *smm_mask;    // 19x19 computeGaussMask, helpers.cpp:104
   const float *sift_mask;   // 41x41 computeCircularGaussMask, helpers.cpp:131
   const int32_t *mask_idx;  // raster-ordered indices of the pixels with sift_mask > 0
   int n_masked;
   // per masked pixel (slot order = mask_idx order, padded to 1280): the constants k_sift_grad needs for it, so that a
   // thread fetches them in one round of loads: {left, right, up, down} stencil neighbours as LDS byte offsets into the
   // patch, and {output slot r * 40 + c (or -1: row / column 40, no weight), mask value bits}
   const int4 *sgrad_nb;
   const int2 *sgrad_om;
   // layout of a keypoint's gradient pairs in HBM (kernels_sift.h: HS_VO_ITEMS): per patch row r < 40 {first item of the row in the
   // keypoint's block minus f_lo, f_lo, f_hi, 0} in 16-byte items (an empty row: f_lo > f_hi), and per item of the block the item of
   // k_sift_grad's 40 x 20 LDS tile it is a copy of (padding items: tile item 0, which holds no masked pixel)
   const int4 *vo_rows;
   const uint16_t *vo_src;
   const int32_t *bin0, *bin1;   // precomputeBinsAndWeights siftdesc.cpp:18 (already x8)
   const float *w0, *w1;
   const float *patch_taps;      // Gaussian taps of every odd P0, concatenated
   const int32_t *patch_tap_off; // offset of P0's taps at index (P0-1)/2
   const int32_t *patch_tap_k;   // K of P0
   int max_p0;
};

// ---------------------------------------------------------------------------------------
// k_affine: AffineShape::findAffineShape affine.cpp:35-100.
//  per iteration: 361 bilinear taps -> LDS img; gradients and the three products per pixel ->
//  LDS; three lanes add the 361 terms of a,b,c in index order; one lane runs the
//  double-precision invSqrt and the U update.
// ---------------------------------------------------------------------------------------
// (AffineOut: device_lists.h)

// interpolate()'s return flag ("some tap fell outside the image", helpers.cpp:209-244) for the P x P window of
// normalizeAffine's smoothing branch (affine.cpp:126), without visiting the P^2 taps.  The tap coordinate
//    w(j, i) = fl(fl(ofs + fl(j * a_row)) + fl(i * a_col))        j, i in [-half, half]
// is monotone in i for fixed j and in j for fixed i (a float product or sum with one operand fixed is monotone under
// round-to-nearest), so over the grid it takes its extremes at the four corners; a tap is inside iff
// 0 <= floor(w) < limit, i.e. 0 <= w < limit for the integer limits cols - 1 / rows - 1.  Hence "some tap outside" <=>
// "some corner outside".  Non-finite values: an infinite product at an inner index is also infinite at the corner of the
// same sign, and a NaN operand makes every coordinate NaN, so a corner fails whenever any tap would.
__device__ inline bool hs_window_outside(int imRows, int imCols, float ofsx, float ofsy, float a11, float a12, float a21, float a22, int half)
{
   const float width = (float)(imCols - 1), height = (float)(imRows - 1);
   bool outside = false;
#pragma unroll
   for (int q = 0; q < 4; q++) {
      const int j = (q & 1) ? half : -half, i = (q & 2) ? half : -half;
      const float rx = ofsx + (float)j * a12, ry = ofsy + (float)j * a22;
      const float fx = floorf(rx + (float)i * a11), fy = floorf(ry + (float)i * a21);
      outside = outside || !(fx >= 0.0f && fy >= 0.0f && fx < width && fy < height);
   }
   return outside;
}

// ---------------------------------------------------------------------------------------
// hs_affine_groups: the same iteration with SIXTEEN persistent keypoint slots per wavefront.
// Per iteration a keypoint needs 361 parallel taps + products, then three 361-term sequential
// sums and one double-precision invSqrt.  A round of the wavefront serves every active slot once:
//   * four batches q = 0..3.  In batch q the four 16-lane groups serve slots 4q .. 4q+3: corner test, taps (the untested
//     variant when the windows of all the batch's active slots are inside), gradients and products, and the three sums in
//     index order on 12 lanes, which leave a, b, c in s_abc[slot].  Every batch uses the same s_arr; a batch none of whose
//     slots is active is skipped.
//   * one tail: lane s < 16 owns slot s.  It runs invSqrt, the U update and the convergence logic on s_abc[s], so the
//     double-precision stretch is executed once per round for sixteen keypoints.  The slot's iteration state (keypoint
//     index, iteration count, U, both eigen ratios) lives in that lane's registers; a slot whose keypoint converged or was
//     rejected stores the result and takes the block's next keypoint there, so keypoints with different iteration counts
//     do not wait for each other.
// What the sampling lanes need of a slot (plane, extent, position, ratio, U, active flag) is published by the tail lane in
// the slot's LDS record and read by the slot's group at the start of its batch.  An inactive slot's record holds no valid
// plane pointer: its group neither samples nor sums.
// Every keypoint goes through the operations of the single-keypoint form on the same operands in the same order.
// block = 64 threads (one wavefront), LDS 4 x 3 x 364 floats + mask + 16 records + s_abc (19.5 KB: eight blocks per CU).
// ---------------------------------------------------------------------------------------
// One pass of the iteration's tail, affine.cpp:72-97, on the three sums a, b, c of a keypoint: invSqrt, the eigen ratio, the U update
// (n = [a b; b c] * u), getEigenvalues and the two decisions.  a, b, c leave as invSqrt's; l1, l2 as invSqrt's where getEigenvalues
// refuses, else as getEigenvalues'.  Returns 0 continue, 1 break (rejected), 2 converged.
__device__ __forceinline__ int hs_affine_tail(float &a, float &b, float &c, float u11, float u12, float u21, float u22, float &eigen_ratio_act,
                                              float &eigen_ratio_bef, float convergenceThreshold, float &l1, float &l2, float &n11, float &n12,
                                              float &n21, float &n22)
{
   hs_inv_sqrt(a, b, c, l1, l2);
   eigen_ratio_bef = eigen_ratio_act;
   eigen_ratio_act = 1 - l2 / l1;
   const float u11t = u11, u12t = u12;
   n11 = a * u11t + b * u21; n12 = a * u12t + b * u22;
   n21 = b * u11t + c * u21; n22 = b * u12t + c * u22;
   int state = 0;
   if (!hs_eigenvalues(n11, n12, n21, n22, l1, l2)) state = 1;
   else if ((l1 / l2 > 6) || (l2 / l1 > 6)) state = 1;
   else if (eigen_ratio_act < convergenceThreshold && eigen_ratio_bef < convergenceThreshold) state = 2;
   return state;
}

#define HS_AFF_SLOTS 16   // keypoints a wavefront iterates on at a time; the launch sites size their grids by it
// consecutive keypoints a block takes from the list at a time.  Alone on the device, per 32 UHD images: 16 -> 22.1 ms, 4 -> 19.2 ms,
// 1 -> 18.2 ms (the four-group form: 21.1 ms).  All blocks of a launch are resident, so the launch lasts as long as its largest share.
#define HS_AFF_ITEM 1
// a batch: four keypoints side by side, 16 lanes each (two keypoints of 32 lanes would halve the LDS per wavefront and double
// the wavefronts per CU, but the serial sums would then serve two keypoints instead of four)
#define HS_AFFP_G 4
#define HS_AFFP_L (64 / HS_AFFP_G)
#define HS_AFFP_SH 4    // log2(HS_AFFP_L)
#define HS_AFFP_NT ((HS_SMM_PIX + HS_AFFP_L - 1) / HS_AFFP_L)
#define HS_AFF_BATCHES 2
#define HS_AFF_ARR 364  // 361 rounded up to a multiple of 4 floats
// a slot's record, 32-bit words
enum { HS_AFR_PTR_LO, HS_AFR_PTR_HI, HS_AFR_PITCH, HS_AFR_WIDTH, HS_AFR_HEIGHT, HS_AFR_LX, HS_AFR_LY, HS_AFR_RATIO,
       HS_AFR_U11, HS_AFR_U12, HS_AFR_U21, HS_AFR_U22, HS_AFR_ACTIVE, HS_AFR_WORDS };

struct AffKp { const float *blur; int rows, cols, pitch; float x, y, s, pd; };

template <class Fetch>
__device__ __forceinline__ void hs_affine_groups(uint32_t first, uint32_t n, const float *__restrict__ mask_g, const DConsts &k, AffineOut out,
                                                 Fetch fetch)
{
   __shared__ __attribute__((aligned(16))) float s_arr[HS_AFFP_G][3][HS_AFF_ARR];   // img, then a terms | b terms | c terms
   __shared__ float s_mask[HS_AFF_ARR];
   __shared__ float s_abc[HS_AFF_SLOTS][3];
   __shared__ uint32_t s_slot[HS_AFF_SLOTS][HS_AFR_WORDS];
   const int lane = threadIdx.x, grp = lane >> HS_AFFP_SH, li = lane & (HS_AFFP_L - 1);
   const bool tail_lane = lane < HS_AFF_SLOTS;   // lane s owns slot s
   for (int i = lane; i < HS_SMM_PIX; i += 64) s_mask[i] = mask_g[i];
   float *s_img = s_arr[grp][0], *s_pa = s_arr[grp][0], *s_pb = s_arr[grp][1], *s_pc = s_arr[grp][2];   // the a terms replace the image
   // A block walks the list in items of HS_AFF_ITEM consecutive keypoints at the block's stride.  Position p of its walk is
   // keypoint p % HS_AFF_ITEM of its item p / HS_AFF_ITEM; the slots start on positions 0..15, and a slot that finishes takes
   // the next position no slot has taken yet, so the slots of a block run dry together however unevenly the iteration
   // counts fall.  (With a fixed stride per slot a block waits for its unluckiest slot with most batches a quarter full:
   // 26.2 ms against the four-group form's 21.3 ms per 32 UHD images.)
   // XCD-aware order: block b runs on XCD b % 8 (observed dispatch order, a speed assumption only).  The keypoints are
   // ordered by image, octave, level and raster position, so neighbours in the list sample the same cache lines of the
   // same plane: each XCD takes one contiguous eighth of the list, its blocks stride inside that eighth, and those lines
   // are fetched into ONE private L2 instead of eight.  (Grids that are not a multiple of 8 blocks keep the plain stride.)
   uint32_t hstep = gridDim.x * HS_AFF_ITEM, h_end = n;
   uint32_t h0 = first + blockIdx.x * HS_AFF_ITEM;   // the block's first item
   if ((gridDim.x & 7u) == 0u && n > first) {
      const uint32_t n_items = (n - first + HS_AFF_ITEM - 1) / HS_AFF_ITEM;
      const uint32_t xcd = blockIdx.x & 7u, rank = blockIdx.x >> 3, per_xcd = gridDim.x >> 3;
      const uint32_t it_lo = (uint32_t)(((unsigned long long)n_items * xcd) >> 3), it_hi = (uint32_t)(((unsigned long long)n_items * (xcd + 1)) >> 3);
      hstep = per_xcd * HS_AFF_ITEM;
      h_end = min(first + it_hi * HS_AFF_ITEM, n);
      h0 = first + (it_lo + rank) * HS_AFF_ITEM;
   }
   auto walk = [&](uint32_t p) { return h0 + (p / HS_AFF_ITEM) * hstep + (p % HS_AFF_ITEM); };
   uint32_t h = walk((uint32_t)lane);
   uint32_t next_p = HS_AFF_SLOTS;   // first position of the block's walk that no slot has taken (wave-uniform)
   if (k.maxIterations <= 0) {   // no iteration: U = identity, not converged
      if (lane < HS_AFF_ITEM)
         for (; h < h_end; h += hstep) {
            out.converged[h] = 0; out.iters[h] = 0;
            out.U[4 * h + 0] = 1.0f; out.U[4 * h + 1] = 0.0f; out.U[4 * h + 2] = 0.0f; out.U[4 * h + 3] = 1.0f;
         }
      return;
   }
   // the slot's iteration state, in its tail lane (the other lanes stay inactive and hold nothing)
   int l = 0;
   float u11 = 1.0f, u12 = 0.0f, u21 = 0.0f, u22 = 1.0f;
   float eigen_ratio_act = 0.0f, eigen_ratio_bef = 0.0f;
   bool active = tail_lane && h < h_end;
   // the slot takes keypoint h (or goes idle): the tail lane resets its state and publishes the record
   auto load_kp = [&]() {
      uint32_t *rec = s_slot[lane];
      rec[HS_AFR_ACTIVE] = active ? 1u : 0u;
      if (active) {
         const AffKp q = fetch(h);
         const unsigned long long pa = reinterpret_cast<unsigned long long>(q.blur);
         rec[HS_AFR_PTR_LO] = (uint32_t)pa; rec[HS_AFR_PTR_HI] = (uint32_t)(pa >> 32);
         rec[HS_AFR_PITCH] = (uint32_t)q.pitch; rec[HS_AFR_WIDTH] = (uint32_t)(q.cols - 1); rec[HS_AFR_HEIGHT] = (uint32_t)(q.rows - 1);
         rec[HS_AFR_LX] = __float_as_uint(q.x / q.pd); rec[HS_AFR_LY] = __float_as_uint(q.y / q.pd);
         rec[HS_AFR_RATIO] = __float_as_uint(q.s / (k.affInitialSigma * q.pd));
         u11 = 1.0f; u12 = 0.0f; u21 = 0.0f; u22 = 1.0f;
         rec[HS_AFR_U11] = __float_as_uint(u11); rec[HS_AFR_U12] = __float_as_uint(u12);
         rec[HS_AFR_U21] = __float_as_uint(u21); rec[HS_AFR_U22] = __float_as_uint(u22);
         eigen_ratio_act = 0.0f; eigen_ratio_bef = 0.0f;
         l = 0;
      }
   };
   if (tail_lane) load_kp();
   HS_WAVE_LDS_SYNC();
   while (__ballot(active) != 0ull) {
#pragma unroll 1
      for (int q = 0; q < HS_AFF_SLOTS / HS_AFFP_G; q++) {
         const int slot = q * HS_AFFP_G + grp;
         const uint32_t *rec = s_slot[slot];
         const bool act = rec[HS_AFR_ACTIVE] != 0u;   // this group's slot iterates in this round
         if (__ballot(act) == 0ull) continue;
         // the slot's record, replicated in the group's 16 lanes (an inactive slot's is stale: read, never used)
         // (rebuilt as a pointer into global memory: from a bare integer the taps would become flat loads, which also wait on the LDS counter)
         typedef const __attribute__((address_space(1))) float *hs_gptr;
         const float *blur = (const float *)(hs_gptr)(((unsigned long long)rec[HS_AFR_PTR_HI] << 32) | rec[HS_AFR_PTR_LO]);
         const int pitch = (int)rec[HS_AFR_PITCH], width = (int)rec[HS_AFR_WIDTH], height = (int)rec[HS_AFR_HEIGHT];
         const float lx = __uint_as_float(rec[HS_AFR_LX]), ly = __uint_as_float(rec[HS_AFR_LY]), ratio = __uint_as_float(rec[HS_AFR_RATIO]);
         const float su11 = __uint_as_float(rec[HS_AFR_U11]), su12 = __uint_as_float(rec[HS_AFR_U12]);
         const float su21 = __uint_as_float(rec[HS_AFR_U21]), su22 = __uint_as_float(rec[HS_AFR_U22]);
         bool win_in = true;
         if (act) {
            const float a11 = su11 * ratio, a12 = su12 * ratio, a21 = su21 * ratio, a22 = su22 * ratio;
            // interpolate(), helpers.cpp:209-244 (return value ignored at affine.cpp:47): 23 taps per lane in two batches.
            // The tap coordinates are monotone in i and in j (hs_window_outside): when the four corners of the 19 x 19 grid
            // are inside the level, every tap is, and the taps need no bounds test, no selects and only 32-bit offsets;
            // a window that touches the border (a few per cent) keeps the tested tap, which zeroes what lies outside.
            win_in = !hs_window_outside(height + 1, width + 1, lx, ly, a11, a12, a21, a22, HS_SMM >> 1);
         }
         // one decision per batch (a branch per group would split the batches of gathers): the untested taps when the
         // windows of all its active slots are inside, the tested ones for everybody otherwise
         const bool all_in = __ballot(act && !win_in) == 0ull;
         auto sample = [&](auto inside_c) {
            constexpr bool INSIDE = decltype(inside_c)::value;
            const float a11 = su11 * ratio, a12 = su12 * ratio, a21 = su21 * ratio, a22 = su22 * ratio;
#pragma unroll
            for (int half = 0; half < HS_AFF_BATCHES; half++) {
               constexpr int NB = (HS_AFFP_NT + HS_AFF_BATCHES - 1) / HS_AFF_BATCHES;
               float sv[NB];
#pragma unroll
               for (int t = 0; t < NB; t++) {
                  const int idx = min(li + HS_AFFP_L * (half * NB + t), HS_SMM_PIX - 1);
                  const int jj = idx / HS_SMM, ii = idx - jj * HS_SMM;
                  const int j = jj - (HS_SMM >> 1), i = ii - (HS_SMM >> 1);
                  const float rx = lx + (float)j * a12;
                  const float ry = ly + (float)j * a22;
                  const float wx = rx + (float)i * a11;
                  const float wy = ry + (float)i * a21;
                  if (INSIDE) {
                     sv[t] = hs_tap_inside_ptr(blur, pitch, wx, wy);
                  } else {
                     bool outside = false;
                     sv[t] = hs_bilinear(blur, pitch, width, height, wx, wy, outside);
                  }
               }
#pragma unroll
               for (int t = 0; t < NB; t++) HS_KEEP(sv[t]);
#pragma unroll
               for (int t = 0; t < NB; t++) {
                  const int idx = li + HS_AFFP_L * (half * NB + t);
                  if (idx < HS_SMM_PIX) s_img[idx] = sv[t];
               }
            }
         };
         if (act) {
            if (all_in) sample(std::true_type{});
            else sample(std::false_type{});
         }
         HS_WAVE_LDS_SYNC();
         if (act) {
            // computeGradient affine.cpp:14-33 + products affine.cpp:62-68.  The a terms take the place of
            // the sampled image in LDS, so they wait in registers until every lane has read its neighbours.
            float pa[HS_AFFP_NT];
#pragma unroll
            for (int t = 0; t < HS_AFFP_NT; t++) {
               const int idx = min(li + HS_AFFP_L * t, HS_SMM_PIX - 1);
               const int r = idx / HS_SMM, c = idx - r * HS_SMM;
               // hs_grad with clamped neighbour indices (one-sided differences at the tile border)
               const float gxx = s_img[idx + (c < HS_SMM - 1 ? 1 : 0)] - s_img[idx - (c > 0 ? 1 : 0)];
               const float gyy = s_img[idx + (r < HS_SMM - 1 ? HS_SMM : 0)] - s_img[idx - (r > 0 ? HS_SMM : 0)];
               const float v = s_mask[idx];
               const float gxy = gxx * gyy;
               pa[t] = gxx * gxx * v;
               if (li + HS_AFFP_L * t < HS_SMM_PIX) {
                  s_pb[idx] = gxy * v;
                  s_pc[idx] = gyy * gyy * v;
               }
            }
            HS_WAVE_LDS_SYNC();
#pragma unroll
            for (int t = 0; t < HS_AFFP_NT; t++) {
               const int idx = li + HS_AFFP_L * t;
               if (idx < HS_SMM_PIX) s_pa[idx] = pa[t];
            }
         }
         HS_WAVE_LDS_SYNC();
         if (act && li < 3) {
            // 361 terms in index order (affine.cpp:57-68); float4 LDS reads, the adds stay sequential
            const float *pp = s_arr[grp][li];
            const float4 *p4 = reinterpret_cast<const float4 *>(pp);
            float acc = 0.0f;
            for (int i0 = 0; i0 < HS_SMM_PIX / 4; i0 += 10) {   // 90 = 9 x 10 float4, ten reads in flight
               float4 q4[10];
#pragma unroll
               for (int u = 0; u < 10; u++) q4[u] = p4[i0 + u];
#pragma unroll
               for (int u = 0; u < 10; u++) { acc += q4[u].x; acc += q4[u].y; acc += q4[u].z; acc += q4[u].w; }
            }
            acc += pp[HS_SMM_PIX - 1];   // 361 = 4 * 90 + 1
            s_abc[slot][li] = acc / (float)HS_SMM_PIX;
         }
         HS_WAVE_LDS_SYNC();   // the next batch's taps overwrite the terms; the tail reads s_abc
      }
      bool finished = false;
      if (active) {   // the tail: one lane per active slot
         float a = s_abc[lane][0], b = s_abc[lane][1], c = s_abc[lane][2];
         float l1, l2, n11, n12, n21, n22;
         const int state = hs_affine_tail(a, b, c, u11, u12, u21, u22, eigen_ratio_act, eigen_ratio_bef, k.convergenceThreshold, l1, l2, n11, n12, n21, n22);
         u11 = n11; u12 = n12; u21 = n21; u22 = n22;
         if (state != 0 || l + 1 >= k.maxIterations) {
            // affine.cpp:88-99: converged -> onAffineShapeFound(..., l); otherwise the keypoint is dropped
            out.converged[h] = (state == 2) ? 1 : 0;
            out.iters[h] = (state == 2) ? l : 0;
            out.U[4 * h + 0] = u11; out.U[4 * h + 1] = u12; out.U[4 * h + 2] = u21; out.U[4 * h + 3] = u22;
            finished = true;
         } else {
            uint32_t *rec = s_slot[lane];
            rec[HS_AFR_U11] = __float_as_uint(u11); rec[HS_AFR_U12] = __float_as_uint(u12);
            rec[HS_AFR_U21] = __float_as_uint(u21); rec[HS_AFR_U22] = __float_as_uint(u22);
            l++;
         }
      }
      // the finished slots take the next positions of the block's walk, in slot order
      const unsigned long long fin = __ballot(finished);
      if (finished) {
         const uint32_t p = next_p + (uint32_t)__popcll(fin & ((1ull << lane) - 1ull));
         h = walk(p);
         active = h < h_end;
         load_kp();
      }
      next_p += (uint32_t)__popcll(fin);
      HS_WAVE_LDS_SYNC();
   }
}

__global__ __launch_bounds__(64) void k_affine(PlaneTab pt, HessList hl, uint32_t h_lo, uint32_t h_hi, const uint32_t *__restrict__ n_ptr,
                                               KpTables tb, DConsts k, AffineOut out)
{
   const uint32_t n = min(min(*n_ptr, hl.cap), h_hi);   // keypoints [h_lo, h_hi) of the list
   hs_affine_groups(
      h_lo, n, tb.smm_mask, k, out, [&](uint32_t h) {
      const int meta = hl.meta[h];
      const int b = meta >> 8, octave = (meta >> 4) & 15, level = (meta >> 2) & 3;
      const DPlane &P = pt.L[octave][level];
      AffKp q;
      q.blur = P.img(b); q.rows = P.rows; q.cols = P.cols; q.pitch = P.pitch;
      q.x = hl.x[h]; q.y = hl.y[h]; q.s = hl.s[h]; q.pd = k.pd0 * (float)(1 << octave);
      return q;
   });
}

// stage API flavour: n keypoints on a single plane, pixelDistance given explicitly
__global__ __launch_bounds__(64) void k_affine_stage(DPlane P, const float *__restrict__ kp /*n x 4*/, int n, KpTables tb, DConsts k,
                                                     AffineOut out)
{
   hs_affine_groups(0u, (uint32_t)n, tb.smm_mask, k, out, [&](uint32_t h) {
      AffKp q;
      q.blur = P.img(0); q.rows = P.rows; q.cols = P.cols; q.pitch = P.pitch;
      q.x = kp[4 * h]; q.y = kp[4 * h + 1]; q.s = kp[4 * h + 2]; q.pd = kp[4 * h + 3];
      return q;
   });
}

// hs_affine_tail on caller-supplied operands, thread per row: abc[n][3] and U[n][4] in and out, ratio[n] in (eigen_ratio_act of the
// pass before) and out, l[n][4] = l1, l2 of invSqrt then l1, l2 as the tail leaves them, state[n] (0 continue, 1 rejected, 2 converged)
__global__ void k_affine_tail_stage(int n, float convergenceThreshold, float *abc, float *U, float *ratio, float *l, int32_t *state)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i >= n) return;
   float a = abc[3 * i], b = abc[3 * i + 1], c = abc[3 * i + 2];
   float eigen_ratio_act = ratio[i], eigen_ratio_bef = 0.0f;
   float l1, l2, n11, n12, n21, n22;
   // (invSqrt's l1, l2: the tail's first statement, once more, since the tail goes on to overwrite them)
   { float a0 = a, b0 = b, c0 = c; hs_inv_sqrt(a0, b0, c0, l1, l2); l[4 * i] = l1; l[4 * i + 1] = l2; }
   const int st = hs_affine_tail(a, b, c, U[4 * i], U[4 * i + 1], U[4 * i + 2], U[4 * i + 3], eigen_ratio_act, eigen_ratio_bef, convergenceThreshold,
                                 l1, l2, n11, n12, n21, n22);
   abc[3 * i] = a; abc[3 * i + 1] = b; abc[3 * i + 2] = c;
   U[4 * i] = n11; U[4 * i + 1] = n12; U[4 * i + 2] = n21; U[4 * i + 3] = n22;
   ratio[i] = eigen_ratio_act;
   l[4 * i + 2] = l1; l[4 * i + 3] = l2;
   state[i] = st;
}

// ---------------------------------------------------------------------------------------
// k_prepare_patch: onAffineShapeFound hesaff.cpp:72-82 up to the border test of
// normalizeAffine affine.cpp:108-113: rectify (helpers.cpp:90-97), mrScale / P0 / scale,
// interpolateCheckBorders.  Thread per keypoint.  Survivors are binned by window size P so
// that each patch kernel launch has a uniform LDS footprint.
// ---------------------------------------------------------------------------------------
// (HS_NBINS bins with HS_BIN3_PMAX as the last bound: plan_consts.h)
__host__ __device__ inline int hs_patch_bin(int P) { return P <= 41 ? 0 : (P <= 64 ? 1 : (P <= 128 ? 2 : (P <= HS_BIN3_PMAX ? 3 : 4))); }

// (PatchWork: device_lists.h)

// window side of normalizeAffine's smoothing branch from the scale alone (affine.cpp:106-109,120): 0 when P0 is out of range
__device__ __forceinline__ int hs_window_p0(float s, float mrSize)
{
   const float mrScale = ceilf(s * mrSize);
   // int(mrScale): saturate; the tap table bound rejects such a window anyway
   const int m = (mrScale < 1.0e6f) ? (int)mrScale : 1000000;
   return 2 * m + 1;
}

// Upper bound, per image, of the T' rows the huge windows (last bin) of its keypoints need: depends on the scales
// only, so it is known right after detection and the host can size / group the patch stage without waiting for the
// affine iteration.  rows[b] += P for every Hessian keypoint whose window falls into the last bin.
// rows[nimg + 1] (one past the per-image sums: StartsBlock::largest_window() of batch_plan.h, rows being its large_rows()) receives the
// largest such P of the batch: the row kernel's LDS is sized for the
// windows that exist, not for the largest the image could hold.
// A window wider than the tabulated taps (max_p0) is never extracted (k_prepare_patch rejects it): it adds no rows.
__global__ __launch_bounds__(256) void k_image_large_rows(HessList hl, const uint32_t *__restrict__ n_ptr, float mrSize, uint32_t *__restrict__ rows, int nimg,
                                                          int max_p0);

// ONLY_ALIVE (k_prepare_patch_second, kernels_orient.h): a keypoint whose alive flag is already 0 stays rejected.
template <bool RECTIFY, bool ONLY_ALIVE = false>
__device__ __forceinline__ void hs_prepare_patch_body(const HessList &hl, uint32_t h_lo, uint32_t n, const AffineOut &aff, int imRows, int imCols,
                                                      const DConsts &k, const KpTables &tb, const PatchWork &pw)
{
   for (uint32_t h0 = h_lo + blockIdx.x * blockDim.x; h0 < n; h0 += gridDim.x * blockDim.x) {
      const uint32_t h = h0 + threadIdx.x;
      const bool valid = h < n;
      int alive = 0, P0 = 0;
      if (valid && (!RECTIFY || aff.converged[h]) && (!ONLY_ALIVE || pw.alive[h])) {
         float a11, a12, a21, a22;
         if (RECTIFY) {
            a11 = aff.U[4 * h]; a12 = aff.U[4 * h + 1]; a21 = aff.U[4 * h + 2]; a22 = aff.U[4 * h + 3];
            hs_rectify(a11, a12, a21, a22);
            pw.A[4 * h] = a11; pw.A[4 * h + 1] = a12; pw.A[4 * h + 2] = a21; pw.A[4 * h + 3] = a22;
         } else {
            a11 = pw.A[4 * h]; a12 = pw.A[4 * h + 1]; a21 = pw.A[4 * h + 2]; a22 = pw.A[4 * h + 3];
         }
         P0 = hs_window_p0(hl.s[h], k.mrSize);
         const float scale = (float)P0 / (float)HS_PATCH;
         bool rej = hs_check_borders(imRows, imCols, hl.x[h], hl.y[h], a11 * scale, a12 * scale, a21 * scale, a22 * scale);
         // smoothing branch (affine.cpp:114-135): a window that leaves the image rejects the keypoint
         if (!rej && (double)scale > 0.4) rej = hs_window_outside(imRows, imCols, hl.x[h], hl.y[h], a11, a12, a21, a22, (P0 + 2) >> 1);
         // P0 > max_p0: the P x P window cannot fit into the image (a11*a22 = 1), the window test has
         // rejected it; no taps are tabulated for it.
         alive = (!rej && P0 <= tb.max_p0) ? 1 : 0;
      }
      if (valid) {
         pw.alive[h] = alive;
         pw.P0[h] = alive ? P0 : 0;
      }
      int bin = -1;
      if (alive) {
         const float scale = (float)P0 / (float)HS_PATCH;
         const int P = ((double)scale > 0.4) ? P0 + 2 : 0;
         bin = hs_patch_bin(P);
      }
      // one atomic per (wave, bin) instead of one per keypoint
      const int lane = threadIdx.x & 63;
#pragma unroll
      for (int bq = 0; bq < HS_NBINS; bq++) {
         const unsigned long long m = __ballot(bin == bq);
         if (m == 0ull) continue;
         const int leader = __ffsll((long long)m) - 1;
         uint32_t base = 0;
         if (lane == leader) base = atomicAdd(pw.bin_count + bq, (uint32_t)__popcll(m));
         base = __shfl(base, leader, 64);
         if (bin == bq) pw.bin_items[(size_t)bq * pw.cap + base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = h;
      }
   }
}

__global__ __launch_bounds__(256) void k_image_large_rows(HessList hl, const uint32_t *__restrict__ n_ptr, float mrSize, uint32_t *__restrict__ rows, int nimg,
                                                          int max_p0)
{
   const uint32_t n = min(*n_ptr, hl.cap);
   for (uint32_t h = blockIdx.x * blockDim.x + threadIdx.x; h < n; h += gridDim.x * blockDim.x) {
      const int P0 = hs_window_p0(hl.s[h], mrSize);
      const float scale = (float)P0 / (float)HS_PATCH;
      const int P = ((double)scale > 0.4) ? P0 + 2 : 0;
      if (hs_patch_bin(P) == HS_NBINS - 1 && P0 < (1 << 20) && P0 <= max_p0) {
         atomicAdd(rows + (hl.meta[h] >> 8), (uint32_t)P);
         atomicMax(rows + nimg + 1, (uint32_t)P);
      }
   }
}

__global__ __launch_bounds__(256) void k_prepare_patch(HessList hl, uint32_t h_lo, uint32_t h_hi, const uint32_t *__restrict__ n_ptr, AffineOut aff,
                                                       int imRows, int imCols, DConsts k, KpTables tb, PatchWork pw)
{
   hs_prepare_patch_body<true>(hl, h_lo, min(min(*n_ptr, hl.cap), h_hi), aff, imRows, imCols, k, tb, pw);   // keypoints [h_lo, h_hi) of the list
}

// stage API: the rectified matrices are already in pw.A (normalizeAffine's own arguments)
__global__ __launch_bounds__(256) void k_prepare_patch_given_A(HessList hl, const uint32_t *__restrict__ n_ptr, int imRows, int imCols,
                                                               DConsts k, KpTables tb, PatchWork pw)
{
   AffineOut none;
   none.converged = nullptr; none.U = nullptr; none.iters = nullptr;
   hs_prepare_patch_body<false>(hl, 0u, min(*n_ptr, hl.cap), none, imRows, imCols, k, tb, pw);
}

// ---------------------------------------------------------------------------------------
// k_pack: stable compaction of the described keypoints into hesaff_keypoint records
// (hesaff.cpp:87-91), rank from the exclusive scan of `alive`.
// ---------------------------------------------------------------------------------------
// (KeyRec and HS_PACK_DW, the dwords of a record: device_lists.h)

// A block takes 64 consecutive Hessian keypoints: their head fields come in as coalesced runs of the nine arrays, their descriptors as one
// 8 KB run, the records are assembled in LDS in rank order - the ranks of a run's survivors are consecutive (stable compaction) - and leave as
// ONE contiguous run of dwords.  (Round 4's form - 32 lanes per keypoint, lane 0 fetching nine fields from nine lines and storing nine
// dwords - ran at 2.2 TB/s: 4.6 ms per 256 UHD images; profiles/r05_notes.md.)
#define HS_PACK_KP 64
__global__ __launch_bounds__(256) void k_pack(HessList hl, const uint32_t *__restrict__ n_ptr, PatchWork pw,
                                              const uint32_t *__restrict__ rank, const uint8_t *__restrict__ desc, KeyRec *__restrict__ out)
{
   static_assert(sizeof(KeyRec) == 4 * HS_PACK_DW, "record layout");
   __shared__ uint32_t s_rec[HS_PACK_KP * HS_PACK_DW];
   __shared__ int s_lr[HS_PACK_KP];   // rank inside the block's run of records, -1: not described
   const uint32_t n = min(*n_ptr, hl.cap);
   const int tid = threadIdx.x;
   const uint32_t *desc32 = reinterpret_cast<const uint32_t *>(desc);
   uint32_t *out32 = reinterpret_cast<uint32_t *>(out);
   for (uint32_t h0 = blockIdx.x * HS_PACK_KP; h0 < n; h0 += gridDim.x * HS_PACK_KP) {
      const uint32_t base = rank[h0];   // exclusive scan of `alive`: records of earlier keypoints
      if (tid < HS_PACK_KP) {
         const uint32_t h = h0 + tid;
         const bool live = h < n && pw.alive[h];
         const int lr = live ? (int)(rank[h] - base) : -1;
         s_lr[tid] = lr;
         if (live) {
            uint32_t *r = s_rec + lr * HS_PACK_DW;
            const float4 A = *reinterpret_cast<const float4 *>(pw.A + 4 * (size_t)h);
            r[0] = __float_as_uint(hl.x[h]); r[1] = __float_as_uint(hl.y[h]); r[2] = __float_as_uint(hl.s[h]);
            r[3] = __float_as_uint(A.x); r[4] = __float_as_uint(A.y); r[5] = __float_as_uint(A.z); r[6] = __float_as_uint(A.w);
            r[7] = __float_as_uint(hl.response[h]);
            r[8] = (uint32_t)(hl.meta[h] & 3);
         }
      }
      __syncthreads();
      int n_live = 0;
#pragma unroll
      for (int q = 0; q < HS_PACK_KP * 32 / 256; q++) {
         const int idx = tid + 256 * q, j = idx >> 5, d = idx & 31;
         const int lr = s_lr[j];
         if (lr >= 0) s_rec[lr * HS_PACK_DW + 9 + d] = desc32[(size_t)(h0 + j) * 32 + d];
      }
      // the run's length: the last described keypoint's rank + 1 (s_lr is non-decreasing over the described ones)
      for (int j = HS_PACK_KP - 1; j >= 0; j--)
         if (s_lr[j] >= 0) { n_live = s_lr[j] + 1; break; }
      __syncthreads();
      const uint32_t total = (uint32_t)n_live * HS_PACK_DW;
      uint32_t *o = out32 + (size_t)base * HS_PACK_DW;
      for (uint32_t i = tid; i < total; i += 256) o[i] = s_rec[i];
      __syncthreads();
   }
}

// ---------------------------------------------------------------------------------------
// k_pack_regions: one hesaff_region record (include/hesaff_amd.h, 64 bytes) per Hessian keypoint of the batch, in list
// order = the reference's onHessianKeypointDetected order (pyramid.h:43-47), with what hesaff.cpp:66-105 made of it:
// findAffineShape's un-rectified U and iteration count (affine.h:48-58; zero when it did not converge, whatever the
// affine stage left in those slots), normalizeAffine's verdict, and the row of its keys record (rank[h] from k_pack's scan
// minus the image's first row).  Only hesaff_detect_regions launches it, straight into the chunk's staging slot.
// A lane per record: the structure-of-arrays reads are coalesced runs, and the record leaves as four 16-byte stores, so
// the four stores of a wavefront cover 4 KB back to back.
// ---------------------------------------------------------------------------------------
struct RegionTab { float pd[HS_MAX_OCTAVES]; };   // pixelDistance of every octave, the host's octave schedule (pyramid.cpp:264-288)
#define HS_REGION_DW 16   // dwords per record
__global__ __launch_bounds__(256) void k_pack_regions(HessList hl, uint32_t n, AffineOut aff, PatchWork pw, const uint32_t *__restrict__ rank,
                                                      const int32_t *__restrict__ desc_starts, RegionTab tab, uint4 *__restrict__ out)
{
   for (uint32_t h = blockIdx.x * blockDim.x + threadIdx.x; h < n; h += gridDim.x * blockDim.x) {
      const int meta = hl.meta[h];
      const int b = meta >> 8, octave = (meta >> 4) & 15, level = (meta >> 2) & 3, type = meta & 3;
      const bool converged = aff.converged[h] != 0;
      const bool described = converged && pw.alive[h] != 0;
      uint4 U = make_uint4(0u, 0u, 0u, 0u);
      uint32_t iters = 0u;
      if (converged) {
         U = *reinterpret_cast<const uint4 *>(aff.U + 4 * (size_t)h);
         iters = (uint32_t)aff.iters[h];
      }
      const uint32_t outcome = converged ? (described ? 2u : 1u) : 0u;
      const uint32_t key = described ? rank[h] - (uint32_t)desc_starts[b] : 0xffffffffu;
      uint4 *o = out + 4 * (size_t)h;
      o[0] = make_uint4(__float_as_uint(hl.x[h]), __float_as_uint(hl.y[h]), __float_as_uint(hl.s[h]), __float_as_uint(tab.pd[octave]));
      o[1] = make_uint4(__float_as_uint(hl.response[h]), (uint32_t)type, (uint32_t)octave, (uint32_t)level);
      o[2] = U;
      o[3] = make_uint4(iters, outcome, key, 0u);
   }
}

// ---------------------------------------------------------------------------------------
// k_ingest_regions: the other direction (hesaff_describe_regions).  The caller's hesaff_region records of a chunk - image
// after image, starts[b] .. starts[b + 1] those of image b - become the Hessian list the detector would have left:
// x, y, s, response and meta = image << 8 | octave << 4 | level << 2 | type.  With `shapes` (HESAFF_FROM_SHAPES) the
// affine stage's output is written as well, as if findAffineShape had converged on the caller's U (hesaff.cpp:73-105
// entered directly).  Also sets what run_detection's ordering step leaves behind: the list's length and the per-image starts.
// The host has checked every record (describe_bad_record): what arrives here is finite and in range.  Octave and level
// are not used for addressing after a HESAFF_FROM_SHAPES ingest; fields the record format cannot hold are taken as 0.
// A lane per record: four 16-byte loads cover its 64 bytes (a wavefront reads 4 KB back to back), and every store is a
// coalesced run of one structure-of-arrays column.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ingest_regions(const uint4 *__restrict__ recs, uint32_t n, const int32_t *__restrict__ starts, int nimg,
                                                        int shapes, HessList hl, AffineOut aff, uint32_t *__restrict__ n_hess,
                                                        int32_t *__restrict__ hess_starts)
{
   const uint32_t t0 = blockIdx.x * blockDim.x + threadIdx.x;
   if (t0 <= (uint32_t)nimg) hess_starts[t0] = starts[t0];
   if (t0 == 0) *n_hess = n;
   for (uint32_t h = t0; h < n; h += gridDim.x * blockDim.x) {
      const uint4 *r = recs + 4 * (size_t)h;
      const uint4 q0 = r[0], q1 = r[1];
      // the image of record h: the last b with starts[b] <= h (empty images share a start with their successor)
      int lo = 0, hi = nimg;
      while (hi - lo > 1) {
         const int mid = (lo + hi) >> 1;
         if ((uint32_t)starts[mid] <= h) lo = mid; else hi = mid;
      }
      const uint32_t octave = q1.z < (uint32_t)HS_MAX_OCTAVES ? q1.z : 0u, level = q1.w < 4u ? q1.w : 0u, type = q1.y & 3u;
      hl.x[h] = __uint_as_float(q0.x); hl.y[h] = __uint_as_float(q0.y); hl.s[h] = __uint_as_float(q0.z);
      hl.response[h] = __uint_as_float(q1.x);
      hl.meta[h] = (int32_t)(((uint32_t)lo << 8) | (octave << 4) | (level << 2) | type);
      hl.r0c0[h] = 0;
      if (shapes) {
         const uint4 q2 = r[2], q3 = r[3];
         *reinterpret_cast<uint4 *>(aff.U + 4 * (size_t)h) = q2;
         aff.converged[h] = 1;
         aff.iters[h] = (int32_t)q3.x;
      }
   }
}

// device check of hmath.h against the host (stage API)
__global__ void k_math(int n, const float *__restrict__ a, const float *__restrict__ b, float *__restrict__ at, float *__restrict__ pw)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i >= n) return;
   at[i] = hm_atan2f(a[i], b[i]);
   pw[i] = hm_pow2f(a[i]);
}

__global__ void k_rectify_stage(int n, float *A)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i >= n) return;
   hs_rectify(A[4 * i], A[4 * i + 1], A[4 * i + 2], A[4 * i + 3]);
}
