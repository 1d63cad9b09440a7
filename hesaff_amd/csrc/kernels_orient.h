// kernels_orient.h -- the dominant-orientation mode (hesaff_set_orientation, include/hesaff_amd.h; no counterpart in the
// reference, which describes every region in the "up is up" frame of rectifyAffineTransformationUpIsUp, hesaff.cpp:79).
// Between two runs of normalizeAffine the frame is turned by the dominant gradient angle of the first run's patch:
//   k_orientation            theta from the 41 x 41 patch of the up-is-up matrix A, then A' = A * R(theta) in place
//   k_prepare_patch_second   the border tests and the window-size bins again, for A', over the keypoints pass one left alive
// The definition ("Dominant orientation"), all binary32, no FMA, evaluated left to right:
//   r, c in 1..39:  gx = p[r][c+1] - p[r][c-1],  gy = p[r+1][c] - p[r-1][c],  w = M[r][c] * sqrtf(gx*gx + gy*gy)
//                   t = (atan2f(gy, gx) + PI) * (36 / (2 PI)),  b = (int)t, 36 -> 0         M: computeCircularGaussMask(41)
//   row[r][b] += w over c ascending;  h[b] = sum of row[r][b] over r ascending;  six circular passes of ((h[b-1] + h[b]) + h[b+1]) / 3
//   m = first index of the maximum;  h[m] == 0: theta = 0 and A stays, bit for bit
//   else off = (0.5 (l - r)) / ((l + r) - (q + q)) (0 when the denominator is 0),  theta = ((m + 0.5) + off) * (2 PI / 36) - PI
// The two-level order of the sums is what lets a lane own a patch row and, later, a histogram bin: no atomics, no cross-lane
// reduction, and the same bits on every run.
//
// With an orientation count K > 1 (hesaff_set_orientation_count) k_orientation_peaks takes k_orientation's place: the same histogram,
// then the peak rule of orient_peaks.h, and up to K frames A'_j = A * R(theta_j), each from the same up-is-up A.  Rank 0 lands where
// k_orientation puts its one frame; rank j >= 1 in the rank arrays (OrientRanks), with the flag "this keypoint has a rank j" that
// k_prepare_patch_second over those arrays then turns into "normalizeAffine accepted rank j".
#pragma once
#include "kernels_sift.h"
#include "orient_peaks.h"

#define HS_ORI_PITCH 37   // floats between two rows' histograms in LDS: odd, so the 36 column sums read conflict-free
#define HS_ORI_ROWS (HS_PATCH - 2)

struct OrientIO {
   const float *patches;    // [n][1681] (index = h - h_lo): pass one's patches, before photometric normalisation
   uint32_t h_lo, h_hi;     // keypoints [h_lo, h_hi) of the list ...
   const uint32_t *n_ptr;   // ... clipped to the list's length on the device and to its capacity, as k_prepare_patch clips (null: h_hi stands)
   uint32_t cap;
   const int32_t *alive;    // [n] by h (null: every keypoint): a keypoint pass one rejected has no patch
   float *A;                // [n][4] by h, rewritten in place (null: not written)
   float *theta, *hist, *cs;   // the stage entry point's outputs by h - h_lo (each may be null): theta, hist[36] after smoothing, (cos, sin)
};

// (OrientRanks, what the ranks j >= 1 of an orientation count K own: device_lists.h)

// One wavefront per keypoint, blocks persistent over the list.  The patch comes into LDS as coalesced runs; lanes 0..38 each
// march one row (41 floats apart: an odd stride over the banks) and add into their own 36 bins; lanes 0..35 add the 39 rows of one
// bin and smooth through two LDS copies of h; lane 0 finds the peak and turns the frame.  19536 B (19.1 KiB) of LDS per block, the mask
// (read once per block) included: 8 blocks per CU.
__global__ __launch_bounds__(64) void k_orientation(OrientIO io, KpTables tb)
{
   __shared__ float s_p[HS_PATCH_PIX];
   __shared__ float s_m[HS_PATCH_PIX];
   __shared__ float s_row[HS_ORI_ROWS * HS_ORI_PITCH];
   __shared__ float s_h[2][HS_ORI_BINS];
   const int lane = threadIdx.x;
   const float PI = hm_u2f(0x40490fdbu);   // (float)M_PI
   const float to_bin = 36.0f / (2.0f * PI), bin_width = (2.0f * PI) / 36.0f;
   const uint32_t n = io.n_ptr ? min(min(*io.n_ptr, io.cap), io.h_hi) : io.h_hi;
   for (int i = lane; i < HS_PATCH_PIX; i += 64) s_m[i] = tb.sift_mask[i];
   for (uint32_t h = io.h_lo + blockIdx.x; h < n; h += gridDim.x) {
      if (io.alive && !io.alive[h]) continue;   // (the same for every lane)
      const size_t k = (size_t)(h - io.h_lo);
      __syncthreads();   // the keypoint before has been read out of s_p and s_h
      const float *pp = io.patches + k * HS_PATCH_PIX;
      for (int i = lane; i < HS_PATCH_PIX; i += 64) s_p[i] = pp[i];
      __syncthreads();
      if (lane < HS_ORI_ROWS) {
         float *row = s_row + lane * HS_ORI_PITCH;
         for (int b = 0; b < HS_ORI_BINS; b++) row[b] = 0.0f;
         const float *q = s_p + (lane + 1) * HS_PATCH, *mk = s_m + (lane + 1) * HS_PATCH;
         for (int c = 1; c <= HS_ORI_ROWS; c++) {
            const float gx = q[c + 1] - q[c - 1], gy = q[c + HS_PATCH] - q[c - HS_PATCH];
            const float w = mk[c] * sqrtf(gx * gx + gy * gy);
            const float t = (hm_atan2f_sel(gy, gx) + PI) * to_bin;
            int b = (int)t;
            if (b >= HS_ORI_BINS) b -= HS_ORI_BINS;
            b = min(max(b, 0), HS_ORI_BINS - 1);   // (only a non-finite patch value gets here out of range)
            row[b] += w;
         }
      }
      __syncthreads();
      if (lane < HS_ORI_BINS) {
         float acc = 0.0f;
         for (int r = 0; r < HS_ORI_ROWS; r++) acc = acc + s_row[r * HS_ORI_PITCH + lane];
         s_h[0][lane] = acc;
      }
      for (int it = 0; it < 6; it++) {
         __syncthreads();
         if (lane < HS_ORI_BINS) {
            const float *hp = s_h[it & 1];
            const float l = hp[lane == 0 ? HS_ORI_BINS - 1 : lane - 1], r = hp[lane == HS_ORI_BINS - 1 ? 0 : lane + 1];
            s_h[(it + 1) & 1][lane] = ((l + hp[lane]) + r) / 3.0f;
         }
      }
      __syncthreads();
      const float *hs = s_h[0];   // six passes: back in the first copy
      if (io.hist && lane < HS_ORI_BINS) io.hist[k * HS_ORI_BINS + lane] = hs[lane];
      if (lane == 0) {
         int m = 0;
         for (int b = 1; b < HS_ORI_BINS; b++)
            if (hs[b] > hs[m]) m = b;
         float theta = 0.0f;
         const bool flat = hs[m] == 0.0f;
         if (!flat) {
            const float l = hs[m == 0 ? HS_ORI_BINS - 1 : m - 1], q = hs[m], r = hs[m == HS_ORI_BINS - 1 ? 0 : m + 1];
            const float den = (l + r) - (q + q);
            const float off = den == 0.0f ? 0.0f : (0.5f * (l - r)) / den;
            theta = (((float)m + 0.5f) + off) * bin_width - PI;
         }
         float sn, cs;
         hm_sincosf(theta, &sn, &cs);
         if (io.theta) io.theta[k] = theta;
         if (io.cs) { io.cs[2 * k] = cs; io.cs[2 * k + 1] = sn; }
         if (io.A && !flat) {
            float4 *Ap = reinterpret_cast<float4 *>(io.A + 4 * (size_t)h);
            const float4 a = *Ap;   // a11, a12, a21, a22
            float4 o;
            o.x = a.x * cs + a.y * sn;
            o.y = a.y * cs - a.x * sn;
            o.z = a.z * cs + a.w * sn;
            o.w = a.w * cs - a.z * sn;
            *Ap = o;
         }
      }
   }
}

// The multi form (orientation count mr.K > 1): k_orientation's steps 1-4 word for word - the same LDS, the same occupancy - then the peak
// rule of orient_peaks.h on lane 0, whose extra work lives in registers.  (A body shared with k_orientation through a template compiled
// k_orientation to another register allocation; K = 1 must launch the kernel as it stands, so the text is repeated.)
__global__ __launch_bounds__(64) void k_orientation_peaks(OrientIO io, KpTables tb, OrientRanks mr)
{
   __shared__ float s_p[HS_PATCH_PIX];
   __shared__ float s_m[HS_PATCH_PIX];
   __shared__ float s_row[HS_ORI_ROWS * HS_ORI_PITCH];
   __shared__ float s_h[2][HS_ORI_BINS];
   const int lane = threadIdx.x;
   const float PI = hm_u2f(0x40490fdbu);   // (float)M_PI
   const float to_bin = 36.0f / (2.0f * PI);
   const uint32_t n = io.n_ptr ? min(min(*io.n_ptr, io.cap), io.h_hi) : io.h_hi;
   for (int i = lane; i < HS_PATCH_PIX; i += 64) s_m[i] = tb.sift_mask[i];
   for (uint32_t h = io.h_lo + blockIdx.x; h < n; h += gridDim.x) {
      if (io.alive && !io.alive[h]) {           // (the same for every lane)
         if (lane > 0 && lane < mr.K && mr.alive) mr.alive_of(lane)[h] = 0;   // pass one rejected it: no rank has a key
         continue;
      }
      const size_t k = (size_t)(h - io.h_lo);
      __syncthreads();   // the keypoint before has been read out of s_p and s_h
      const float *pp = io.patches + k * HS_PATCH_PIX;
      for (int i = lane; i < HS_PATCH_PIX; i += 64) s_p[i] = pp[i];
      __syncthreads();
      if (lane < HS_ORI_ROWS) {
         float *row = s_row + lane * HS_ORI_PITCH;
         for (int b = 0; b < HS_ORI_BINS; b++) row[b] = 0.0f;
         const float *q = s_p + (lane + 1) * HS_PATCH, *mk = s_m + (lane + 1) * HS_PATCH;
         for (int c = 1; c <= HS_ORI_ROWS; c++) {
            const float gx = q[c + 1] - q[c - 1], gy = q[c + HS_PATCH] - q[c - HS_PATCH];
            const float w = mk[c] * sqrtf(gx * gx + gy * gy);
            const float t = (hm_atan2f_sel(gy, gx) + PI) * to_bin;
            int b = (int)t;
            if (b >= HS_ORI_BINS) b -= HS_ORI_BINS;
            b = min(max(b, 0), HS_ORI_BINS - 1);   // (only a non-finite patch value gets here out of range)
            row[b] += w;
         }
      }
      __syncthreads();
      if (lane < HS_ORI_BINS) {
         float acc = 0.0f;
         for (int r = 0; r < HS_ORI_ROWS; r++) acc = acc + s_row[r * HS_ORI_PITCH + lane];
         s_h[0][lane] = acc;
      }
      for (int it = 0; it < 6; it++) {
         __syncthreads();
         if (lane < HS_ORI_BINS) {
            const float *hp = s_h[it & 1];
            const float l = hp[lane == 0 ? HS_ORI_BINS - 1 : lane - 1], r = hp[lane == HS_ORI_BINS - 1 ? 0 : lane + 1];
            s_h[(it + 1) & 1][lane] = ((l + hp[lane]) + r) / 3.0f;
         }
      }
      __syncthreads();
      const float *hs = s_h[0];   // six passes: back in the first copy
      if (io.hist && lane < HS_ORI_BINS) io.hist[k * HS_ORI_BINS + lane] = hs[lane];
      if (lane == 0) {
         int bins[HS_ORI_MAX_COUNT];
         const int n_ori = hs_ori_peaks(hs, mr.K, bins);
         const bool flat = hs[bins[0]] == 0.0f;
         float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
         if (io.A) a = *reinterpret_cast<const float4 *>(io.A + 4 * (size_t)h);   // a11, a12, a21, a22: the up-is-up frame every rank turns
         if (mr.n_ori) mr.n_ori[k] = n_ori;
         for (int j = 0; j < mr.K; j++) {
            const bool has = j < n_ori;
            const float theta = (has && !flat) ? hs_ori_theta(hs, bins[j]) : 0.0f;
            if (mr.bins) mr.bins[k * HS_ORI_MAX_COUNT + j] = has ? bins[j] : -1;
            if (mr.thetas) mr.thetas[k * HS_ORI_MAX_COUNT + j] = theta;
            if (j > 0 && mr.alive) mr.alive_of(j)[h] = has ? 1 : 0;
            if (!has || !io.A || (j == 0 && flat)) continue;   // a flat histogram has rank 0 alone, and its frame stays bit for bit
            float sn, cs;
            hm_sincosf(theta, &sn, &cs);
            float4 o;
            o.x = a.x * cs + a.y * sn;
            o.y = a.y * cs - a.x * sn;
            o.z = a.z * cs + a.w * sn;
            o.w = a.w * cs - a.z * sn;
            *reinterpret_cast<float4 *>((j == 0 ? io.A : mr.A_of(j)) + 4 * (size_t)h) = o;
         }
      }
   }
}

// normalizeAffine's border tests and the bins for the turned frames: hs_prepare_patch_body over pw.A as it stands, and only over the
// keypoints pass one left alive - a keypoint it rejected stays rejected, whatever its entry of pw.A holds.  The caller has cleared
// the bin counters.
__global__ __launch_bounds__(256) void k_prepare_patch_second(HessList hl, uint32_t h_lo, uint32_t h_hi, const uint32_t *__restrict__ n_ptr, int imRows,
                                                              int imCols, DConsts k, KpTables tb, PatchWork pw)
{
   AffineOut none;
   none.converged = nullptr; none.U = nullptr; none.iters = nullptr;
   hs_prepare_patch_body<false, true>(hl, h_lo, min(min(*n_ptr, hl.cap), h_hi), none, imRows, imCols, k, tb, pw);
}

// ---- the pack stage of an orientation count K > 1: a region owns as many adjacent rows as it has keys, in ascending rank ----

// keys of keypoint i: the scan's load (exclusive_scan).  p: rank 0's flags (and the pointer k_scan_down tests for alignment).
struct LoadKeyCount {
   const int32_t *p;
   const int32_t *ranks;   // OrientRanks::alive
   uint32_t cap;
   int K;
   __device__ uint32_t operator()(long long i) const
   {
      uint32_t n = p[i] != 0 ? 1u : 0u;
      for (int j = 1; j < K; j++) n += ranks[(size_t)(j - 1) * cap + (size_t)i] != 0 ? 1u : 0u;
      return n;
   }
   __device__ void load16(long long base, uint32_t *v) const
   {
#pragma unroll
      for (int i = 0; i < 16; i++) v[i] = (*this)(base + i);
   }
};

// k_pack for K > 1: a wavefront per Hessian keypoint, lane d the d-th dword of a record, a record per rank that has a key, from row
// rank[h] (the exclusive scan of the key counts) on.  Rows at and beyond out_cap - the records b_out is sized for - are not written:
// the host sees the total and refuses the batch (HESAFF_ERR_CAPACITY).
__global__ __launch_bounds__(256) void k_pack_peaks(HessList hl, const uint32_t *__restrict__ n_ptr, PatchWork pw, OrientRanks mr,
                                                    const uint32_t *__restrict__ rank, const uint8_t *__restrict__ desc, KeyRec *__restrict__ out, uint32_t out_cap)
{
   const uint32_t n = min(*n_ptr, hl.cap);
   const int lane = threadIdx.x & 63;
   const uint32_t waves = gridDim.x * (blockDim.x >> 6);
   uint32_t *out32 = reinterpret_cast<uint32_t *>(out);
   for (uint32_t h = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); h < n; h += waves) {
      uint32_t row = rank[h];
      for (int j = 0; j < mr.K; j++) {
         const int32_t *alive = j == 0 ? pw.alive : mr.alive_of(j);
         if (!alive[h]) continue;   // (the same for every lane)
         if (row < out_cap && lane < HS_PACK_DW) {
            const float *A = j == 0 ? pw.A : mr.A_of(j);
            const uint32_t *d32 = reinterpret_cast<const uint32_t *>(j == 0 ? desc : mr.desc_of(j));
            uint32_t v;
            if (lane == 0) v = __float_as_uint(hl.x[h]);
            else if (lane == 1) v = __float_as_uint(hl.y[h]);
            else if (lane == 2) v = __float_as_uint(hl.s[h]);
            else if (lane < 7) v = __float_as_uint(A[4 * (size_t)h + (lane - 3)]);
            else if (lane == 7) v = __float_as_uint(hl.response[h]);
            else if (lane == 8) v = (uint32_t)(hl.meta[h] & 3);
            else v = d32[(size_t)h * 32 + (lane - 9)];
            out32[(size_t)row * HS_PACK_DW + lane] = v;
         }
         row++;
      }
   }
}

// k_pack_regions for K > 1: outcome 2 iff the region has a key, `key` the row of its first one, `reserved` their number (-1 and 0 without)
__global__ __launch_bounds__(256) void k_pack_regions_peaks(HessList hl, uint32_t n, AffineOut aff, PatchWork pw, OrientRanks mr, const uint32_t *__restrict__ rank,
                                                            const int32_t *__restrict__ desc_starts, RegionTab tab, uint4 *__restrict__ out)
{
   for (uint32_t h = blockIdx.x * blockDim.x + threadIdx.x; h < n; h += gridDim.x * blockDim.x) {
      const int meta = hl.meta[h];
      const int b = meta >> 8, octave = (meta >> 4) & 15, level = (meta >> 2) & 3, type = meta & 3;
      const bool converged = aff.converged[h] != 0;
      uint32_t n_keys = 0;
      if (converged) {
         n_keys = pw.alive[h] != 0 ? 1u : 0u;
         for (int j = 1; j < mr.K; j++) n_keys += mr.alive_of(j)[h] != 0 ? 1u : 0u;
      }
      uint4 U = make_uint4(0u, 0u, 0u, 0u);
      uint32_t iters = 0u;
      if (converged) {
         U = *reinterpret_cast<const uint4 *>(aff.U + 4 * (size_t)h);
         iters = (uint32_t)aff.iters[h];
      }
      const uint32_t outcome = converged ? (n_keys ? 2u : 1u) : 0u;
      const uint32_t key = n_keys ? rank[h] - (uint32_t)desc_starts[b] : 0xffffffffu;
      uint4 *o = out + 4 * (size_t)h;
      o[0] = make_uint4(__float_as_uint(hl.x[h]), __float_as_uint(hl.y[h]), __float_as_uint(hl.s[h]), __float_as_uint(tab.pd[octave]));
      o[1] = make_uint4(__float_as_uint(hl.response[h]), (uint32_t)type, (uint32_t)octave, (uint32_t)level);
      o[2] = U;
      o[3] = make_uint4(iters, outcome, key, n_keys);
   }
}
