// orient_peaks.h -- the peak rule of the orientation count (hesaff_set_orientation_count, include/hesaff_amd.h; DESIGN.md, "Secondary
// orientation peaks"): which bins of the smoothed 36-bin gradient histogram make a key, and the angle of one.  No HIP here:
// k_orientation_peaks (kernels_orient.h) and tests/native/orient_peaks_check.cpp run the same text.  All binary32, no FMA, left to right.
#pragma once

#if defined(__HIPCC__)
#define HS_OP_HD __host__ __device__ __forceinline__
#else
#define HS_OP_HD inline
#endif

#define HS_ORI_BINS 36
#define HS_ORI_MAX_COUNT 4   // the largest orientation count: keys of one region

// h[36] after the smoothing passes, K in 1..HS_ORI_MAX_COUNT -> n_ori, and bins[0 .. n_ori):
//   rank 0: m, the first index of the maximum.  h[m] == 0 (a flat histogram): that one alone.
//   candidates: every b != m with h[b] > h[b-1], h[b] > h[b+1] (circular, strict) and h[b] >= 0.8f * h[m] (one multiplication);
//   a comparison with a NaN is false.  Ordered by h[b] descending, equal heights lower bin first; rank j >= 1 is the j-th of them.
//   n_ori = min(K, 1 + candidates).
HS_OP_HD int hs_ori_peaks(const float *h, int K, int *bins)
{
   int m = 0;
   for (int b = 1; b < HS_ORI_BINS; b++)
      if (h[b] > h[m]) m = b;
   bins[0] = m;
   if (h[m] == 0.0f) return 1;
   const float least = 0.8f * h[m];
   float height[HS_ORI_MAX_COUNT];
   height[0] = h[m];
   int n = 1;
   for (int b = 0; b < HS_ORI_BINS && K > 1; b++) {
      if (b == m) continue;
      const float l = h[b == 0 ? HS_ORI_BINS - 1 : b - 1], q = h[b], r = h[b == HS_ORI_BINS - 1 ? 0 : b + 1];
      if (!(q > l && q > r && q >= least)) continue;
      // behind every kept candidate that is at least as high (b ascends: of equal heights the lower bin stays in front)
      int pos = n;
      while (pos > 1 && q > height[pos - 1]) pos--;
      if (pos >= K) continue;
      for (int i = (n < K ? n : K - 1); i > pos; i--) { bins[i] = bins[i - 1]; height[i] = height[i - 1]; }
      bins[pos] = b; height[pos] = q;
      if (n < K) n++;
   }
   return n;
}

// step 5's angle around bin b: the parabola through (l, q, r), its `den == 0 -> off = 0` clause included
HS_OP_HD float hs_ori_theta(const float *h, int b)
{
   const float PI = (float)3.14159265358979323846;   // 0x40490fdb
   const float bin_width = (2.0f * PI) / 36.0f;
   const float l = h[b == 0 ? HS_ORI_BINS - 1 : b - 1], q = h[b], r = h[b == HS_ORI_BINS - 1 ? 0 : b + 1];
   const float den = (l + r) - (q + q);
   const float off = den == 0.0f ? 0.0f : (0.5f * (l - r)) / den;
   return (((float)b + 0.5f) + off) * bin_width - PI;
}
