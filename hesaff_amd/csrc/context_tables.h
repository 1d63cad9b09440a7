// context_tables.h -- the host arithmetic of context setup: every table a context uploads once (masks, SIFT bins, k_sift_grad's per-pixel
// constants, the gradient-pair layout, the pyramid taps), the per-keypoint patch taps a plan grows, the octave schedule and DConsts.
// Each entry is an index, an offset or a weight that a kernel follows without a bounds check.  Pure functions and plain structs, no HIP:
// pipeline.hip uploads what they return (DeviceTables), and tests/native/tables_check.cpp checks them on the CPU
// (tests/test_context_tables.py) before they meet a GPU.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "chunk_engine.h"   // HsError (and, through it, hesaff_params of include/hesaff_amd.h)
#include "hmath.h"
#include "host_tables.h"
#include "plan_consts.h"

namespace hesaff {

inline OctaveSchedule make_schedule(float initialSigma, bool upscale)
{
   OctaveSchedule s;
   // pyramid.cpp:227 : powf(2, 1/numberOfScales) ; hm_pow2f == glibc powf(2,.) bit for bit
   const float sigmaStep = hm_pow2f(1.0f / (float)HS_NSCALES);
   float curSigma = initialSigma;
   // pyramid.cpp:263-280: the input is taken to be blurred by 0.5 already (1.0 after the 2x up-sampling);
   // no initial blur when initialSigma does not exceed that
   const float inputSigma = upscale ? 0.5f * 2.0f : 0.5f;
   s.init_sigma = initialSigma > inputSigma ? sqrtf(initialSigma * initialSigma - inputSigma * inputSigma) : 0.0f;
   s.level_sigma[0] = curSigma;
   s.blur_sigma[0] = 0.0f;
   {
      const float n = curSigma * curSigma;
      s.norm2[0] = n * n;
   }
   for (int i = 1; i < HS_NSCALES + 2; i++) {
      s.blur_sigma[i] = curSigma * sqrtf(sigmaStep * sigmaStep - 1.0f);
      const float sigma = curSigma * sigmaStep;
      s.level_sigma[i] = sigma;
      const float n = sigma * sigma;
      s.norm2[i] = n * n;
      curSigma *= sigmaStep;
   }
   return s;
}

// the K taps of a blur whose size gauss_ksize chose: a single tap is the identity (helpers.cpp:286-295 hands cv::GaussianBlur a 1 x 1 kernel)
inline void blur_taps(int K, float sigma, float *cf)
{
   if (K == 1) cf[0] = 1.0f;
   else gauss_taps(K, sigma, cf);
}

} // namespace hesaff

namespace hesaff_plan {

using hesaff_engine::HsError;

// What a context keeps of its tables on the host once they are uploaded ...
struct ContextScalars {
   int pyr_K[5];             // [0] initial blur (0 = none), [1..4] octave blurs
   int pyr_tap_off[5];       // each level owns 256 floats of pyr_taps from here
   bool pyr_march = false;   // the four octave blurs have K = 9, 11, 13, 15 (default initialSigma): marching kernel
   int n_masked = 0;         // pixels inside the circular mask
   int up = 0;               // upscaleInputImage, pyramid.h:34
   hesaff::OctaveSchedule sched;
   DConsts consts;
};
// ... and the tables themselves, in the layouts of KpTables (kernels_keypoint.h)
struct ContextTables : ContextScalars {
   std::vector<float> smm, sift_mask, w0, w1;   // 19 x 19 and 41 x 41 masks, SIFT bin weights
   std::vector<int32_t> bin0, bin1;
   std::vector<int32_t> mask_idx;               // raster-ordered indices of the pixels with sift_mask > 0
   std::vector<int32_t> sgrad_nb, sgrad_om;     // int4 / int2 per slot, 1280 slots
   std::vector<int32_t> vo_rows;                // int4 per row, HS_VO_DIM rows
   std::vector<uint16_t> vo_src;                // HS_VO_ITEMS
   std::vector<float> pyr_taps;
};

inline ContextTables build_context_tables(const hesaff_params &p)
{
   ContextTables t;
   t.smm.resize(HS_SMM_PIX); t.sift_mask.resize(HS_PATCH_PIX); t.w0.resize(HS_PATCH); t.w1.resize(HS_PATCH);
   t.bin0.resize(HS_PATCH); t.bin1.resize(HS_PATCH);
   const std::vector<float> &sm = t.sift_mask;
   hesaff::gauss_mask(HS_SMM, t.smm.data());
   hesaff::circ_gauss_mask(HS_PATCH, t.sift_mask.data());
   hesaff::sift_bins(t.bin0.data(), t.bin1.data(), t.w0.data(), t.w1.data());
   {
      std::vector<int32_t> &midx = t.mask_idx;
      for (int i = 0; i < HS_PATCH_PIX; i++)
         if (sm[i] > 0) midx.push_back(i);
      t.n_masked = (int)midx.size();
      // k_sift_grad's per-pixel constants (affine.cpp:14-33 stencil convention: one-sided differences at the patch border)
      std::vector<int32_t> &nb = t.sgrad_nb, &om = t.sgrad_om;
      nb.assign(4 * 1280, 0); om.assign(2 * 1280, 0);
      for (size_t s = 0; s < 1280; s++) {
         const bool used = s < midx.size();
         const int i = used ? midx[s] : 0, r = i / HS_PATCH, cc = i - r * HS_PATCH;
         const bool valid = used && r < HS_PATCH - 1 && cc < HS_PATCH - 1;   // row / column 40 carry no weight in samplePatch
         if (valid) {
            nb[4 * s + 0] = 4 * (cc == 0 ? i : i - 1);
            nb[4 * s + 1] = 4 * (i + 1);
            nb[4 * s + 2] = 4 * (r == 0 ? i : i - HS_PATCH);
            nb[4 * s + 3] = 4 * (i + HS_PATCH);
         }
         om[2 * s + 0] = valid ? r * (HS_PATCH - 1) + cc : -1;
         memcpy(&om[2 * s + 1], &sm[i], 4);
      }
      // layout of the gradient pairs in HBM (plan_consts.h: HS_VO_ITEMS), from the mask itself: per row the span of 16-byte items
      // (two pixels) that hold a pixel with weight, rows back to back
      std::vector<int32_t> &vrow = t.vo_rows;
      std::vector<uint16_t> &vsrc = t.vo_src;
      vrow.assign(4 * HS_VO_DIM, 0); vsrc.assign(HS_VO_ITEMS, 0);
      int at = 0;
      for (int r = 0; r < HS_VO_DIM; r++) {
         int flo = 1, fhi = 0;
         for (int cc = 0; cc < HS_VO_DIM; cc++)
            if (sm[r * HS_PATCH + cc] > 0) { if (fhi < flo) flo = cc / 2; fhi = cc / 2; }
         vrow[4 * r + 0] = at - flo; vrow[4 * r + 1] = flo; vrow[4 * r + 2] = fhi;
         for (int f = flo; f <= fhi; f++, at++)
            if (at < HS_VO_ITEMS) vsrc[(size_t)at] = (uint16_t)(r * (HS_VO_DIM / 2) + f);
      }
      // the layout constants of plan_consts.h are those of THIS mask (helpers.cpp:131-147 at patchSize 41)
      if (at != HS_VO_ZERO || sm[0] > 0) throw HsError(HESAFF_ERR_ARG, "internal: gradient-pair layout does not match the circular mask");
   }
   t.up = p.upscaleInputImage > 0 ? 1 : 0;
   t.sched = hesaff::make_schedule(p.initialSigma, t.up != 0);
   std::vector<float> &taps = t.pyr_taps;
   for (int i = 0; i < 5; i++) {
      const float sigma = i == 0 ? t.sched.init_sigma : t.sched.blur_sigma[i];
      t.pyr_tap_off[i] = (int)taps.size();
      taps.resize(taps.size() + 256, 0.0f);
      if (i == 0 && !(t.sched.init_sigma > 0.0f)) { t.pyr_K[0] = 0; continue; }   // pyramid.cpp:276: no initial blur
      const int K = hesaff::gauss_ksize(sigma);
      if (K > 255) throw HsError(HESAFF_ERR_ARG, "initialSigma too large (a pyramid blur would need more than 255 taps)");
      t.pyr_K[i] = K;
      hesaff::blur_taps(K, sigma, taps.data() + t.pyr_tap_off[i]);
   }
   t.pyr_march = t.pyr_K[1] == 9 && t.pyr_K[2] == 11 && t.pyr_K[3] == 13 && t.pyr_K[4] == 15;
   DConsts &k = t.consts;
   // pyramid.h:59-64
   k.edgeScoreThreshold = (p.edgeEigenValueRatio + 1.0f) * (p.edgeEigenValueRatio + 1.0f) / p.edgeEigenValueRatio;
   k.finalThreshold = p.threshold * p.threshold;
   k.positiveThreshold = (float)(0.8 * k.finalThreshold);
   k.negativeThreshold = -k.positiveThreshold;
   k.convergenceThreshold = p.convergenceThreshold;
   k.affInitialSigma = 1.6f;   // AffineShapeParams::initialSigma affine.h:40 (not overridden by hesaff.cpp)
   k.mrSize = p.mrSize;
   k.maxBinValue = p.maxBinValue;
   k.maxIterations = p.maxIterations;
   k.pd0 = t.up ? 0.5f : 1.0f;   // pixelDistance of octave 0, pyramid.cpp:264,270
   return t;
}

// taps of the per-keypoint patch blur (affine.cpp:129: sigma = 1.5f * P0/41) for every odd P0 <= max_p0 (an even request is rounded up):
// P0's K = k[(P0 - 1) / 2] taps start at taps[off[(P0 - 1) / 2]]
struct PatchTaps {
   std::vector<float> taps;
   std::vector<int32_t> off, k;
   int max_p0;
};
inline PatchTaps build_patch_taps(int max_p0)
{
   if ((max_p0 & 1) == 0) max_p0++;
   PatchTaps t;
   t.max_p0 = max_p0;
   t.off.resize((max_p0 + 1) / 2); t.k.resize((max_p0 + 1) / 2);
   for (int P0 = 1; P0 <= max_p0; P0 += 2) {
      const float scale = (float)P0 / (float)HS_PATCH;
      const float sigma = 1.5f * scale;
      const int K = hesaff::gauss_ksize(sigma);
      t.off[(P0 - 1) / 2] = (int32_t)t.taps.size();
      t.k[(P0 - 1) / 2] = K;
      t.taps.resize(t.taps.size() + K);
      hesaff::blur_taps(K, sigma, t.taps.data() + t.off[(P0 - 1) / 2]);
   }
   return t;
}

} // namespace hesaff_plan
