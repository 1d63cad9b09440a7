// plan_consts.h -- the constants that both the kernels and the host's plans (batch_plan.h, context_tables.h) compute with.
// No HIP here: the kernel headers take them through device_common.h, the CPU checks of the plans through batch_plan.h and context_tables.h.
#pragma once

#define HS_PATCH 41                 // patchSize, affine.h:42 / siftdesc.h:30
#define HS_BORDER 5                 // PyramidParams::border, pyramid.h:39
#define HS_NSCALES 3                // numberOfScales, pyramid.h:35
#define HS_MAX_OCTAVES 16
#define HS_PATCH_PIX (41 * 41)
#define HS_SMM 19                   // smmWindowSize, affine.h:43
#define HS_SMM_PIX (19 * 19)

#define BM_STRIP 248                // columns per wavefront of k_blur_hess_march (kernels_pyramid.h)
#define EXM_STRIP 248               // columns per wavefront of k_extrema_march (kernels_pyramid.h)
#define HS_CAND_BLOCK 64u           // slots a wavefront reserves at a time (one global atomic per 64 candidates)

#define HS_NBINS 5   // window size P: 0: <=41, 1: <=64 (full blur in LDS); 2: <=128 (row-streamed, LDS); 3: <=512, 4: larger (row-streamed, HBM)
#define HS_BIN3_PMAX 512
#define HS_NEED 82          // blurred columns (and rows) the 41x41 resample reads: 2 per output
#define HS_NSIDE 4          // side streams of the patch stage (one per window-size bin 0..3)
#define HS_NSLOT 3          // patch buffer slots of the group pipeline (group_schedule.h)
#define HS_LARGE_CHUNK 18   // consecutive window rows per wavefront task of k_patch_large_rows (a multiple of three: its three-row form)

// The gradient pairs of a keypoint in HBM (written once by k_sift_grad, read by k_sift_hist: the largest stream of the descriptor stage, and
// what both kernels are bound by - profiles/r05_notes.md).  Compact layout: only the 16-byte items (2 pixels) of every row's span inside the
// circular mask are stored, row after row (row r: items f_lo(r) .. f_hi(r) of its 20) - 642 items + 6 zero items instead of 800: 10.4 KB
// instead of 12.8 KB per keypoint.  KpTables::vo_rows / vo_src (built from the mask itself: context_tables.h) describe the layout to both kernels.
#define HS_VO_DIM 40                          // rows/columns of the patch that carry weight in samplePatch
#define HS_VO_ITEMS 648   // 16-byte items per keypoint; the items from HS_VO_ZERO on are zero
#define HS_VO_ZERO 642    // an item that is (0, 0, 0, 0) in every keypoint's block
#define HS_VO_PITCH (2 * HS_VO_ITEMS)             // float2 per keypoint in the gradient-pair buffer

// constants of one context (context_tables.h), handed to the kernels by value
struct DConsts {
   float edgeScoreThreshold, finalThreshold, positiveThreshold, negativeThreshold;  // pyramid.h:60-64
   float convergenceThreshold;  // affine.h:41
   float affInitialSigma;       // affine.h:40
   float mrSize;                // affine.h:44
   float maxBinValue;           // siftdesc.h:29
   int maxIterations;           // affine.h:39
   float pd0;                   // pixelDistance of octave 0: 1, or 0.5 with upscaleInputImage (pyramid.cpp:264,270)
};
