// plan_consts.h -- the constants that both the kernels and the host's batch plan (batch_plan.h) compute with.
// No HIP here: the kernel headers take them through device_common.h, the CPU check of the plan through batch_plan.h.
#pragma once

#define HS_PATCH 41                 // patchSize, affine.h:42 / siftdesc.h:30
#define HS_BORDER 5                 // PyramidParams::border, pyramid.h:39
#define HS_NSCALES 3                // numberOfScales, pyramid.h:35
#define HS_MAX_OCTAVES 16

#define BM_STRIP 248                // columns per wavefront of k_blur_hess_march (kernels_pyramid.h)
#define EXM_STRIP 248               // columns per wavefront of k_extrema_march (kernels_pyramid.h)
#define HS_CAND_BLOCK 64u           // slots a wavefront reserves at a time (one global atomic per 64 candidates)

#define HS_NBINS 5   // window size P: 0: <=41, 1: <=64 (full blur in LDS); 2: <=128 (row-streamed, LDS); 3: <=512, 4: larger (row-streamed, HBM)
#define HS_BIN3_PMAX 512
#define HS_NEED 82          // blurred columns (and rows) the 41x41 resample reads: 2 per output
#define HS_LARGE_CHUNK 18   // consecutive window rows per wavefront task of k_patch_large_rows (a multiple of three: its three-row form)
