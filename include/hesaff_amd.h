/* hesaff_amd.h -- C ABI of libhesaff_amd.so: MI355X (gfx950) Hessian-Affine + SIFT hot path.
 *
 * Drop-in boundary for perdoch/hesaff's detect+describe path.  Plain pointers and sizes
 * only; no C++/torch types.  Every entry point cites the reference interface it replaces
 * (file:line under the reference tree).  Return value: 0 = HESAFF_OK, negative = error;
 * hesaff_last_error() gives the message.  One context per device; a context is not
 * thread-safe, distinct contexts may be used concurrently.
 *
 * The library has NO CPU fallback: every function that computes needs a visible gfx950
 * device and fails with HESAFF_ERR_DEVICE otherwise.
 */
#ifndef HESAFF_AMD_H
#define HESAFF_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HESAFF_OK 0
#define HESAFF_ERR_DEVICE (-1)    /* no usable GPU / HIP runtime error            */
#define HESAFF_ERR_ARG (-2)       /* bad argument                                 */
#define HESAFF_ERR_CAPACITY (-3)  /* keypoint capacity exceeded (raise max_kpts_per_mpx) */
#define HESAFF_ERR_IO (-4)        /* file I/O                                     */
#define HESAFF_ERR_NOMEM (-5)

/* Layout version of the structs below (hesaff_params, hesaff_timings, hesaff_result, hesaff_file_status, hesaff_region).  Neither struct
 * carries a size field, so a caller built against another header would pass shifted fields without any error: callers
 * compare hesaff_abi_version() (and, if they wish, the sizeof functions) with the header they were compiled against
 * before the first hesaff_create - hesaff.hpp and the Python binding do.  New fields are appended at the END of a
 * struct and bump this number.   1: round 1;  2: + upscaleInputImage, fast, pack_ms (inserted mid-struct);  3: + extrema_*;
 * 4: hesaff_params.fast = 1 withdrawn, HESAFF_FILE_REJECTED, rows formatted on the device;
 * 5: + hesaff_jpeg_layout, hesaff_read_jpeg_coefficients, hesaff_stage_jpeg_pixels (JPEG pixels made on the device);
 * 6: + hesaff_host_plan_for, allocator-owned read buffers (hesaff_read_*_alloc);
 * 7: + hesaff_set_pinned_read_budget, hesaff_set_pool_priority, hesaff_stage_threads_for_pool, HESAFF_OUT_STRICT; hesaff_set_resume
 *    takes 0 / 1 / 2; no struct changed;
 * 8: this header (+ hesaff_region, hesaff_region_result, hesaff_detect_regions, hesaff_sizeof_region; no existing struct changed).
 *    Version 8 also carries the float-input entry points (hesaff_detect_batch_f32, hesaff_detect_batch_cb_f32, hesaff_detect_regions_f32,
 *    hesaff_detect_batch_device_f32, hesaff_stage_pyramid_f32): they add no struct and change none, so the version stays; a caller that
 *    needs them finds them by symbol (dlsym) in the library it loaded.  The same holds for hesaff_describe_regions and
 *    hesaff_describe_regions_f32 (HESAFF_FROM_POINTS / HESAFF_FROM_SHAPES): new symbols over the structs of version 8.  And for
 *    hesaff_set_keypoint_limit / hesaff_get_keypoint_limit: two more symbols, no struct touched, the version stays 8.
 *    hesaff_set_keypoint_grid / hesaff_get_keypoint_grid: two more symbols, no struct touched, the version stays 8.
 *    Likewise hesaff_set_next_masks / hesaff_set_next_masks_device (per-image detection masks): symbols only, version 8.
 *    And for the test hook hesaff_stage_sift_alive.
 *    And for hesaff_set_orientation / hesaff_get_orientation / hesaff_stage_orientation (dominant-orientation mode): symbols only, version 8.
 *    And for the stage entry point hesaff_stage_detect_planes.
 *    And for hesaff_set_descriptor / hesaff_get_descriptor / hesaff_stage_sift_mode (RootSIFT descriptor mode): symbols only, version 8.
 *    And for hesaff_set_orientation_count / hesaff_get_orientation_count / hesaff_stage_orientation_peaks (secondary orientation peaks):
 *    symbols only, version 8.  With a count above 1, hesaff_region.reserved carries the number of a region's keys.
 *    And for visual-word assignment (hesaff_set_vocabulary and the ten symbols declared with it, HESAFF_OUT_WORDS): symbols only, version 8.
 *    And for vocabulary training (hesaff_train_vocabulary, hesaff_train_vocabulary_device, hesaff_stage_accumulate_words,
 *    hesaff_get_training_ms): symbols only, version 8.
 *    And for the image index (hesaff_index_build and the nine symbols declared with it): symbols only, version 8.
 *    And for spatial verification (hesaff_verify_matches and the six symbols declared with it): symbols only, version 8.
 *    And for vocabulary cells (hesaff_set_vocabulary_cells and the eight symbols declared with it): symbols only, version 8.
 *    And for vocabulary probes (hesaff_set_vocabulary_probes / hesaff_get_vocabulary_probes / hesaff_stage_probe_cells): symbols only, version 8.
 *    And for Hamming embedding (hesaff_set_embedding and the twenty symbols declared with it): symbols only, version 8.
 *    And for the growing, durable index (hesaff_index_add and the nine symbols declared with it): symbols only, version 8.
 *    And for batched index queries (hesaff_index_query_batch and the seven symbols declared with it): symbols only, version 8.
 *    And for vocabulary neighbours (hesaff_set_vocabulary_neighbours and the five symbols declared with it): symbols only, version 8.
 *    And for removal from the index (hesaff_index_remove, hesaff_get_index_remove_ms): symbols only, version 8.
 *    And for query expansion (hesaff_expand_query, hesaff_expand_query_device, hesaff_get_expand_ms): symbols only, version 8.
 * Image sizes: a side of at most 65535 pixels at the first pyramid level, and sqrt(width x height) of at most about 27900 (the largest window
 * normalizeAffine could ask for, affine.cpp:114-124, must fit a compute unit's LDS as one row): HESAFF_ERR_ARG beyond. */
#define HESAFF_ABI_VERSION 8
int hesaff_abi_version(void);
size_t hesaff_sizeof_params(void);
size_t hesaff_sizeof_timings(void);
size_t hesaff_sizeof_region(void);

typedef struct hesaff_ctx hesaff_ctx;

/* Parameters = the reference's compile-time structs flattened.
 * PyramidParams pyramid.h:18-41, AffineShapeParams affine.h:17-46,
 * SIFTDescriptorParams siftdesc.h:19-32, HessianAffineParams hesaff.cpp:21-36.
 * patchSize (41), smmWindowSize (19), spatialBins (4), orientationBins (8),
 * numberOfScales (3) and border (5) are fixed at the reference defaults. */
typedef struct hesaff_params {
   float threshold;            /* 16/3  pyramid.h:37, hesaff.cpp:30   */
   float edgeEigenValueRatio;  /* 10    pyramid.h:38                  */
   float initialSigma;         /* 1.6   pyramid.h:36 only: PyramidParams::initialSigma.  AffineShapeParams::initialSigma
                                *       (affine.h:40, read at affine.cpp:40) stays 1.6 whatever this is, as in the reference's
                                *       main, which sets neither (tests/test_reference.py pins this reading) */
   int maxIterations;          /* 16    affine.h:39, hesaff.cpp:31    */
   float convergenceThreshold; /* 0.05  affine.h:41                   */
   float mrSize;               /* 3*sqrt(3) affine.h:44, hesaff.cpp:32 */
   float maxBinValue;          /* 0.2   siftdesc.h:29                 */
   int upscaleInputImage;      /* 0     pyramid.h:34 (1: first octave on the 2x up-sampled image, helpers.cpp:297-329) */
   /* capacity knobs (no reference counterpart) */
   int max_batch;              /* images processed together on the device (default 64; hesaff_detect_batch pipelines chunks of this size) */
   int max_kpts_per_mpx;       /* candidate/keypoint capacity per megapixel (default 40000) */
   /* 0 (default): parity mode, results bit-identical to the reference's arithmetic.
    * 2: a different algorithm for the windows larger than the 41 x 41 patch (27 % of the keypoints, 3/4 of the patch stage's
    *    time): their samples are taken from the scale-space level whose blur matches (1681 taps) instead of warping and
    *    blurring a P x P window of the original (affine.cpp:114-135).  Detection, affine shapes, the set of described keypoints
    *    and the descriptors of the small windows stay those of parity mode; the other descriptors differ visibly, see DESIGN.md
    *    for the measured effect on descriptors and matching.
    * 1 was "the same algorithm with free summation order and approximate division" (ABI versions 2-3).  It bought 1.02x
    *    and is withdrawn: hesaff_create refuses it. */
   int fast;
} hesaff_params;

/* One detected + described region = the reference's `struct Keypoint` hesaff.cpp:41-48,
 * same field order and types (164 bytes). */
typedef struct hesaff_keypoint {
   float x, y, s;
   float a11, a12, a21, a22;
   float response;
   int32_t type;               /* HESSIAN_DARK 0 / BRIGHT 1 / SADDLE 2, pyramid.h:51-55 */
   uint8_t desc[128];
} hesaff_keypoint;

/* Per-image result of hesaff_detect_batch. keys is library-owned host memory, valid until
 * the next hesaff_detect_batch / hesaff_destroy on the same context.  Order = the
 * reference's detection order (octave, level, raster of the initial extremum). */
typedef struct hesaff_result {
   int32_t count_hessian;      /* g_numberOfPoints,       hesaff.cpp:38,68  */
   int32_t count_desc;         /* g_numberOfAffinePoints, hesaff.cpp:39,103 */
   const hesaff_keypoint *keys;
} hesaff_result;

/* Stage timings of the last device batch, milliseconds.  Every bracket is a HIP event pair recorded on the
 * stream its kernels are launched on.  pyramid / detect / pack run one after the other on the main stream; the
 * affine, patch and descriptor stages run CONCURRENTLY on their own streams over groups of images (three-deep
 * pipeline), so their three figures are per-stream busy times that overlap in wall-clock time: they add up to
 * more than total_ms - pyramid_ms - detect_ms - pack_ms. */
typedef struct hesaff_timings {
   float pyramid_ms;           /* grey + blur + Hessian + decimation (the roofline kernels) */
   float detect_ms;            /* extrema + localisation + ordering                          */
   float affine_ms;            /* Baumberg iteration, sum over groups (affine stream)        */
   float patch_ms;             /* rectify + normalizeAffine, sum over groups (main + bin streams) */
   float sift_ms;              /* descriptor kernels, sum over groups (descriptor stream)    */
   float pack_ms;              /* final stable compaction into hesaff_keypoint records       */
   float total_ms;
   float blur_hess_ms;         /* sum of the k_blur_hess launches only                       */
   int32_t blur_hess_launches;
   double blur_hess_bytes;     /* algorithmic bytes of those launches (12 N each, + 8 N with the fused R0, + 2 N with the fused decimation) */
   double pyramid_bytes;       /* algorithmic bytes B_pyr = 5 N0 + 58 sum N_k, whole batch   */
   /* appended in ABI version 3 (profiling level 2) */
   float extrema_ms;           /* sum of the k_extrema_march launches (3x3x3 extrema of the three scans of an octave) */
   int32_t extrema_launches;
   double extrema_bytes;       /* algorithmic bytes of those launches: 20 N per octave (five response planes read once), SURVEY.md 8d B_ext */
   /* appended in ABI version 4 */
   float export_ms;            /* hesaff_process_files: the export kernels (row lengths, offsets, text / sidecar rows) of the last chunk delivered */
   int32_t export_rows;        /* ... and the rows they formatted */
} hesaff_timings;

int hesaff_default_params(hesaff_params *p);

/* replaces: AffineHessianDetector ctor hesaff.cpp:56-64 (+ mask/table setup affine.h:71,
 * siftdesc.h:47-48).  device = HIP device ordinal. */
int hesaff_create(hesaff_ctx **out, const hesaff_params *p, int device);
void hesaff_destroy(hesaff_ctx *ctx);
const char *hesaff_last_error(const hesaff_ctx *ctx);   /* ctx may be NULL: last create error */

/* replaces: main()'s grey conversion hesaff.cpp:138-148 + detectPyramidKeypoints
 * hesaff.cpp:167 (pyramid.cpp:261) with the whole callback chain hesaff.cpp:66-105,
 * for n images at once.  images[i]: 8-bit, channels[i] = 1 (grey) or 3 (BGR as cv::imread
 * delivers; pass RGB bytes of a PPM in any order - the three are summed), row stride in
 * bytes.  Images of different sizes are allowed (grouped internally).  Chunks of max_batch images
 * are pipelined: host staging + H2D of the next chunk and D2H of the previous one overlap the
 * kernels of the current one.  results[i].keys point into library-owned pinned memory, valid
 * until the next call on this context. */
int hesaff_detect_batch(hesaff_ctx *ctx, int n, const uint8_t *const *images, const int *widths,
                        const int *heights, const int *strides, const int *channels, hesaff_result *results);

/* The same call with bounded host memory: results are handed to `sink` chunk by chunk (at most max_batch images at a
 * time, image_index[i] = position in the caller's arrays) and are valid only until sink returns; the library cycles
 * through three pinned result blocks however long the list is.  (hesaff_detect_batch keeps every chunk's block until
 * the next call: about 19 MB per dense UHD image, 39 GB for 2048 of them - use this form or hesaff_process_files for
 * long lists.)  A non-zero return of sink stops the run: HESAFF_ERR_IO. */
typedef int (*hesaff_chunk_sink)(void *user, int n_images, const int *image_index, const hesaff_result *results);
int hesaff_detect_batch_cb(hesaff_ctx *ctx, int n, const uint8_t *const *images, const int *widths, const int *heights,
                           const int *strides, const int *channels, hesaff_chunk_sink sink, void *user);

/* replaces: main() hesaff.cpp:133-180 for a list of image files - cv::imread (:137), grey conversion (:138-148),
 * detectPyramidKeypoints (:167), the output name <image>.hesaff.sift (:170-173) and exportKeypoints (:175) - as a
 * bounded three-stage host pipeline on one device: decode threads -> chunks of max_batch consecutive images of one
 * size through the device (copy in / kernels / copy out overlapped) -> writer threads.  Host memory stays bounded
 * (about 2 max_batch decoded images and three result blocks).  out_paths may be NULL (or hold NULLs): the reference's
 * name.  status[i].rc = HESAFF_OK, or why file i was skipped (unreadable input, unwritable output); one bad file does
 * not stop the others.  decode_threads / write_threads: 0 = auto (hesaff_host_plan_for(1): this context has the host to itself); the two counts add up to ONE pool of
 * host threads that decode when the look-ahead window has room and write otherwise.  The rows of the output files are formatted
 * on the device (hesaff.cpp:124-128 as a kernel): a writer only write()s what the copy engine delivered. */
#define HESAFF_FILE_PENDING 0   /* never reached (the run stopped on a device error before this file) */
#define HESAFF_FILE_UNREADABLE 1
#define HESAFF_FILE_DETECTED 2  /* detected and described, but the output file could not be written (rc says why) */
#define HESAFF_FILE_WRITTEN 3
#define HESAFF_FILE_REJECTED 4  /* decoded, but the device refused it: a side above 65535 pixels or a window the kernels cannot hold
                                   (rc = HESAFF_ERR_ARG), more keypoints than max_kpts_per_mpx plans for (HESAFF_ERR_CAPACITY); the other
                                   files of the list are not affected */
#define HESAFF_FILE_SKIPPED 5   /* hesaff_set_resume: the complete output of an earlier run exists; the image was not read (rc = HESAFF_OK,
                                   count_desc = the row count that output states, count_hessian = -1: not known) */
typedef struct hesaff_file_status {
   int32_t rc;                 /* HESAFF_OK only in stage HESAFF_FILE_WRITTEN */
   int32_t stage;              /* how far this file got: HESAFF_FILE_* */
   int32_t count_hessian;      /* g_numberOfPoints        hesaff.cpp:38 */
   int32_t count_desc;         /* g_numberOfAffinePoints  hesaff.cpp:39 */
} hesaff_file_status;
int hesaff_process_files(hesaff_ctx *ctx, int n, const char *const *paths, const char *const *out_paths, int decode_threads,
                         int write_threads, hesaff_file_status *status);
/* What hesaff_process_files writes for every image: HESAFF_OUT_TEXT (default) = <image>.hesaff.sift in the reference's text
 * format; HESAFF_OUT_BIN = <image>.hesaff.bin (hesaff_write_bin); HESAFF_OUT_TEXT | HESAFF_OUT_BIN = both.  With out_paths
 * given, the binary file is out_paths[i] + ".bin" when both are written, out_paths[i] itself when only the binary one is. */
#define HESAFF_OUT_TEXT 1
#define HESAFF_OUT_BIN 2
#define HESAFF_OUT_WORDS 4        /* <image>.hesaff.words (hesaff_write_words; needs a vocabulary, hesaff_set_vocabulary): alone or or-ed with the
                                     other two.  With out_paths given: out_paths[i] + ".words" when combined, out_paths[i] itself when alone. */
#define HESAFF_OUT_STRICT 0x100   /* hesaff_output_is_complete only: also count the rows of a text file (reads the whole file) */
int hesaff_set_output_format(hesaff_ctx *ctx, int format);
/* Resume a list that was interrupted (checkpoint / resume; no counterpart in the reference, which handles one
 * image per process): with on != 0 hesaff_process_files skips every image whose output file(s) of the selected format exist and
 * are complete - a .hesaff.sift with its two header lines, a plausible size and a final newline, a .hesaff.bin whose size matches its
 * row count (three small reads per file).  on = 2 (strict): the rows of an existing text file are counted as well - the whole file is
 * read, about 46 MB per dense 3840 x 2160 image, on the decode threads - for directories that a writer which does not rename its
 * outputs into place (the reference binary) may have left torn at a row boundary.  Every writer of this library puts its output under
 * a temporary name ("<name>.part.<pid>.<tid>") and renames it when it is complete, so a run that is killed never leaves a torn file
 * under the final name; a target that is not a regular file (/dev/stdout, a FIFO) or whose directory takes no new file is written in
 * place. */
int hesaff_set_resume(hesaff_ctx *ctx, int on);

/* replaces: the two virtual callbacks the reference chains its stages through - HessianKeypointCallback::onHessianKeypointDetected
 * (pyramid.h:43-47, installed by setHessianKeypointCallback pyramid.h:69) and AffineShapeCallback::onAffineShapeFound (affine.h:48-58,
 * installed by setAffineShapeCallback affine.h:87), chained by hesaff.cpp:66-105 - as one record per Hessian keypoint.  Records are
 * in the reference's call order (the order of onHessianKeypointDetected, = hesaff_stage_hessian_keypoints' order); 64 bytes each. */
typedef struct hesaff_region {
   float x, y, s, pixelDistance, response;  /* pyramid.cpp:203, the arguments of onHessianKeypointDetected                         */
   int32_t type;                            /* HESSIAN_DARK 0 / BRIGHT 1 / SADDLE 2, pyramid.h:51-55                               */
   int32_t octave, level;                   /* the `blur` plane passed: same indices as hesaff_stage_hessian_keypoints / hesaff_stage_pyramid */
   float a11, a12, a21, a22;                /* U as passed to onAffineShapeFound (affine.cpp:95), NOT rectified; 0 when not converged */
   int32_t iters;                           /* `l` at affine.cpp:95; 0 when not converged                                          */
   int32_t outcome;                         /* 0: findAffineShape returned false; 1: converged, normalizeAffine rejected (hesaff.cpp:82);
                                               2: described (a row of keys)                                                          */
   int32_t key;                             /* row of its record in this image's keys, -1 unless outcome == 2                      */
   int32_t reserved;                        /* 0 */
} hesaff_region;

/* Per-image result of hesaff_detect_regions: regions[count_hessian] (NULL when count_hessian is 0) and keys[count_desc], the latter
 * byte-identical to hesaff_detect_batch's keys for the same image.  Both are library-owned, valid until the next call on the context. */
typedef struct hesaff_region_result {
   int32_t count_hessian;      /* g_numberOfPoints,       hesaff.cpp:38,68  */
   int32_t count_desc;         /* g_numberOfAffinePoints, hesaff.cpp:39,103 */
   const hesaff_region *regions;
   const hesaff_keypoint *keys;
} hesaff_region_result;

/* hesaff_detect_batch that also returns every Hessian keypoint with what followed it (hesaff_region): the keypoints that got no
 * descriptor, the un-rectified U and iteration count of findAffineShape, and which row of keys each one became.  Same inputs, same
 * chunking and the same lifetime contract as hesaff_detect_batch; the records leave the device with the keys of their chunk.
 * The callbacks observe a chain that has already run: nothing a caller does with a record changes the later stages.  What a
 * caller kept of the records - or keypoints of its own - goes through the rest of the chain with hesaff_describe_regions below. */
int hesaff_detect_regions(hesaff_ctx *ctx, int n, const uint8_t *const *images, const int *widths, const int *heights,
                          const int *strides, const int *channels, hesaff_region_result *results);

/* ---- float grey planes: the reference's own detector input ----
 * replaces: detectPyramidKeypoints(const Mat &image) with a CV_32FC1 image (pyramid.h:73, pyramid.cpp:261-292) and the callback chain
 * hesaff.cpp:66-105 - what main() hands the detector after its grey conversion (hesaff.cpp:138-148), and what a caller that uses the
 * reference as a library passes when it made the plane itself (linearised or gamma-corrected images, 16-bit sources scaled to float,
 * planes normalised to [0, 1]).  Each _f32 entry point is its 8-bit twin with float planes in place of bytes: the same chunking, mixed
 * sizes, size limits and lifetime contract; from the grey plane on, the arithmetic is the one the twin runs.
 *
 * Input layout: images[i] is H x W float32, one channel, rows strides[i] BYTES apart (at least 4 * width and a multiple of 4; strides
 * NULL: tightly packed rows); every pointer 4-byte aligned.  Anything else: HESAFF_ERR_ARG.
 *
 * Accepted values: every pixel finite with |v| <= 2^20 (1048576) - [0, 1], [0, 255] and [0, 65535] inputs with room to spare.  An image
 * with a NaN, an infinity or a larger magnitude makes the whole call return HESAFF_ERR_ARG; hesaff_last_error names the caller's image
 * index and the first offending pixel in raster order (row, column, value).  The context stays usable.  (The reference takes any float;
 * this bound is a deliberate difference, INTEGRATION.md.)  Where the check runs: the host entry points check each image while the
 * staging thread copies it into pinned memory (no extra pass over the caller's list); hesaff_detect_batch_device_f32 runs a read-only
 * check kernel over the planes first.  Either way no refused value reaches a keypoint kernel.
 * Why 2^20 is enough: no pixel value ever forms an address (every index comes from the image geometry, or from keypoint positions
 * clamped to the plane), and no intermediate overflows float: a blur is a convex combination (|L| <= 2^20); the Hessian terms of
 * pyramid.cpp:95-100 stay below 2^22 and the response below 2^45 sigma^4 (2^53 at the default sigmas, sigma <= 4.1); localisation's
 * second differences stay below 2^56, its edge score below 2^113, and solveLinear3x3 (helpers.cpp:46-90) pivots, so its multipliers
 * are at most 1; the affine stage's second-moment sums of squared gradients (19 x 19 window) stay below 2^52 and its eigenvalue terms
 * below 2^105; normalizeAffine interpolates (|v| <= 2^20), and the SIFT stage's mean / variance sums stay below 2^52 before the patch is
 * normalised.  Every one is far below 2^128.
 *
 * hesaff_detect_batch_cb_f32: chunks before a refused image may already have gone to the sink when the call returns HESAFF_ERR_ARG. */
int hesaff_detect_batch_f32(hesaff_ctx *ctx, int n, const float *const *images, const int *widths, const int *heights, const int *strides,
                            hesaff_result *results);
int hesaff_detect_batch_cb_f32(hesaff_ctx *ctx, int n, const float *const *images, const int *widths, const int *heights,
                               const int *strides, hesaff_chunk_sink sink, void *user);
/* records and keys as hesaff_detect_regions returns them */
int hesaff_detect_regions_f32(hesaff_ctx *ctx, int n, const float *const *images, const int *widths, const int *heights,
                              const int *strides, hesaff_region_result *results);
/* hesaff_detect_batch_device with float planes already in device memory: plane b starts img_stride bytes after plane b-1, its rows are
 * row_stride bytes apart (0 = tightly packed: row_stride = 4 * width, img_stride = row_stride * height); n <= max_batch.  A check kernel
 * reads the planes first and the call returns HESAFF_ERR_ARG (naming the image, 0-based in this call) before any detection kernel runs. */
int hesaff_detect_batch_device_f32(hesaff_ctx *ctx, int n, const void *d_planes, int width, int height, int row_stride,
                                   int64_t img_stride, int32_t *count_hessian, int32_t *count_desc, const void **d_keys_out,
                                   int64_t *total_out);

/* ---- describe caller-supplied keypoints: the second half of the chain, entered where the reference's callbacks enter it ----
 * replaces: a caller's own calls of the two public callback members of AffineHessianDetector - onHessianKeypointDetected
 * (hesaff.cpp:66-71: findAffineShape on the blur plane, then hesaff.cpp:73-105 when it converges) and onAffineShapeFound
 * (hesaff.cpp:73-105: rectify, normalizeAffine, SIFT) - for counts[i] records of image i, n images at once: what a subclass that keeps
 * the strongest N keypoints (or those inside a mask) before findAffineShape does, and what a caller with a detector of its own does.
 *   from = HESAFF_FROM_POINTS: as calling onHessianKeypointDetected(blur, x, y, s, pixelDistance, type, response) per record, with
 *          blur = the scale-space plane (octave, level) of image i and pixelDistance that octave's own;
 *   from = HESAFF_FROM_SHAPES: as calling onAffineShapeFound(blur, x, y, s, pixelDistance, a11, a12, a21, a22, type, response, iters)
 *          per record (blur and pixelDistance are not used by hesaff.cpp:73-105).  No scale space is built in parity mode (fast = 0):
 *          the grey plane is all normalizeAffine needs; fast = 2 builds it, because its larger windows are sampled from it.
 * The input record is hesaff_region itself: what hesaff_detect_regions returned, whole or any subset in any order (a record given
 * twice is described twice), goes straight back in.  Fields read: x, y, s, response, type always; octave, level with
 * HESAFF_FROM_POINTS only (the indices hesaff_detect_regions reports; only planes the detector finds keypoints on: octave below the
 * image's octave count, level 0..2); a11..a22 (U as onAffineShapeFound receives it, NOT rectified) and iters (echoed) with
 * HESAFF_FROM_SHAPES only.  pixelDistance, outcome, key and reserved are ignored on input, and so are a11..a22 and iters with
 * HESAFF_FROM_POINTS.  With HESAFF_FROM_SHAPES octave and level are echoed (taken as 0 when outside what a record can name, octave
 * 0..15 and level 0..3).  Records that hesaff_detect_regions returned with outcome == 0 carry a zero U: drop them before
 * HESAFF_FROM_SHAPES, which refuses them (below).
 * Output: results[i] as hesaff_detect_regions fills it, same lifetime contract: count_hessian = counts[i]; regions[counts[i]] in the
 * caller's order with pixelDistance = the octave's own value (pd0 * 2^octave, pd0 = 0.5 with upscaleInputImage, else 1), a11..a22,
 * iters, outcome and key as hesaff_detect_regions defines them (HESAFF_FROM_SHAPES: U and iters echoed, outcome 1 or 2, never 0);
 * keys[count_desc] in the caller's record order (keys.push_back in call order, hesaff.cpp:87).  counts[i] == 0: an empty result
 * (regions[i] may then be NULL; results[i].regions is NULL).  Mixed image sizes and chunks of max_batch images as in
 * hesaff_detect_regions; a chunk's records travel with its images (staged into pinned memory, one copy in).
 * Refused (HESAFF_ERR_ARG; hesaff_last_error names the caller's image index and the first offending record of that image; the context
 * stays usable): from not 1 or 2; counts[i] < 0, or regions[i] NULL with counts[i] > 0; type not in 0..2; octave or level outside
 * the image's pyramid (HESAFF_FROM_POINTS); x, y, s or response not finite; |x| or |y| above 2^20; s not in (0, 2^20]; with
 * HESAFF_FROM_SHAPES also an a_ij that is not finite or exceeds 2^20 in magnitude, and - evaluated in double -
 * a11 * a22 - a12 * a21 == 0 or a11^2 + a12^2 == 0, the two divisors of rectifyAffineTransformationUpIsUp (helpers.cpp:90-97).
 * More records in a chunk than the context's keypoint capacity for it (max_kpts_per_mpx): HESAFF_ERR_CAPACITY.
 * The records are checked on the host while the staging thread copies them into pinned memory: no refused value reaches a kernel.
 * Why the accepted ranges are safe: a position never forms an address unchecked - findAffineShape's taps (k_affine) and normalizeAffine's
 * (the patch kernels) are either proven inside the plane by the four corners of their window (hs_window_outside, interpolateCheckBorders)
 * or individually tested, an outside tap reading pixel (0, 0) and contributing 0 (helpers.cpp:227-240), and the tests are written so
 * that a NaN or infinite coordinate counts as outside.  With |x|, |y|, s <= 2^20 and pixelDistance >= 0.5 the window coordinates of
 * the first iteration stay below 2^45; later iterations may overflow U to infinity or NaN for absurd keypoints, which the tests above
 * classify as outside, after which the iteration ends unconverged (as it does in the reference).  The window side 2 * int(ceil(s *
 * mrSize)) + 1 is formed through a guard that saturates at 10^6 (hs_window_p0) and a window wider than the tabulated taps (about
 * sqrt(width * height)) is rejected, not tabulated, so no scale sizes a buffer.  With HESAFF_FROM_SHAPES the rectified matrix
 * (helpers.cpp:90-97) is finite or has infinite entries of a definite sign - never NaN, since both divisors are non-zero and every
 * term is below 2^41 in double - and an infinite corner fails interpolateCheckBorders' comparisons, so such a record is rejected
 * (outcome 1) like any window that leaves the image. */
#define HESAFF_FROM_POINTS 1   /* = calling onHessianKeypointDetected per record: hesaff.cpp:66-71, then :73-105 when findAffineShape converges */
#define HESAFF_FROM_SHAPES 2   /* = calling onAffineShapeFound per record: hesaff.cpp:73-105 (rectify, normalizeAffine, SIFT) */
int hesaff_describe_regions(hesaff_ctx *ctx, int n, const uint8_t *const *images, const int *widths, const int *heights,
                            const int *strides, const int *channels, const hesaff_region *const *regions, const int *counts, int from,
                            hesaff_region_result *results);
/* the same with float grey planes: input layout, accepted pixel values and their check as the other _f32 entry points */
int hesaff_describe_regions_f32(hesaff_ctx *ctx, int n, const float *const *images, const int *widths, const int *heights,
                                const int *strides, const hesaff_region *const *regions, const int *counts, int from,
                                hesaff_region_result *results);

/* ---- a keypoint budget per image: the N strongest Hessian keypoints, chosen on the device ----
 * No counterpart in the reference, whose caller would filter inside HessianKeypointCallback::onHessianKeypointDetected (pyramid.h:43-47)
 * - once the whole list is known, so in a second pass - before findAffineShape.  Here the context holds keypoint_limit, an int:
 * 0, the default, means no limit, and everything is bit for bit what it is without this call.  With limit N >= 1, for each image the N
 * Hessian keypoints of greatest strength are kept; the rest are discarded before findAffineShape and cost nothing after detection.
 * Strength of keypoint i is |response_i|, the float `response` of onHessianKeypointDetected (saddles and dark blobs have negative
 * responses; responses are finite and non-zero because they passed the threshold, so comparing the strengths as floats and comparing
 * the uint32 bit patterns of fabsf(response) is the same order).  With i the keypoint's position in the reference's detection order
 * within its image, keypoint i is kept iff
 *    #{j : |r_j| > |r_i|} + #{j < i : |r_j| == |r_i|} < N:
 * ties at the cut go to the earlier keypoint; the result does not depend on launch geometry and is the same from run to run.
 * The kept keypoints stay in the reference's order, and everything downstream (regions, keys, text rows, the callbacks hesaff.hpp
 * replays) is what the unlimited run produces for those keypoints, bit for bit, in that order: a keypoint's chain does not depend on
 * the other keypoints, so a kept keypoint's hesaff_region record equals its unlimited record except for `key`, which is renumbered
 * over the image's kept, described keypoints, and its hesaff_keypoint bytes equal its unlimited key.
 * count_hessian is the number kept, min(N, detected); count_desc <= count_hessian.  N bounds the Hessian keypoints, NOT the descriptors:
 * the strongest keypoints are often saddles on which findAffineShape does not converge, so expect fewer than N keys.
 * The limit applies to every entry point that detects - hesaff_detect_batch, _cb, _f32, _cb_f32, hesaff_detect_regions, _f32,
 * hesaff_detect_batch_device, _device_f32, hesaff_process_files - with any parameter set (fast = 2, upscaleInputImage = 1: the
 * selection comes before either matters).  It does not apply to hesaff_describe_regions* (the records are the caller's) or to the
 * hesaff_stage_* operators.  max_kpts_per_mpx still has to hold every DETECTED keypoint: the selection runs after the ordering step.
 * n: 0 = off.  n < 0 or ctx NULL: HESAFF_ERR_ARG (hesaff_get_keypoint_limit: ctx or n NULL). */
int hesaff_set_keypoint_limit(hesaff_ctx *ctx, int n);
int hesaff_get_keypoint_limit(const hesaff_ctx *ctx, int *n);

/* ---- per-image detection masks: keypoints off the mask are dropped on the device (OpenCV's detect(image, keypoints, mask)) ----
 * The other half of the sentence above hesaff_describe_regions: a caller of the reference who wants keypoints only inside a mask
 * filters inside onHessianKeypointDetected (pyramid.h:43-47).  Here the masks are armed for the NEXT detecting call on the context
 * and consumed (cleared) by that call whatever it returns; the selection runs where the keypoint limit runs, between detection's
 * ordering step and findAffineShape.
 * Each image may have a mask: height x width 8-bit pixels, one channel, at the size of the image as passed - also with
 * upscaleInputImage = 1, since keypoint coordinates are in the caller's pixels.  Non-zero means "detect here".  Hessian keypoint i of
 * an image with a mask is eligible iff mask[row][col] != 0 with
 *    col = clamp((int)(x + 0.5f), 0, width - 1),  row = clamp((int)(y + 0.5f), 0, height - 1)
 * - the add in binary32, the conversion truncating (OpenCV's runByPixelsMask rounding, clamped); x, y are the floats
 * onHessianKeypointDetected receives.  In numpy: np.clip((x + np.float32(0.5)).astype(np.int32), 0, W - 1).  An image without a mask
 * has every keypoint eligible.  Ineligible keypoints are discarded before findAffineShape and cost nothing after detection.
 * With a keypoint limit N >= 1 the rule of hesaff_set_keypoint_limit applies over the eligible keypoints only (counts and ties among
 * eligible j; ties at the cut to the earlier one): mask first, then the N strongest of what is left.  With limit 0 every eligible
 * keypoint is kept.  Kept keypoints stay in the reference's order; count_hessian is the number kept; each hesaff_region record equals
 * its unmasked record except `key`, which is renumbered, and each hesaff_keypoint has the bytes of its unmasked key; text rows, sidecar
 * rows and the callbacks hesaff.hpp replays follow from these records.  max_kpts_per_mpx must still hold every DETECTED keypoint: the
 * mask acts after the ordering step.  The result does not depend on launch geometry and is the same from run to run.
 *
 * hesaff_set_next_masks (host memory) serves hesaff_detect_batch, _cb, _f32, _cb_f32, hesaff_detect_regions and _f32.  masks[i]
 * belongs to image i of that call, NULL = image i is unmasked; strides[i] = bytes between the rows of mask i, >= width (strides NULL:
 * tightly packed).  The two lists are copied here, the planes are not: they must stay valid until the detecting call returns.
 * n = 0 (or masks NULL with n = 0) disarms.  ctx NULL, n < 0, or n > 0 with masks NULL: HESAFF_ERR_ARG.  At the call: n differing
 * from the call's n, or a stride below the image's width: HESAFF_ERR_ARG (hesaff_last_error names both counts / the image), and the
 * masks are cleared.
 * hesaff_set_next_masks_device serves hesaff_detect_batch_device and _device_f32: n planes in device memory, row_stride / img_stride
 * in bytes, 0 = tight (row_stride = width, img_stride = row_stride * height).  A negative stride: HESAFF_ERR_ARG.
 * Masks armed in host memory that meet a device-resident call, or the reverse: HESAFF_ERR_ARG, masks cleared.
 * While masks are armed, hesaff_describe_regions* (the records are the caller's) and hesaff_process_files (no masks travel with a
 * file list) return HESAFF_ERR_ARG and clear them; the hesaff_stage_* operators neither read nor clear them.  The context stays
 * usable after every refusal. */
int hesaff_set_next_masks(hesaff_ctx *ctx, int n, const uint8_t *const *masks, const int *strides);
int hesaff_set_next_masks_device(hesaff_ctx *ctx, int n, const void *d_masks, int row_stride, int64_t img_stride);

/* ---- a spatially uniform keypoint budget: the N / (rows * cols) strongest Hessian keypoints of every cell of a grid ----
 * OpenCV 2.4's GridAdaptedFeatureDetector(detector, maxTotalKeypoints, gridRows, gridCols), with one stated difference: OpenCV runs the
 * detector on every sub-image, here the selection is taken from the full image's detection, so there are no border effects at the
 * seams of the cells.  The context holds a grid R x C, default 1 x 1 (no grid).  With keypoint limit N >= 1 and R * C > 1 let
 * Q = N / (R * C) in integer division.  For an image of W x H pixels as the caller passed it (also with upscaleInputImage = 1, as for
 * the masks):
 *  - keypoint i has the pixel col = clamp((int)(x + 0.5f), 0, W - 1), row = clamp((int)(y + 0.5f), 0, H - 1) - the add in binary32, the
 *    conversion truncating: the masks' rule, the same code;
 *  - its cell is cr * C + cc with cr = ((row + 1) * R - 1) / H and cc = ((col + 1) * C - 1) / W in integer division: the closed form
 *    of OpenCV's cell ranges, row in [cr * H / R, (cr + 1) * H / R) and columns likewise.  It is NOT row * R / H: the two differ wherever
 *    H is no multiple of R;
 *  - a keypoint is eligible under the masks' rule (an image without a mask: every keypoint);
 *  - an eligible keypoint i of cell k is kept iff
 *       #{j eligible in cell k : |r_j| > |r_i|} + #{j < i, eligible in cell k : |r_j| == |r_i|} < Q:
 *    mask first, then the Q strongest of every cell; ties at a cell's cut go to the earlier keypoint of the reference's order;
 *  - the unused quota of a sparse cell is not handed to other cells (OpenCV's adapter does not do that either).
 * count_hessian is the number kept, at most Q * R * C <= N.  Kept keypoints stay in the reference's order; each hesaff_region equals its
 * unlimited record except `key`, which is renumbered, and each hesaff_keypoint has the bytes of its unlimited key.  The result does not
 * depend on launch geometry and is the same from run to run.
 * Limit 0 with a grid set: the grid is inert.  A 1 x 1 grid: hesaff_set_keypoint_limit's rule, and its code path.
 * Scope: the limit's - every detecting entry point and hesaff_process_files, with any parameter set and orientation mode; not
 * hesaff_describe_regions* nor the hesaff_stage_* operators.
 * rows, cols >= 1 and rows * cols <= 64.  HESAFF_ERR_ARG: ctx NULL; a getter pointer NULL; a value out of range; a grid that would leave
 * Q = 0 under the current limit (0 < N < rows * cols).  hesaff_set_keypoint_limit likewise refuses 0 < n < R * C under the current grid
 * (with the default grid it accepts what it always did).  A refused call changes no state, so the two setters never leave a context that
 * a detecting call would have to refuse: to go from (N, R x C) to a smaller N and a smaller grid, set the grid first. */
int hesaff_set_keypoint_grid(hesaff_ctx *ctx, int rows, int cols);
int hesaff_get_keypoint_grid(const hesaff_ctx *ctx, int *rows, int *cols);

/* ---- dominant-orientation mode: rotation-invariant descriptors ----
 * Replaces nothing: the reference describes every region in the "up is up" frame of rectifyAffineTransformationUpIsUp (hesaff.cpp:79,
 * helpers.cpp:90-97) and has no other.  The detector and the affine shapes follow an in-plane rotation of the image, the descriptors
 * of that frame do not.  With HESAFF_ORI_DOMINANT the frame of every keypoint is turned by the dominant gradient angle of its own
 * patch, on the device, between two runs of normalizeAffine.  The definition is this library's; everything is binary32 unless stated,
 * no FMA contraction, operations evaluated left to right as written, sqrt and / IEEE-exact.  For one keypoint, p is the 41 x 41 patch
 * normalizeAffine produced for the up-is-up matrix A (the raw values, before photometric normalisation), M is
 * computeCircularGaussMask(41) (hesaff_table_circ_gauss_mask), PI = (float)M_PI, atan2f as hesaff_stage_math computes it (glibc's):
 *  1. for r, c in 1..39:  gx = p[r][c+1] - p[r][c-1],  gy = p[r+1][c] - p[r-1][c],  w = M[r][c] * sqrtf(gx*gx + gy*gy),
 *     t = (atan2f(gy, gx) + PI) * (36.0f / (2.0f * PI)),  b = (int)t truncating, b >= 36: b -= 36;
 *  2. row[r][b] accumulates w over c = 1..39 in increasing c, starting from +0;
 *  3. h[b] = ((row[1][b] + row[2][b]) + ...) + row[39][b], in increasing r, starting from +0;
 *  4. six times, circularly, every h' from the previous h:  h'[b] = ((h[b-1] + h[b]) + h[b+1]) / 3.0f;
 *  5. m = the lowest index of the maximum of h.  h[m] == 0: theta = 0 and A' = A bit for bit.  Otherwise, with l = h[m-1], q = h[m],
 *     r = h[m+1] (circular):  den = (l + r) - (q + q),  off = den == 0 ? 0 : (0.5f * (l - r)) / den,
 *     theta = (((float)m + 0.5f) + off) * ((2.0f * PI) / 36.0f) - PI;
 *  6. c, s = cos theta, sin theta of that binary32 theta, each computed in binary64 and rounded once to binary32 (the correctly
 *     rounded value but for an angle in 3e8);  A' = A * R(theta):  a11' = a11*c + a12*s,  a12' = a12*c - a11*s,
 *     a21' = a21*c + a22*s,  a22' = a22*c - a21*s;  normalizeAffine(image, x, y, s, A') runs again, its patch goes to the SIFT
 *     descriptor, and A' is what the hesaff_keypoint stores.
 * What follows:  a keypoint is described iff normalizeAffine accepts it in BOTH runs, otherwise its hesaff_region has outcome 1 and no
 * key.  hesaff_region is unchanged: U stays un-rectified and un-turned, x, y, s, response, type, iters as in mode 0.  The ellipse and
 * the text row are unchanged up to rounding (A' * A'^T = A * A^T); the file formats carry no orientation; theta is recoverable from
 * a key as atan2(-a12', a11'), because the rectified a12 is 0 and a11 > 0.  One orientation per keypoint, unless an orientation count is set (the next block).
 * The mode is context state, like the keypoint limit.  HESAFF_ORI_UP, the default, is today's behaviour bit for bit: nothing is
 * launched, allocated or copied for the mode.  HESAFF_ORI_DOMINANT applies to every detecting entry point (hesaff_detect_batch*,
 * hesaff_detect_regions*, hesaff_detect_batch_device*), to hesaff_process_files and to hesaff_describe_regions* in both `from` modes
 * (HESAFF_FROM_SHAPES rectifies the caller's U, then orients), with any parameter set - with fast = 2 the first run's patch, however
 * it was sampled, feeds the estimator - and composes with the keypoint limit and the masks, which act before the affine stage.  It
 * does not apply to the hesaff_stage_* operators.  The second run doubles patch_ms and, the patch stage being the longest stream, the step
 * (measured: DESIGN.md section 7).
 * ctx NULL or mode not 0 / 1: HESAFF_ERR_ARG (hesaff_get_orientation: ctx or mode NULL). */
#define HESAFF_ORI_UP 0
#define HESAFF_ORI_DOMINANT 1
int hesaff_set_orientation(hesaff_ctx *ctx, int mode);
int hesaff_get_orientation(const hesaff_ctx *ctx, int *mode);

/* ---- secondary orientation peaks: up to four keys per region ----
 * Lowe's detector, OpenCV and VLFeat emit one descriptor per histogram peak within 80 % of the maximum; on a patch with two comparable
 * gradient directions the highest peak flips between views, and a matcher that holds one of the two descriptors loses the region.  The
 * context has an ORIENTATION COUNT K in 1..4, default 1, read only in HESAFF_ORI_DOMINANT; in HESAFF_ORI_UP it is inert, as a keypoint
 * grid is with limit 0.  The arithmetic conventions are those of the block above.  For one keypoint, with h[0..35] after step 4 and m
 * from step 5:
 *  - flat histogram: h[m] == 0: one orientation, theta = 0, A' = A bit for bit, as with K = 1;
 *  - candidates: otherwise every bin b != m with h[b] > h[b-1], h[b] > h[b+1] and h[b] >= 0.8f * h[m] - the neighbour comparisons strict
 *    and circular, the product one binary32 multiplication, a comparison with a NaN false - ordered by h[b] descending, equal heights
 *    lower bin first;
 *  - ranks: rank 0 is bin m, rank j >= 1 the j-th candidate; n_ori = min(K, 1 + number of candidates);
 *  - angle: theta_j is step 5's formula with (l, q, r) taken around bin b_j, its `den == 0 -> off = 0` clause included;
 *  - frame: A'_j = A * R(theta_j) by step 6, each from the same up-is-up A - the frames are never cumulative;
 *  - keys: for every rank j < n_ori, normalizeAffine(image, x, y, s, A'_j) runs; if it accepts, that patch goes to the descriptor (SIFT
 *    or RootSIFT, as the context says) and makes one hesaff_keypoint that stores A'_j.
 * A region has keys iff the first run of normalizeAffine (on A) accepted it, and its keys are those ranks whose own run accepted: rank 0
 * may be rejected while a later rank is described.
 * Output: the keys of one region are adjacent, in ascending rank, and regions stay in the reference's order.  In a hesaff_region, outcome
 * is 2 iff the region has at least one key, `key` is the row of its first key and `reserved` the number of its keys (-1 and 0 without a
 * key); every other field is unchanged.  count_desc MAY EXCEED count_hessian: a caller sizes for up to K keys per region.  Text and
 * sidecar rows follow from the keys; the formats carry no rank.  The keys of a chunk must fit the keypoint capacity
 * (hesaff_params.max_kpts_per_mpx) the result blocks are sized for: otherwise the call returns HESAFF_ERR_CAPACITY and the context stays
 * usable.
 * K = 1 is the dominant-orientation mode as it stands - every byte, `reserved` = 0 included, every kernel launched, nothing allocated.
 * The first call with K > 1 allocates 152 bytes per keypoint of capacity and rank above 0 (HESAFF_ERR_NOMEM when the device cannot hold
 * them), and a batch runs K patch passes and K descriptor chains per image group besides pass one; a pass with no live keypoint costs
 * its launches.  Scope: that of the orientation mode.
 * HESAFF_ERR_ARG, with nothing changed: ctx NULL, k outside 1..4 (hesaff_get_orientation_count: ctx or k NULL). */
int hesaff_set_orientation_count(hesaff_ctx *ctx, int k);
int hesaff_get_orientation_count(const hesaff_ctx *ctx, int *k);

/* ---- descriptor mode: SIFT or RootSIFT bytes ----
 * Replaces nothing: the reference has the L2-normalised, clipped, 512-scaled SIFT byte vector only (siftdesc.cpp:98-113).  RootSIFT
 * (Arandjelovic and Zisserman 2012) L1-normalises the vector and takes element-wise square roots, so that the Euclidean distance of
 * two results is the Hellinger kernel of the histograms.  A caller cannot do that well from the 0..255 bytes, which are truncated
 * already; the float vector is in registers at the end of the descriptor kernel, where the mode costs one more 128-term sum, eight
 * divisions and eight square roots per lane.  The definition is this library's; everything is binary32, no FMA contraction, / and
 * sqrtf IEEE-exact.  Let v[0..127] be `vec` as it stands after siftdesc.cpp:102-106: normalize, clip at maxBinValue, normalize again
 * only if a bin was clipped.
 *  HESAFF_DESC_SIFT (0, the default):  byte[i] = min((int)(512.0f * v[i]), 255) - today's bytes, bit for bit; nothing is launched,
 *     allocated or copied for the mode.
 *  HESAFF_DESC_ROOTSIFT (1):
 *   1. s = ((v[0] + v[1]) + ...) + v[127], in increasing i, starting from +0 (every v[i] is +0 or positive: the L1 norm);
 *   2. u[i] = sqrtf(v[i] / s);
 *   3. byte[i] = min((int)(512.0f * u[i]), 255), truncating; byte[i] = 0 where 512.0f * u[i] is NaN (the existing guard: only the
 *      all-zero histogram gets there, whose v is NaN in both modes).
 * u has unit L2 norm, so the scale 512 and the saturation at 255 keep the meaning they have for SIFT.  Every other field of
 * hesaff_keypoint and hesaff_region, the set and order of the described keypoints, the counts and the file formats (which carry no
 * flag for the mode) are those of mode 0.
 * The mode is context state, like the orientation.  It applies to every entry point that produces descriptors: hesaff_detect_batch*,
 * hesaff_detect_regions*, hesaff_detect_batch_device*, hesaff_process_files (text and sidecar rows) and hesaff_describe_regions* in
 * both `from` modes, with any parameter set (fast = 2, upscaleInputImage), and composes with the dominant orientation, the keypoint
 * limit, the grid and the masks.  It does not apply to the hesaff_stage_* operators: hesaff_stage_sift, _parts and _alive stay SIFT
 * whatever the context holds, hesaff_stage_sift_mode takes the mode as an argument.
 * ctx NULL or mode not 0 / 1: HESAFF_ERR_ARG, nothing changed (hesaff_get_descriptor: ctx or mode NULL). */
#define HESAFF_DESC_SIFT 0
#define HESAFF_DESC_ROOTSIFT 1
int hesaff_set_descriptor(hesaff_ctx *ctx, int mode);
int hesaff_get_descriptor(const hesaff_ctx *ctx, int *mode);

/* Visual-word assignment (no counterpart in the reference; the quantisation step of a retrieval pipeline): the nearest row of a
 * vocabulary for every key, found on the device, so that a caller keeps (x, y, a, b, c, word) per region instead of 128 bytes.
 * A vocabulary is K rows of 128 unsigned bytes, 1 <= K <= 2^20, in the byte space of the descriptors the context produces (SIFT or
 * RootSIFT: the library does not check which).  For a key with descriptor bytes d[0..127]:
 *     dist2(k) = sum_j (d[j] - w_k[j])^2        integers, at most 128 * 255^2 = 8 323 200
 *     word     = the LOWEST k that minimises dist2(k)
 *     dist2    = dist2(word)
 * No floating point, no approximation, no dependence on launch geometry: exact, ties to the lowest row.  (On the device: with
 * d' = d ^ 0x80 and w' = w ^ 0x80 read as signed bytes, dist2(k) = |d'|^2 + |w'_k|^2 - 2 d'.w'_k, every term within int32, the dot
 * products on the i8 matrix instructions; kernels_words.h.)
 * hesaff_set_vocabulary: words[k][128], copied to the device; k = 0 (words may be NULL): no vocabulary, the default.  The vocabulary
 * is context state, like the descriptor mode.  With none set everything is bit for bit what it is without this feature: nothing is
 * launched, allocated or copied.  With one set, every entry point that produces keys also assigns their words: hesaff_detect_batch*,
 * hesaff_detect_regions*, hesaff_describe_regions*, hesaff_detect_batch_device* and hesaff_process_files; the keys do not change by a bit.
 * HESAFF_ERR_NOMEM: the device cannot hold the vocabulary; the previous one stays set.
 * hesaff_get_words: `image` is the caller's image index of the last host call; *words = int32_t[count][2] = (word, dist2), row for row
 * that image's `keys` (count == count_desc: with an orientation count above 1 one row per key, not per region); *words is NULL when
 * count is 0.  The pointer lives as long as the keys do; in the _cb forms it is valid inside the sink for the images of the chunk
 * being delivered.
 * hesaff_get_words_device: the device array parallel to d_keys_out of the last device-resident call.
 * hesaff_assign_words_device: words for n caller-held descriptors in device memory; descriptor i is the 128 bytes at d_desc + i * stride
 * + offset (stride = 164, offset = 36: a hesaff_keypoint array; stride = 128, offset = 0: a packed tensor); d_words_out receives n x 2
 * int32.  hesaff_stage_assign_words: the same for desc[n][128] in host memory, words_out[n][2].
 * hesaff_get_assign_ms: the HIP-event time of the last batch's assignment launch at profiling level >= 1 (0 otherwise).
 * HESAFF_ERR_ARG, nothing changed, the context usable as before: ctx NULL; k < 0 or k > 2^20; words NULL with k > 0; a getter's out
 * pointer NULL; hesaff_get_words*, hesaff_assign_words_device, hesaff_stage_assign_words, or HESAFF_OUT_WORDS in hesaff_process_files,
 * with no vocabulary set; `image` outside the last host call's images; stride < 128, offset < 0, offset + 128 > stride, or stride,
 * offset or a device pointer not a multiple of 4; n < 0. */
int hesaff_set_vocabulary(hesaff_ctx *ctx, int k, const uint8_t *words);
int hesaff_get_vocabulary_size(const hesaff_ctx *ctx, int *k);
int hesaff_get_words(const hesaff_ctx *ctx, int image, const int32_t **words, int *count);
int hesaff_get_words_device(const hesaff_ctx *ctx, const void **d_words, int64_t *total);
int hesaff_assign_words_device(hesaff_ctx *ctx, int64_t n, const void *d_desc, int64_t stride, int64_t offset, void *d_words_out);
int hesaff_stage_assign_words(hesaff_ctx *ctx, int n, const uint8_t *desc, int32_t *words_out);
int hesaff_get_assign_ms(const hesaff_ctx *ctx, float *ms);
/* The words file of an image, what a retrieval index keeps of its keys.  Little-endian:
 *   char magic[8] = "HESAFFW1"; uint32 vocabulary_size; uint32 count; count x { float x, y, a, b, c; uint32 word }   (24 bytes per row)
 * The five floats are those of hesaff_write_bin's row of the same key; words = (word, dist2) per key as hesaff_get_words hands them. */
int hesaff_write_words(const char *path, const hesaff_keypoint *keys, const int32_t *words, int n, float mrSize, int vocabulary_size);
/* Vocabulary file.  Little-endian:  char magic[8] = "HESAFFV1"; uint32 dim = 128; uint32 count; count x uint8[128]
 * hesaff_read_vocabulary: *words is malloc'ed (hesaff_free); HESAFF_ERR_IO for a file that cannot be read or is not a whole vocabulary
 * file (magic, dim, count outside 1 .. 2^20, size other than 16 + 128 count). */
int hesaff_read_vocabulary(const char *path, uint8_t **words, int *k);
int hesaff_write_vocabulary(const char *path, const uint8_t *words, int k);

/* Vocabulary training (no counterpart in the reference): exact integer k-means on the device, which produces the vocabulary that
 * hesaff_set_vocabulary consumes.  Inputs: n descriptors d_i of 128 unsigned bytes, 1 <= n <= 2^24; K rows, 1 <= K <= 2^20; T >= 1
 * iterations; an initial vocabulary V_0 of K rows (`init`), or init == NULL: row k of V_0 is d_floor(k n / K), the product in 64 bits,
 * which needs n >= K.  Iteration t = 1 .. T:
 *     (word_i, dist2_i) = hesaff_set_vocabulary's assignment under V_{t-1}: the lowest row of least squared distance
 *     count[k]          = #{i : word_i = k}
 *     sum[k][j]         = sum of d_i[j] over the keys with word_i = k
 *     distortion[t-1]   = sum_i dist2_i                                   (int64)
 *     empty[t-1]        = #{k : count[k] = 0}
 *     V_t[k][j]         = (2 sum[k][j] + count[k]) / (2 count[k])         integer division in 64 bits: the mean rounded half up
 *     V_t[k]            = V_{t-1}[k] where count[k] = 0: an empty word keeps its row, nothing is reseeded
 *     V_t == V_{t-1} byte for byte: stop, iterations_done = t.  Otherwise iterations_done = T.
 * Output: V_{iterations_done}, and distortion[] / empty[] for the iterations that ran.  distortion[t-1] belongs to V_{t-1}; the
 * distortion of the returned vocabulary itself is not computed.
 * No floating point, no dependence on launch geometry or on the order of accumulation: every call with the same inputs returns the
 * same bytes.  The rounded mean is the integer row that minimises a word's squared error over its keys, and the assignment minimises
 * every key's distance over the rows, so distortion[t] <= distortion[t-1], always.
 * n <= 2^24 so that a sum fits uint32 (2^24 * 255 < 2^32); a call beyond that is refused before anything is read.
 * hesaff_train_vocabulary_device: descriptors in device memory, addressed as in hesaff_assign_words_device (stride 164, offset 36: a
 * hesaff_keypoint array; stride 128, offset 0: a packed tensor).  init: K x 128 host bytes or NULL; words_out: K x 128 host bytes;
 * distortion: int64_t[iterations], empty: int32_t[iterations], iterations_done: each may be NULL.
 * hesaff_train_vocabulary: the same for desc[n][128] in host memory.
 * Training neither reads nor changes the context's own vocabulary (it works on a private one, in device memory it allocates for the
 * call and releases before it returns); a caller installs the result with hesaff_set_vocabulary.
 * hesaff_stage_accumulate_words: the accumulation kernels alone - words[n] are the caller's words in 0 .. k - 1, sums_out is
 * uint32_t[k][128], counts_out uint32_t[k].
 * hesaff_get_training_ms: the HIP-event times of the last training call at profiling level >= 1, summed over its iterations:
 * assignment, accumulation (grouping the keys by word and summing), update.  0 otherwise.
 * HESAFF_ERR_ARG, nothing changed, the context usable as before: ctx NULL; the descriptors or words_out NULL; n < 1 or n > 2^24;
 * k < 1 or k > 2^20; iterations < 1; init NULL with n < k; stride, offset or the device pointer outside the rules of
 * hesaff_assign_words_device; in the stage operator a NULL array or a word outside 0 .. k - 1 (checked on the host); a getter's out
 * pointer NULL.  HESAFF_ERR_NOMEM: the device cannot hold the working arrays (n = 2^24, K = 2^20: about 1 GB beside the descriptors). */
int hesaff_train_vocabulary_device(hesaff_ctx *ctx, int64_t n, const void *d_desc, int64_t stride, int64_t offset, int k, const uint8_t *init,
                                   int iterations, uint8_t *words_out, int64_t *distortion, int32_t *empty, int *iterations_done);
int hesaff_train_vocabulary(hesaff_ctx *ctx, int64_t n, const uint8_t *desc, int k, const uint8_t *init, int iterations, uint8_t *words_out,
                            int64_t *distortion, int32_t *empty, int *iterations_done);
int hesaff_stage_accumulate_words(hesaff_ctx *ctx, int n, const uint8_t *desc, const int32_t *words, int k, uint32_t *sums_out, uint32_t *counts_out);
int hesaff_get_training_ms(const hesaff_ctx *ctx, float *assign_ms, float *accumulate_ms, float *update_ms);

/* Vocabulary cells (no counterpart in the reference): a coarse layer over a set vocabulary, so that a key is compared with C coarse
 * rows and then only with the rows of one cell - C + K / C exact distances instead of K.  Symbols only, version 8.
 * A cell layer over a vocabulary of K rows is C coarse rows g_c of 128 bytes, 1 <= C <= K, and first[0 .. C] with first[0] = 0,
 * first[C] = K, strictly increasing: cell c owns rows first[c] .. first[c + 1] - 1, and no cell is empty.  For a key with bytes d, dist2
 * being hesaff_set_vocabulary's:
 *     cell     = the LOWEST c of least dist2(d, g_c)
 *     word     = the LOWEST k in [first[cell], first[cell + 1]) of least dist2(d, w_k)
 *     dist2    = dist2(d, w_word)
 * Integers, exact, ties decided, no dependence on launch geometry.  With C = 1 this is the flat assignment; a row outside the key's
 * cell never wins, however near it is.
 * hesaff_set_vocabulary_cells: coarse[c][128] and first[c + 1], copied to the device; a vocabulary must be set first; c = 0 (the arrays
 * may be NULL) removes the layer, and so does every hesaff_set_vocabulary call (first[C] = K no longer describes the new rows).  With
 * a layer set, every entry point that assigns words uses it - the detecting and describing calls, hesaff_assign_words_device,
 * hesaff_stage_assign_words, hesaff_process_files - and the outputs keep their layout.  Without one nothing is launched, allocated or
 * copied for it.  The working arrays (12 bytes per key of the largest call so far, at most 2^24 keys: longer sources run in slices;
 * and arrays of size C) belong to the context, are allocated by the first assignment through a layer and only grow.
 * hesaff_get_vocabulary_cells: *c = C, 0 without a layer.
 * hesaff_get_assign_cells_ms: hesaff_get_assign_ms of the last assignment through a layer, split into the coarse assignment, the
 * grouping of the keys by cell and the assignment inside the cells (profiling level >= 1; 0 otherwise).
 * HESAFF_ERR_ARG, the previous layer stays set and the context usable as before: ctx NULL; no vocabulary set; c < 0 or c > K; an array
 * NULL with c > 0; first[0] != 0, first[c] != K, or first not strictly increasing; a getter's out pointer NULL.
 * hesaff_build_vocabulary_cells: a layer for any k rows (1 <= k <= 2^20) given c coarse rows (1 <= c <= k).  Every row is assigned to
 * its nearest coarse row (the lowest of least dist2, on the device, against a private copy of `coarse`: the context's vocabulary is
 * neither read nor changed), the rows are sorted by cell (stable, on the host), cells that received no row are dropped and their
 * coarse rows compacted in order.  words_out[k][128]: the rows in the new order; order_out[new] = old row; coarse_out[c][128] and
 * first_out[c + 1]: room for c cells, *c_out of them filled.  Deterministic.  HESAFF_ERR_ARG: a pointer NULL, k or c outside the bounds.
 * hesaff_train_vocabulary_cells_device / hesaff_train_vocabulary_cells: hesaff_train_vocabulary[_device] on the K rows of a layer with
 * the coarse rows and `first` fixed: the assignment of every iteration is the one above under V_{t-1}; the accumulation, the update, its
 * rounding, the rule for empty words and the stop at a fixed point are training's.  `init` (the K rows, in the layer's order) is
 * required.  A key's cell does not change during a call, so distortion[t] <= distortion[t - 1].  Bounds, outputs and errors are
 * hesaff_train_vocabulary's, and HESAFF_ERR_ARG also answers init or coarse NULL and a `first` that is no layer over k rows.
 * Cells file, kept beside the vocabulary file of the same rows (which stays an ordinary flat vocabulary).  Little-endian:
 *   char magic[8] = "HESAFFC1"; uint32 dim = 128; uint32 cells; uint32 rows; uint32 reserved = 0; cells x uint8[128]; (cells + 1) x uint32
 * hesaff_write_vocabulary_cells: rows = first[c]; HESAFF_ERR_ARG for a `first` that breaks the rules above.
 * hesaff_read_vocabulary_cells: *coarse and *first are malloc'ed (hesaff_free each); HESAFF_ERR_IO for a file that cannot be read or is
 * not a whole cells file (magic, dim, reserved, cells outside 1 .. rows, rows beyond 2^20, size, or a `first` that breaks the rules). */
int hesaff_set_vocabulary_cells(hesaff_ctx *ctx, int c, const uint8_t *coarse, const uint32_t *first);
int hesaff_get_vocabulary_cells(const hesaff_ctx *ctx, int *c);
int hesaff_get_assign_cells_ms(const hesaff_ctx *ctx, float *coarse_ms, float *group_ms, float *fine_ms);
int hesaff_build_vocabulary_cells(hesaff_ctx *ctx, int k, const uint8_t *words, int c, const uint8_t *coarse, uint8_t *words_out, int32_t *order_out,
                                  uint8_t *coarse_out, uint32_t *first_out, int *c_out);
int hesaff_train_vocabulary_cells_device(hesaff_ctx *ctx, int64_t n, const void *d_desc, int64_t stride, int64_t offset, int k, const uint8_t *init, int c,
                                         const uint8_t *coarse, const uint32_t *first, int iterations, uint8_t *words_out, int64_t *distortion,
                                         int32_t *empty, int *iterations_done);
int hesaff_train_vocabulary_cells(hesaff_ctx *ctx, int64_t n, const uint8_t *desc, int k, const uint8_t *init, int c, const uint8_t *coarse,
                                  const uint32_t *first, int iterations, uint8_t *words_out, int64_t *distortion, int32_t *empty, int *iterations_done);
int hesaff_read_vocabulary_cells(const char *path, uint8_t **coarse, uint32_t **first, int *c, int *rows);
int hesaff_write_vocabulary_cells(const char *path, int c, const uint8_t *coarse, const uint32_t *first);

/* Vocabulary probes (no counterpart in the reference; FAISS nprobe, FLANN checks): with a cell layer set, a key is searched in its P
 * nearest cells, not in one - the dial between one cell and the flat search.  Symbols only, version 8.
 * With the layer's C coarse rows g_c and first[0 .. C], a probe count P and P' = min(P, C), for a key with bytes d:
 *     probe[0 .. P'-1] = the first P' cells in the order (dist2(d, g_c) ascending, c ascending)
 *     word             = the k of least (dist2(d, w_k), k), lexicographically, over the rows k of the cells probe[0 .. P'-1]
 *     dist2            = dist2(d, w_word)
 * Integers, exact, ties decided, no dependence on launch geometry.  P = 1 is the definition of hesaff_set_vocabulary_cells; P' = C is
 * the flat word and dist2 of hesaff_set_vocabulary exactly; a key's dist2 never increases with P; a row of a cell that is not probed
 * never wins; a tie between rows of two probed cells goes to the lower row, whatever the ranks of their cells; equal coarse rows are
 * probed in ascending c.
 * hesaff_set_vocabulary_probes: 1 <= probes <= 8, default 1.  A setting of the context like the orientation count: it survives
 * hesaff_set_vocabulary and hesaff_set_vocabulary_cells, and has no effect while no layer is set (the flat search is exact already).
 * With a layer set and P > 1 every entry point that assigns words uses the probes - the detecting and describing calls,
 * hesaff_assign_words_device, hesaff_stage_assign_words, hesaff_process_files - and the outputs keep their layout.  The working arrays
 * grow to 20 P' bytes per key, a slice to floor(2^24 / P') keys.  With P' = 1 the kernels, their order and the 12 bytes per key are
 * those of a context on which this was never called.  hesaff_get_assign_cells_ms then reports the search for the P' cells, the grouping
 * of the n P' (key, rank) entries by cell, and the search inside the cells with the merge of a key's P' results.
 * hesaff_build_vocabulary_cells and hesaff_train_vocabulary_cells[_device] do not read the setting: training assigns through its
 * private layer with one probe.
 * hesaff_get_vocabulary_probes: *probes = P.
 * hesaff_stage_probe_cells: the first step alone, for desc[n][128] in host memory with the context's layer and probe count:
 * cells_out[n][P'] and dist2_out[n][P'] (the distance to the coarse row), in probe order.
 * HESAFF_ERR_ARG, with the setting as it was: ctx NULL, probes outside 1..8, a getter's out pointer NULL; hesaff_stage_probe_cells: a
 * pointer NULL with n > 0, n < 0, n P' > 2^24, no layer set. */
int hesaff_set_vocabulary_probes(hesaff_ctx *ctx, int probes);
int hesaff_get_vocabulary_probes(const hesaff_ctx *ctx, int *probes);
int hesaff_stage_probe_cells(hesaff_ctx *ctx, int n, const uint8_t *desc, int32_t *cells_out, int32_t *dist2_out);

/* Vocabulary neighbours (no counterpart in the reference; multiple assignment, Jegou, Douze and Schmid IJCV 2010; related to the soft
 * assignment of Philbin et al. CVPR 2008): the R nearest rows of the vocabulary per key, not just the nearest, so that a QUERY key
 * can be looked up under every word whose cell border it lies near.  The database and the index do not change.  Symbols only,
 * version 8.
 * With a vocabulary of K rows set, the neighbours of a key are the R lexicographically least pairs (dist2(k), k) over the rows
 * k = 0 .. K - 1, in ascending order; dist2 as in hesaff_set_vocabulary.  Integers, exact, ties decided (a tie in dist2 goes to the
 * lower row, also where it decides which row is the R-th), no dependence on launch geometry.  Rank 0 is hesaff_set_vocabulary's
 * (word, dist2) of the key, bit for bit.  Where K < R, the ranks r >= K are (-1, 2^31 - 1).  All rows of a key's list are distinct.
 * On the device one pass over the vocabulary keeps R candidates per key (k_assign_neighbours, kernels_neighbours.h).
 * hesaff_set_vocabulary_neighbours: 1 <= R <= 8, default 1.  A setting of the context like the probe count: it survives
 * hesaff_set_vocabulary.  With R > 1 every entry point that assigns words - the detecting and describing calls,
 * hesaff_assign_words_device, hesaff_stage_assign_words, hesaff_process_files - also leaves int32[n][R][2] neighbours, (word, dist2)
 * per rank, beside the words; the (word, dist2) arrays those entry points hand out keep their layout and their bytes: they are rank 0.
 * With R = 1 the kernels, their order, the allocations and the copies are those of a context on which this was never called; the
 * neighbours array costs 8 R bytes per key and exists only while R > 1.
 * R > 1 and a cell layer do not combine: hesaff_set_vocabulary_cells (cells > 0) with R > 1 set, and this call with R > 1 while a
 * layer is set, return HESAFF_ERR_ARG with a message that says so and leave the context as it was.
 * hesaff_get_neighbours: as hesaff_get_words (the image index, the lifetime, the _cb forms); *neighbours = int32_t[count][*r][2], row
 * for row that image's keys.  hesaff_get_neighbours_device: the device array the last assignment left - parallel to d_keys_out after
 * a device-resident call, to the descriptors after hesaff_assign_words_device or hesaff_stage_assign_words; not after a host call
 * (its rows are in host memory: hesaff_get_neighbours).  *r is the count the rows were written with.  With R = 1 both getters hand
 * out the words themselves, which are [count][1][2].  Changing R leaves the words readable; the neighbours are the next call's.
 * hesaff_assign_neighbours_device / hesaff_stage_assign_neighbours: the neighbours of n caller-held descriptors, addressed and aligned
 * as in hesaff_assign_words_device / in host memory; the output receives n x R x 2 int32 with the context's R, R = 1 as well.  They
 * search the whole vocabulary, whatever layer is set.  hesaff_get_assign_ms reports their launch, and with R > 1 that of the entry
 * points above: the neighbours launch takes the assignment's place, it does not follow it.
 * With an embedding set a (key, rank) pair has a signature of its own, bit i = z[i] > tau[word_r][i]: hesaff_embed_device with
 * d_words = the neighbours + 2 r and word_stride = 2 R, for a rank that every key has (r < K).
 * HESAFF_OUT_WORDS in hesaff_process_files with R > 1: <image>.hesaff.words holds, for every key in key order, one row per present
 * rank in ascending rank - the five floats of the key, the word of the rank - and <image>.hesaff.sigs is row for row with it; ranks
 * absent because K < R are not written.  Such a file is an ordinary words file with up to R rows per key.
 * HESAFF_ERR_ARG, with the setting and the last results as they were: ctx NULL, R outside 1..8, a getter's out pointer NULL, no
 * vocabulary set (getters and operators), `image` outside the last host call's images, the addressing rules of
 * hesaff_assign_words_device, n < 0. */
int hesaff_set_vocabulary_neighbours(hesaff_ctx *ctx, int neighbours);
int hesaff_get_vocabulary_neighbours(const hesaff_ctx *ctx, int *neighbours);
int hesaff_get_neighbours(const hesaff_ctx *ctx, int image, const int32_t **neighbours, int *count, int *r);
int hesaff_get_neighbours_device(const hesaff_ctx *ctx, const void **d_neighbours, int64_t *total, int *r);
int hesaff_assign_neighbours_device(hesaff_ctx *ctx, int64_t n, const void *d_desc, int64_t stride, int64_t offset, void *d_neighbours_out);
int hesaff_stage_assign_neighbours(hesaff_ctx *ctx, int n, const uint8_t *desc, int32_t *neighbours_out);

/* Image index (no counterpart in the reference): an inverted file over visual words with tf-idf scoring, the consumer of the words
 * that hesaff_set_vocabulary assigns.  Symbols only, version 8.
 * An index is built in one call from N images, 1 <= N <= 2^20; image i has counts[i] words, 0 <= counts[i] <= 2^18, each in
 * 0 .. K - 1, 1 <= K <= 2^20; the total number of keys is T <= 2^28.  K is an argument of the call, not the context's vocabulary:
 * the words may come from files.  All integers:
 *     tf(i, w)  = number of keys of image i with word w
 *     df(w)     = #{i : tf(i, w) > 0}
 *     idf(w)    = 0 where df(w) = 0, otherwise ilog2_q8 of N and df(w):
 *                    q = (N << 31) / df                  uint64, floor;  2^31 <= q < 2^55
 *                    e = (index of q's highest set bit) - 31;   m = q >> e        2^31 <= m < 2^32
 *                    r = e
 *                    8 times:  m = (m * m) >> 31;  r = 2 r;  if m >= 2^32 { r += 1; m >>= 1 }
 *                    idf = r          (floor(256 log2(N / df)) but for the truncations; 0 when df = N; at most 6143)
 *     norm2(i)  = sum_w (tf(i, w) * idf(w))^2            uint64
 * The definition is this algorithm, not the logarithm.  A query is n words, 0 <= n <= 2^18, each in 0 .. K - 1, tfq(w) their counts:
 *     nq2      = sum_w (tfq(w) * idf(w))^2                                  uint64
 *     dot(i)   = sum_w tfq(w) * tf(i, w) * idf(w)^2                         uint64
 *     score(i) = 0.0 where dot(i) = 0, otherwise
 *                (double)dot(i) / sqrt((double)nq2 * (double)norm2(i))      conversions round to nearest even; *, sqrt, / are IEEE binary64
 *     result   = the first min(top, N) images in the order (score descending, image index ascending), with their scores; 1 <= top <= 1024
 * Every sum stays inside uint64: idf^2 < 2^26, sum_w tfq * tf <= 2^18 * 2^18 and sum_w tf^2 <= 2^36, so dot, nq2 and norm2 are each
 * below 2^62.  The definition is total: images without keys, and images that share no weighted word with the query, score 0 and
 * rank among themselves by index; an empty query returns images 0, 1, .. with score 0; equal images tie, the lower index first.
 * Integer accumulation throughout: no result depends on launch geometry or on the order of atomics (kernels_index.h).
 * The words of all images are concatenated, image after image; key j's word is words[j * word_stride], word_stride = 1 for a packed
 * array, 2 for the (word, dist2) rows that hesaff_get_words and hesaff_get_words_device hand out.  counts is host memory in both
 * forms.  The host forms check the words while staging them; the device forms run a read-only check kernel first.
 * A successful build replaces the previous index.  The index is context state, like the vocabulary: it survives detecting calls,
 * and without one nothing is launched, allocated or copied anywhere.  The build's scratch (a hash table of at least 2 T slots, 12
 * bytes each) is released before the call returns.
 * hesaff_index_get_scores: dot and score of EVERY image, and nq2, of the last query (zeros before the first); each may be NULL.
 * hesaff_index_get_tables: df[K], idf[K], norm2[N]; each may be NULL.  hesaff_index_get_info: each may be NULL.
 * hesaff_get_index_ms: HIP-event times of the last build and the last query at profiling level >= 1, 0 otherwise.
 * hesaff_read_words: the word column of a words file ("HESAFFW1"); *words is malloc'ed (hesaff_free; NULL when count is 0);
 * HESAFF_ERR_IO for a file that cannot be read or is not a whole words file (magic, a size other than 16 + 24 count).
 * HESAFF_ERR_ARG, nothing changed, the context usable as before: ctx NULL; a required pointer NULL; a count outside the bounds above;
 * word_stride not 1 or 2; a device pointer that is not 4-byte aligned; a word outside 0 .. K - 1; top outside 1..1024; a query, a
 * getter or hesaff_index_get_info with no index built (hesaff_index_clear succeeds without one).
 * HESAFF_ERR_NOMEM: the device cannot hold the index or the build's scratch; a previous index then stays. */
int hesaff_index_build(hesaff_ctx *ctx, int n_images, const int32_t *counts, const int32_t *words, int word_stride, int vocabulary_size);
int hesaff_index_build_device(hesaff_ctx *ctx, int n_images, const int32_t *counts, const void *d_words, int word_stride, int vocabulary_size);
int hesaff_index_query(hesaff_ctx *ctx, int n, const int32_t *words, int word_stride, int top, int32_t *images_out, double *scores_out,
                       int *count_out);
int hesaff_index_query_device(hesaff_ctx *ctx, int n, const void *d_words, int word_stride, int top, int32_t *images_out, double *scores_out,
                              int *count_out);
int hesaff_index_get_scores(const hesaff_ctx *ctx, uint64_t *dots, double *scores, uint64_t *query_norm2);
int hesaff_index_get_tables(const hesaff_ctx *ctx, uint32_t *df, uint32_t *idf, uint64_t *norm2);
int hesaff_index_get_info(const hesaff_ctx *ctx, int *n_images, int *vocabulary_size, int64_t *n_keys, int64_t *n_postings);
int hesaff_index_clear(hesaff_ctx *ctx);
int hesaff_get_index_ms(const hesaff_ctx *ctx, float *build_ms, float *query_ms);
int hesaff_read_words(const char *path, int32_t **words, int *count, int *vocabulary_size);

/* Hamming embedding (no counterpart in the reference; Jegou, Douze, Schmid, ECCV 2008): a 64-bit signature per key places the key
 * inside its word's cell, and a word match counts only where the two signatures are within a Hamming threshold.  Symbols only,
 * version 8.  All arithmetic is integer, and every result is exact to the bit.
 * Projection.  P[64][128] is signed bytes, every entry in -127 .. 127 (an entry of -128 is HESAFF_ERR_ARG).  For the descriptor bytes
 * d[0..127] (unsigned) of a key:  z[i] = sum_j P[i][j] * d[j],  |z[i]| <= 128 * 127 * 255 = 4 145 280 < 2^22.
 * hesaff_embedding_projection(seed, P): the default projection, pure host code.  Entry e = i * 128 + j, e = 0, 1, .., is the e-th
 * output of splitmix64 from s = seed (uint64 arithmetic):
 *     s += 0x9E3779B97F4A7C15;  x = s;  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9;  x = (x ^ (x >> 27)) * 0x94D049BB133111EB;  x ^= x >> 31;
 *     v = (int)(x >> 56) - 128, and -128 becomes -127.
 * Signature of a key with word w: bit i (bit 0 the least significant) of a uint64 is  z[i] > tau[w][i],  strictly greater; tau is
 * int32[K][64], any values, K the rows of the vocabulary that is set.
 * hesaff_set_embedding(ctx, P, tau): needs a vocabulary; both are copied.  NULL, NULL removes the embedding.  hesaff_set_vocabulary
 * removes it as it removes the cells; hesaff_set_vocabulary_cells and hesaff_set_vocabulary_probes leave it (the word alone selects
 * the thresholds, however it was found).  With an embedding set, every call that assigns words also makes the signatures, behind
 * the words: hesaff_get_signatures hands out those of one image of the last host call, row for row with hesaff_get_words and with
 * its lifetime; hesaff_get_signatures_device those of the last device-resident call, parallel to hesaff_get_words_device (8-byte
 * aligned device memory of the context, valid until its next call); hesaff_process_files with HESAFF_OUT_WORDS writes a signatures
 * file beside every words file - its name with ".sigs" in the place of the final ".words", or appended where there is none - and
 * hesaff_set_resume counts it as part of the output.  Without an embedding nothing is launched, allocated, copied or written, and
 * keys, words and words files are those of a context that never had one.  hesaff_get_embedding: *k = the rows of tau (0: none set);
 * P[64][128] and tau[k][64] are filled where not NULL.
 * hesaff_embed_device: n descriptors in device memory (descriptor i at d_desc + i * stride + offset, hesaff_assign_words_device's
 * rules), key i's word the int32 at d_words + 4 i word_stride (word_stride 1 or 2) -> n uint64 at d_sigs_out (8-byte aligned).
 * hesaff_stage_embed: the same on host arrays.  hesaff_stage_project: z[n][64] = P . d of the caller's descriptors under the
 * caller's P, by the kernel that makes the signatures; needs neither vocabulary nor embedding.
 * Thresholds by training.  hesaff_train_embedding(ctx, n, desc, words, word_stride, k, P, tau_out, counts_out), 1 <= n <= 2^24,
 * 1 <= k <= 2^20, every word in 0 .. k - 1: with m_w the number of keys of word w, tau_out[w][i] is the LOWER MEDIAN of that word's
 * z[i] - element (m_w - 1) / 2 of the values sorted ascending - or 0 for every i where m_w = 0, and counts_out[w] = m_w (may be NULL).
 * Nothing depends on the order of arrival or the launch geometry: two calls give the same bytes.  The context's own embedding and
 * vocabulary are neither read nor written; the working set (256 bytes per key for z, 256 per word) is released before the call returns.
 * hesaff_train_embedding_device: the same on descriptors and words in device memory.
 * hesaff_get_embedding_ms: HIP-event times at profiling level >= 1, 0 otherwise: of the last signature launch (a batch's, or
 * hesaff_embed_device's), and of the last training's projection, grouping and median steps.
 * Embedded index.  hesaff_index_build_embedded takes a signature per key beside hesaff_index_build's words (sigs[j] belongs to key
 * j; always packed).  It produces exactly the plain index's df, idf, offsets, postings and norm2, bit for bit, and word-major key
 * lists of (image, signature); the order of the entries inside a list is unspecified, only sums over a list are output.  A plain
 * hesaff_index_query on an embedded index answers as on a plain one.  hesaff_index_query_embedded with threshold T, 0 <= T <= 64:
 *     dot_T(i) = sum over every query key q and every key j of image i with word_j = word_q and popcount(sig_q ^ sig_j) <= T
 *                of idf(word_q)^2                                                          uint64
 *     nq2 and norm2(i) are the plain index's; score(i) = 0.0 where dot_T(i) = 0, otherwise
 *                (double)dot_T(i) / sqrt((double)nq2 * (double)norm2(i)), the plain query's three binary64 operations;
 *     ranking and ties as the plain query.
 * So T = 64 is the plain query bit for bit (dot, nq2, scores, ranking), and dot_T(i) never decreases with T.  The bounds are the plain
 * index's: dot_T <= dot < 2^62.  hesaff_index_get_scores is valid after it.  hesaff_index_get_embedded: *embedded = 1 where the index
 * that is built holds key lists; then offsets[K + 1], and per list entry its image and its signature (images[T], sigs[T]; each may
 * be NULL; on a plain index all three must be NULL).
 * Files, little-endian.  Embedding, kept beside the vocabulary file of the same k rows:
 *     char magic[8] = "HESAFFE1"; uint32 bits = 64, dim = 128, k, reserved = 0; int8 P[64][128]; int32 tau[k][64]
 * Signatures of an image, row for row with its words file:
 *     char magic[8] = "HESAFFS1"; uint32 bits = 64; uint32 count; count x uint64
 * The readers return malloc'ed arrays (hesaff_free; *sigs NULL where count is 0) and HESAFF_ERR_IO for anything that cannot be
 * read or is not a whole file of the format (magic, bits, dim, k outside 1 .. 2^20, reserved, size against count, a P entry of -128).
 * hesaff_signatures_is_complete: the O(1) test of hesaff_set_resume - the rows of a whole signatures file, or -1.
 * HESAFF_ERR_ARG, nothing changed, the context usable as before: ctx or a required pointer NULL (P and tau not both NULL or both set);
 * no vocabulary, or no embedding, where one is needed; a P entry of -128; T outside 0 .. 64; an embedded query on a plain index, or
 * with no index; a word outside 0 .. K - 1; a count outside the bounds; word_stride not 1 or 2; a descriptor or word pointer in
 * device memory that is not 4-byte aligned, a signature pointer that is not 8-byte aligned.
 * HESAFF_ERR_NOMEM: the device cannot hold the arrays; the previous embedding, or the previous index, then stays. */
#define HESAFF_EMBED_BITS 64
int hesaff_embedding_projection(uint64_t seed, int8_t *P);
int hesaff_set_embedding(hesaff_ctx *ctx, const int8_t *P, const int32_t *tau);
int hesaff_get_embedding(const hesaff_ctx *ctx, int *k, int8_t *P, int32_t *tau);
int hesaff_get_signatures(const hesaff_ctx *ctx, int image, const uint64_t **sigs, int *count);
int hesaff_get_signatures_device(const hesaff_ctx *ctx, const void **d_sigs, int64_t *total);
int hesaff_embed_device(hesaff_ctx *ctx, int64_t n, const void *d_desc, int64_t stride, int64_t offset, const void *d_words, int word_stride,
                        void *d_sigs_out);
int hesaff_stage_embed(hesaff_ctx *ctx, int n, const uint8_t *desc, const int32_t *words, int word_stride, uint64_t *sigs_out);
int hesaff_stage_project(hesaff_ctx *ctx, int n, const uint8_t *desc, const int8_t *P, int32_t *z_out);
int hesaff_train_embedding(hesaff_ctx *ctx, int64_t n, const uint8_t *desc, const int32_t *words, int word_stride, int k, const int8_t *P,
                           int32_t *tau_out, uint32_t *counts_out);
int hesaff_train_embedding_device(hesaff_ctx *ctx, int64_t n, const void *d_desc, int64_t stride, int64_t offset, const void *d_words,
                                  int word_stride, int k, const int8_t *P, int32_t *tau_out, uint32_t *counts_out);
int hesaff_get_embedding_ms(const hesaff_ctx *ctx, float *embed_ms, float *project_ms, float *group_ms, float *median_ms);
int hesaff_index_build_embedded(hesaff_ctx *ctx, int n_images, const int32_t *counts, const int32_t *words, int word_stride,
                                const uint64_t *sigs, int vocabulary_size);
int hesaff_index_build_embedded_device(hesaff_ctx *ctx, int n_images, const int32_t *counts, const void *d_words, int word_stride,
                                       const void *d_sigs, int vocabulary_size);
int hesaff_index_query_embedded(hesaff_ctx *ctx, int n, const int32_t *words, int word_stride, const uint64_t *sigs, int hamming, int top,
                                int32_t *images_out, double *scores_out, int *count_out);
int hesaff_index_query_embedded_device(hesaff_ctx *ctx, int n, const void *d_words, int word_stride, const void *d_sigs, int hamming, int top,
                                       int32_t *images_out, double *scores_out, int *count_out);
int hesaff_index_get_embedded(const hesaff_ctx *ctx, int *embedded, uint32_t *offsets, uint32_t *images, uint64_t *sigs);
int hesaff_write_embedding(const char *path, int k, const int8_t *P, const int32_t *tau);
int hesaff_read_embedding(const char *path, int8_t **P, int32_t **tau, int *k);
int hesaff_write_signatures(const char *path, const uint64_t *sigs, int n);
int hesaff_read_signatures(const char *path, uint64_t **sigs, int *count);
int hesaff_signatures_is_complete(const char *path);

/* The index as a durable, growing object (no counterpart in the reference).  Symbols only, version 8.
 * hesaff_index_add(ctx, m, counts, words, word_stride): appends m images, 1 <= m, to the context's index of N images over K words;
 * image j of the call has counts[j] words, 0 <= counts[j] <= 2^18, each in 0 .. K - 1, laid out as hesaff_index_build's.  The new
 * images take the numbers N .. N + m - 1 in the order given, and the index that results IS the index hesaff_index_build would make
 * of the old images followed by the new ones: df, idf = ilog2_q8(N + m, df), the offsets and norm2 are equal bit for bit - the idf
 * of every word changes with N, and with it the norm2 of every old image, which is summed again on the device - and every word's
 * posting list is equal as a multiset (a build defines no order inside a list either).  Queries and hesaff_index_get_scores after
 * an add are therefore bit for bit those of the rebuilt index; the last query's dot and score read zero after an add, as after a
 * build.  hesaff_index_add_embedded takes a signature per key and extends an embedded index, whose key lists are likewise equal as
 * multisets to the rebuilt index's, so embedded queries at every T are too.  The _device forms read words (and signatures) in
 * device memory.  An add works on a new index and installs it when it is whole: its peak is the old index, the new one and a hash
 * table sized for the NEW keys alone.
 * HESAFF_ERR_ARG, with the context's index, vocabulary and embedding byte for byte what they were: no index is built; m < 1 or
 * N + m > 2^20; a count outside 0 .. 2^18; the index's keys and the new ones together above 2^28; a word outside 0 .. K - 1 (found
 * before anything is built); word_stride not 1 or 2; hesaff_index_add on an embedded index, or hesaff_index_add_embedded on a plain
 * one; ctx or a required pointer NULL; a word pointer in device memory that is not 4-byte aligned, a signature pointer that is not
 * 8-byte aligned.  HESAFF_ERR_NOMEM: the device cannot hold the new index beside the old; the old one stays.
 * hesaff_index_get_postings: offsets[K + 1] and, per posting in word-major order, its image and its tf (images[n_postings],
 * tf[n_postings]; each may be NULL; the order inside a list is unspecified) - the plain counterpart of hesaff_index_get_embedded.
 * hesaff_index_save(ctx, path) writes the context's index, hesaff_index_load(ctx, path) replaces it by a file's.  The file, little-
 * endian, every array on a multiple of 8 bytes (4 bytes of zero behind an array of an odd number of uint32):
 *     char magic[8] = "HESAFFI1"; uint32 flags (bit 0: embedded), k, n_images, reserved = 0; uint64 n_keys, n_postings;
 *     uint32 df[k]; { uint32 image, tf } postings[n_postings], word-major: df[0] of word 0, df[1] of word 1, ..;
 *     an embedded index only: uint32 key_count[k]; uint32 key_image[n_keys]; uint64 key_sig[n_keys], word-major by key_count
 * Only what cannot be derived is kept: idf, both offset tables and norm2 are made again on load.  The entries of a list are in the
 * index's current order: two saves of equal indexes may differ as files and are equal as multisets.
 * hesaff_write_index_file / hesaff_read_index_file are the writer and the reader over host arrays, pure host code; postings is
 * uint32[n_postings][2] = (image, tf); the three key arrays are NULL for a plain index; the reader returns malloc'ed arrays
 * (hesaff_free; NULL where an array has no entry or the file is plain).  The reader returns HESAFF_ERR_IO for anything that cannot
 * be read or is not a whole file of the format: a short or long file, wrong magic, unknown flags, reserved not 0, k or n_images
 * outside 1 .. 2^20, n_keys > 2^28, n_postings > n_keys, sum(df) != n_postings, a df > n_images, sum(key_count) != n_keys; the
 * writer returns HESAFF_ERR_ARG for the same.  hesaff_index_load returns the reader's code for these, and then checks the lists
 * on the device in the pass that sums norm2: every posting's image < n_images and 1 <= tf <= 2^18; every image's tf sum <= 2^18;
 * the tf of all postings == n_keys; in an embedded file every word's key count == the tf of its postings and every key's
 * image < n_images.  A file that fails one returns HESAFF_ERR_ARG, hesaff_last_error names the first rule violated in this order,
 * and the context's index is untouched.  That an (image, word) pair occurs once per list is NOT checked: a file with a pair twice
 * loads, and scores as if the image held the word's postings added up, but for norm2, which sums their squares one by one.
 * A loaded index answers every query, embedded query and add bit for bit like the index that was saved.
 * hesaff_get_index_growth_ms: HIP-event times at profiling level >= 1, 0 otherwise: of the last add its hash step, its tables (df,
 * idf, offsets), the merge of the old postings and the scatter of the new ones; of the last load its device pass. */
int hesaff_index_add(hesaff_ctx *ctx, int m_images, const int32_t *counts, const int32_t *words, int word_stride);
int hesaff_index_add_device(hesaff_ctx *ctx, int m_images, const int32_t *counts, const void *d_words, int word_stride);
int hesaff_index_add_embedded(hesaff_ctx *ctx, int m_images, const int32_t *counts, const int32_t *words, int word_stride, const uint64_t *sigs);
int hesaff_index_add_embedded_device(hesaff_ctx *ctx, int m_images, const int32_t *counts, const void *d_words, int word_stride, const void *d_sigs);
int hesaff_index_get_postings(const hesaff_ctx *ctx, uint32_t *offsets, uint32_t *images, uint32_t *tf);
int hesaff_index_save(hesaff_ctx *ctx, const char *path);
int hesaff_index_load(hesaff_ctx *ctx, const char *path);
int hesaff_get_index_growth_ms(const hesaff_ctx *ctx, float *insert_ms, float *tables_ms, float *merge_ms, float *scatter_ms, float *load_ms);
int hesaff_write_index_file(const char *path, int embedded, int vocabulary_size, int n_images, int64_t n_keys, int64_t n_postings, const uint32_t *df,
                            const uint32_t *postings, const uint32_t *key_count, const uint32_t *key_image, const uint64_t *key_sig);
int hesaff_read_index_file(const char *path, int *embedded, int *vocabulary_size, int *n_images, int64_t *n_keys, int64_t *n_postings, uint32_t **df,
                           uint32_t **postings, uint32_t **key_count, uint32_t **key_image, uint64_t **key_sig);

/* Removal from the index (no counterpart in the reference).  Symbols only, version 8.
 * hesaff_index_remove(ctx, m, images, remap_out): images[m] are m distinct image numbers, in any order, 1 <= m <= N - 1, of the
 * context's index of N images over K words (host memory; an index always holds at least one image - emptying it is
 * hesaff_index_clear).  The images that stay keep their order and are renumbered densely: old image i becomes i - #{removed numbers
 * below i}.  remap_out, where not NULL, receives int32[N]: the new number of every old image, -1 for a removed one; it is written
 * only on success.  The index that results IS the index hesaff_index_build (hesaff_index_build_embedded for an embedded index, with
 * the signatures the keys had) would make of the remaining images in that order: df, idf = ilog2_q8(N - m, df), the offsets and
 * norm2 are equal bit for bit - the idf of every word changes with N, and with it the norm2 of every image that stays, which is
 * summed again on the device - n_keys and n_postings are the rebuild's, and every posting list, and every key list of an embedded
 * index, is equal as a multiset (no order inside a list is defined).  So a word whose last posting goes gets df 0 and idf 0, a word
 * every remaining image holds gets idf 0, and a removed image without keys only renumbers and changes N.  Every query, embedded
 * query at every T, batched query, add, save and load afterwards is bit for bit the rebuilt index's; the last query's dot and score
 * read zero after a removal, as after a build or an add, and the batch scratch is released, as by an add.  "Replace image i" is a
 * removal followed by an add.  A removal works on a new index and installs it when it is whole: its peak is the old index, the new
 * one and a scratch of O(N + K) words, no hash table (index_remove_working_set_bytes, index_remove_plan.h: beside the old index at
 * most 2.05 GiB for a plain index of N = K = 2^20 and 2^28 postings, 5.07 GiB for an embedded one of 2^28 keys).
 * HESAFF_ERR_ARG, with the context's index, vocabulary and embedding byte for byte what they were and remap_out untouched: no index
 * is built; ctx or images NULL; m < 1 or m >= N; a number outside 0 .. N - 1; a number given twice (hesaff_last_error names the
 * number).  HESAFF_ERR_NOMEM: the device cannot hold the new index beside the old; the old one stays.
 * hesaff_get_index_remove_ms: HIP-event times of the last removal at profiling level >= 1, 0 otherwise: its counting pass, its
 * tables (idf and the scans), the compaction of the postings, and the key lists (0 for a plain index). */
int hesaff_index_remove(hesaff_ctx *ctx, int m_images, const int32_t *images, int32_t *remap_out);
int hesaff_get_index_remove_ms(const hesaff_ctx *ctx, float *count_ms, float *tables_ms, float *compact_ms, float *keys_ms);

/* Batched index queries: many queries per call, ranked on the device.  Symbols only, version 8.
 * A batch is Q queries, 1 <= Q <= 2^16.  Query q has counts[q] words, 0 <= counts[q] <= 2^18, each in 0 .. K - 1; the total is at most
 * 2^28 words; the words of all queries are concatenated in hesaff_index_build's layout (word_stride 1 or 2).  counts is host memory
 * in both forms.  top applies to every query, 1 <= top <= 1024.
 * THE RESULT OF QUERY q IS, BIT FOR BIT, WHAT hesaff_index_query RETURNS FOR THE SAME WORDS ON THE SAME INDEX (nq2, dot, the three
 * binary64 operations, the order and the tie rules are unchanged): images_out[q * top + r] and scores_out[q * top + r] for
 * r < *count_out = min(top, N); entries past the count are not written.  The embedded forms take a signature per word and answer per
 * query as hesaff_index_query_embedded with the same threshold.
 * The state a batch leaves is the state Q single calls in that order would leave: hesaff_index_get_scores gives the dot, score and
 * nq2 of the batch's last query, and a later single query, add, save or detection behaves as if the batch had been single calls.
 * hesaff_get_index_ms's query_ms reports the whole batch.
 * A batch runs in chunks of consecutive queries: a chunk is the longest run whose device scratch - per query a row of dot and of
 * score over the N images, a head and the ranked row, and the hash table of the chunk's words - fits the budget; one query is always
 * a chunk, even above it.  hesaff_index_set_batch_budget sets the budget in bytes (0: the default, 1 GiB - a design choice, not a
 * measured optimum) and releases what earlier batches allocated; hesaff_index_get_batch_budget reads the budget in force.  The
 * result does not depend on the budget.  The scratch belongs to the context's index, grows to what the batches so far needed, and is
 * released by hesaff_index_clear, by a build, load or add replacing the index, by hesaff_index_set_batch_budget and by destroy;
 * without a batch call nothing is allocated, launched or copied.  The host forms also hold the batch's words (and signatures) in
 * device memory for the call: 4 (12) bytes per word beside the scratch.
 * HESAFF_ERR_ARG, with the index, the last query's scores and the context unchanged: a NULL context or a required pointer NULL; Q, a
 * count, the total or top outside its bounds; word_stride not 1 or 2; a misaligned device pointer (words 4, signatures 8 bytes); a
 * word outside 0 .. K - 1 in any query (the host forms check while staging, the device forms in one read-only pass over all words
 * before any chunk runs); no index built; the embedded forms on a plain index, or hamming outside 0 .. 64.  HESAFF_ERR_NOMEM: what a
 * batch needs is allocated before its first chunk runs, so a batch that cannot get it changes nothing either.
 * hesaff_get_index_batch_ms: HIP-event times at profiling level >= 1, 0 otherwise, summed over the chunks of the last batch: grouping
 * the words, scoring, and finish with selection.  hesaff_index_get_batch_chunks: the chunks the last batch ran in (0 before the first). */
int hesaff_index_query_batch(hesaff_ctx *ctx, int n_queries, const int32_t *counts, const int32_t *words, int word_stride, int top,
                             int32_t *images_out, double *scores_out, int *count_out);
int hesaff_index_query_batch_device(hesaff_ctx *ctx, int n_queries, const int32_t *counts, const void *d_words, int word_stride, int top,
                                    int32_t *images_out, double *scores_out, int *count_out);
int hesaff_index_query_batch_embedded(hesaff_ctx *ctx, int n_queries, const int32_t *counts, const int32_t *words, int word_stride,
                                      const uint64_t *sigs, int hamming, int top, int32_t *images_out, double *scores_out, int *count_out);
int hesaff_index_query_batch_embedded_device(hesaff_ctx *ctx, int n_queries, const int32_t *counts, const void *d_words, int word_stride,
                                             const void *d_sigs, int hamming, int top, int32_t *images_out, double *scores_out, int *count_out);
int hesaff_index_set_batch_budget(hesaff_ctx *ctx, size_t bytes);
int hesaff_index_get_batch_budget(const hesaff_ctx *ctx, size_t *bytes);
int hesaff_index_get_batch_chunks(const hesaff_ctx *ctx, int *chunks);
int hesaff_get_index_batch_ms(const hesaff_ctx *ctx, float *group_ms, float *score_ms, float *select_ms);

/* Spatial verification (no counterpart in the reference): the shortlist of a tf-idf query re-ranked by how many tentative
 * correspondences agree with the best single-correspondence affine hypothesis - the "fast spatial matching" of Philbin et al. 2007
 * under the reference's own assumption that the vertical orientation is preserved (the frame of rectifyAffineTransformationUpIsUp,
 * helpers.cpp:90-97).  It reads the x, y, a, b, c that every words file carries beside the word.  Symbols only, version 8.
 * Everything is binary32 unless stated; no operation is contracted into an FMA; operations are evaluated left to right as written;
 * / and sqrtf are the IEEE operations; a comparison with a NaN is false.
 * Inputs: a query of nq rows and R candidate images of counts[r] rows each, concatenated; a row is the 24-byte row of a words file,
 * { float x, y, a, b, c; uint32 word }.  1 <= R <= 1024 (hesaff_index_query's top); 0 <= nq <= 2^18, 0 <= counts[r] <= 2^18, their sum
 * at most 2^28; K the vocabulary size, 1 <= K <= 2^20, every word < K; P = max_pairs in 1..16; tol = tolerance finite,
 * 0 < tol <= 2^20, in pixels of the candidate image.
 *  1. Frame of a key:  r = sqrtf(c);  q = b / r;  t = a - q * q;  p = sqrtf(t).  N = [[p, 0], [q, r]] satisfies N^T N = [[a, b], [b, c]]
 *     and maps the vertical onto itself.  The key is LIVE iff c > 0, t > 0, 2^-20 <= p <= 2^20, 2^-20 <= r <= 2^20, a <= 2^40,
 *     |x| <= 2^20 and |y| <= 2^20 (all false for a NaN, so a row with a NaN is not live).  Any other key is INERT: it takes part in
 *     nothing and is counted per image.  (hesaff_ellipse can emit canonical NaNs for degenerate regions; such files must verify.)
 *  2. Tentative correspondences of candidate r:  tfq(w) = the live query keys with word w, tf_r(w) = the live keys of candidate r with
 *     word w.  All pairs (query key i, candidate key j), both live, of equal word w with tfq(w) * tf_r(w) <= P, listed in the order
 *     (j ascending, then i ascending); j counts from the candidate's first row.  found_r is their number; the first
 *     M_r = min(found_r, 4096) of the list are USED.
 *  3. Hypothesis h = used correspondence h, query key (xq, yq, pq, qq, rq), candidate key (xd, yd, pd, qd, rd):
 *        L11 = pq / pd;   L22 = rq / rd;   L21 = (qq - qd * L11) / rd          the map T(x) = N_d^-1 N_q (x - x_q) + x_d
 *  4. Error of used correspondence k under h:
 *        dx = xq_k - xq_h;  dy = yq_k - yq_h;  u = L11 * dx;  v = L21 * dx + L22 * dy
 *        ex = (xd_h + u) - xd_k;  ey = (yd_h + v) - yd_k;  e2 = ex * ex + ey * ey
 *     k is an inlier of h iff e2 <= tol2, tol2 = tol * tol; inl(h) = the inliers over k = 0 .. M_r - 1 (k = h among them: inl(h) >= 1).
 *  5. inliers_r = max_h inl(h), the best hypothesis the lowest h that attains it.  M_r = 0: inliers_r = 0, no hypothesis, the key
 *     indices are -1 and the matrix is zeros.
 *  6. The candidates are ranked by (inliers_r descending, position r ascending).
 * Range: for live keys q^2 < a <= 2^40, so |q| < 2^20; hence |L11|, |L22| <= 2^20 / 2^-20 = 2^40 and |L21| < (2^20 + 2^20 * 2^40) * 2^20
 * < 2^81; |dx|, |dy| <= 2^21, so |u| <= 2^61, |v| < 2^103, and ex, ey are finite.  e2 is finite or +inf, never NaN, and +inf is simply
 * not an inlier.  No value forms an address.
 * All accumulations are integer counts: no result depends on launch geometry, on tiling or on the order of atomics; the same input
 * gives the same bytes.
 * hesaff_verify_matches: rows in host memory.  out[R][6] = (inliers, used, found, query_key, candidate_key, inert_keys), hyp[R][3] =
 * (L11, L21, L22) of the best hypothesis, order[R] = the ranking; each may be NULL.  counts is host memory in both forms.
 * hesaff_verify_matches_device: both row arrays in device memory, 4-byte aligned.  The host form checks the words while staging; the
 * device form runs a read-only check kernel first.
 * hesaff_verify_get_pairs: the used correspondences (i, j) of one candidate of the last call, pairs[count][2], in definition order; the
 * memory is the library's, valid until the next hesaff_verify_* call.  hesaff_verify_get_query_inert: the query's inert keys.
 * hesaff_stage_verify_pairs: the production hypothesis kernel alone on m <= 4096 correspondences of the caller's,
 * pairs[m][10] = xq, yq, pq, qq, rq, xd, yd, pd, qd, rd (frames within the live bounds): inl_out[m] = inl(h), *best_out = the best
 * h, -1 for m = 0; each may be NULL.
 * hesaff_get_verify_ms: HIP-event times of the last call at profiling level >= 1 - grouping and pair construction, hypotheses and
 * ranking - 0 otherwise.
 * hesaff_read_words_rows: the whole rows of a words file ("HESAFFW1"), count x 24 bytes; *rows is malloc'ed (hesaff_free; NULL when
 * count is 0); HESAFF_ERR_IO as for hesaff_read_words.
 * Verification is no context state apart from the result of the last call: it neither reads nor changes the vocabulary or the
 * index, its scratch (a hash table of at least 2 sum(counts) slots, 12 bytes each, and 160 KB per candidate) is released before the
 * call returns, and without a call nothing is launched, allocated or copied anywhere.
 * HESAFF_ERR_ARG, nothing changed, the context usable as before: ctx NULL; a required pointer NULL; a count or bound outside the
 * ranges above; a word >= K; tol not finite or out of range; a device pointer that is not 4-byte aligned; a getter before any
 * verify call, or `candidate` outside the last call's.  HESAFF_ERR_NOMEM: the device cannot hold the scratch. */
int hesaff_verify_matches(hesaff_ctx *ctx, int nq, const void *query_rows, int n_candidates, const int32_t *counts, const void *candidate_rows,
                          int vocabulary_size, int max_pairs, float tolerance, int32_t *out, float *hyp, int32_t *order);
int hesaff_verify_matches_device(hesaff_ctx *ctx, int nq, const void *d_query_rows, int n_candidates, const int32_t *counts,
                                 const void *d_candidate_rows, int vocabulary_size, int max_pairs, float tolerance, int32_t *out, float *hyp,
                                 int32_t *order);
int hesaff_verify_get_pairs(hesaff_ctx *ctx, int candidate, const int32_t **pairs, int *count);
int hesaff_verify_get_query_inert(const hesaff_ctx *ctx, int *n);
int hesaff_stage_verify_pairs(hesaff_ctx *ctx, int m, const float *pairs, float tolerance, int32_t *inl_out, int32_t *best_out);
int hesaff_get_verify_ms(const hesaff_ctx *ctx, float *pairs_ms, float *hypotheses_ms);
int hesaff_read_words_rows(const char *path, void **rows, int *count, int *vocabulary_size);

/* Query expansion (no counterpart in the reference): the keys of the verified candidates of a shortlist, back-projected into the
 * query's frame by each candidate's affinity, cut to the query's region and appended to the query - the average query expansion of
 * Chum, Philbin, Sivic, Isard and Zisserman, "Total Recall" (ICCV 2007), over the 5-dof maps hesaff_verify_matches returns.  The
 * result is an ordinary array of words-file rows, which the index and the verifier take unchanged.  Symbols only, version 8.
 * The rules of the verification block hold: binary32, no FMA contraction, operations left to right, one per statement, / and sqrtf
 * the IEEE operations, a comparison with a NaN false; frame, LIVE and the row are those of step 1 there.
 * Inputs: a query of nq rows and R candidates of counts[r] rows, concatenated, within the bounds of hesaff_verify_matches; K =
 * vocabulary_size, every word < K; a uint64 signature per query row and per candidate row, for both sides or for neither;
 * verify_out[R][6] and hyp[R][3] exactly as hesaff_verify_matches returns them - arguments of the caller, no context state, so that
 * constructed hypotheses can be expanded; min_inliers >= 1; max_images in 1..1024; roi[4] = (x0, y0, x1, y1) in the query's frame,
 * finite, |v| <= 2^20, x0 <= x1, y0 <= y1; max_rows with nq <= max_rows <= 2^18, the query limit of the index and of the verifier.
 *  1. Candidate r is ELIGIBLE iff verify_out[r][0] >= min_inliers.  The SELECTED candidates are the first min(max_images, eligible)
 *     eligible ones in the order (inliers descending, r ascending); the position in that order is the rank s.  Of a candidate that
 *     is not eligible nothing but the inlier count is read: its hyp may hold anything.  An eligible candidate - selected or cut by
 *     max_images - must have 0 <= query_key < nq, 0 <= candidate_key < counts[r], both anchor rows live, 2^-40 <= L11 <= 2^40,
 *     2^-40 <= L22 <= 2^40 and |L21| <= 2^81 (the range the verification block derives; false for a NaN): otherwise the call is
 *     refused with HESAFF_ERR_ARG and hesaff_last_error names the lowest such r.
 *  2. Back-projection of key j of a selected candidate, anchors (xq_h, yq_h) = query row query_key, (xd_h, yd_h) = candidate row
 *     candidate_key:
 *        dx = xd_j - xd_h;  dy = yd_j - yd_h;  u = dx / L11;  t = L21 * u;  s = dy - t;  v = s / L22;  x' = xq_h + u;  y' = yq_h + v
 *     and, since x_d - x_dh = L (x_q - x_qh), the ellipse E' = L^T E L:
 *        m0 = a * L11;  m1 = b * L21;  e00 = m0 + m1;  m2 = b * L11;  m3 = c * L21;  e10 = m2 + m3;  e01 = b * L22;  e11 = c * L22
 *        n0 = L11 * e00;  n1 = L21 * e10;  a' = n0 + n1;  n2 = L11 * e01;  n3 = L21 * e11;  b' = n2 + n3;  c' = L22 * e11
 *  3. Key j is KEPT iff it is live, x0 <= x' <= x1, y0 <= y' <= y1 and the frame of (x', y', a', b', c') is live: an expanded row
 *     is always a row the verifier accepts.
 *  4. The expanded query: the nq query rows byte for byte, inert ones included, then the kept rows { x', y', a', b', c', word } in
 *     the order (rank s ascending, j ascending).  Exactly n_out = min(nq + kept_total, max_rows) rows are written: the cut falls on
 *     the weakest selected candidates' highest keys.  The signatures, where given, travel row for row, and words_out[n_out] holds
 *     the words alone (hesaff_index_query takes stride 1 or 2, not 6).
 *  5. info[R][4] = (s or -1, live keys, kept keys, written keys) per candidate; zeros behind the -1 of a candidate that is not selected,
 *     whose rows are not read.
 * Range: for live keys |dx|, |dy| <= 2^21, and L11 >= 2^-40, so u is finite, |u| <= 2^61, and x' is finite.  |t| <= 2^81 * 2^61
 * exceeds binary32: t, s, v and y' may be +-inf, but never NaN - no product has a zero beside an infinity (L21 and u are finite),
 * no sum has two infinities (dy and yq_h are finite), and L22 is finite and positive.  An infinite y' fails the region test.  a' and
 * b' can be NaN (inf - inf from a, b, c <= 2^40 times maps up to 2^81, squared); the frame of a NaN is not live, so the key is
 * dropped.  No value forms an address.
 * It follows that the anchor key itself maps to (xq_h, yq_h) exactly (dx = dy = 0 gives u = t = s = v = 0); that with L = (1, 0, 1)
 * and coordinates that are small integers a shifted copy of the query back-projects to the query's own rows bit for bit; and that a
 * call that selects nothing returns the query unchanged, n_out = nq.
 * The only accumulations are integer counts, and the position of a row follows from counts alone: the same input gives the same
 * bytes whatever the launch geometry.
 * hesaff_expand_query: rows, signatures and the three outputs in host memory; rows_out, words_out (and sigs_out, with signatures)
 * hold min(max_rows, nq + sum(counts)) entries.  sigs_out non-NULL says that signatures are given: then query_sigs (nq > 0) and
 * candidate_sigs (sum(counts) > 0) are required, and without it both must be NULL.  info_out may be NULL.  The words are checked
 * while staging; only the selected candidates' rows are copied to the device.
 * hesaff_expand_query_device: rows, signatures and the three outputs in device memory (rows and words 4-byte, signatures 8-byte
 * aligned), sized as above; counts, verify_out, hyp, roi, n_out and info_out in host memory.  A read-only kernel checks the words.
 * Its outputs feed hesaff_index_query_device(words_out, n_out, 1, ...) and hesaff_verify_matches_device(rows_out, n_out, ...) as
 * they are.
 * hesaff_get_expand_ms: HIP-event times of the last call at profiling level >= 1 - the flags pass with its scan, the scatter - 0
 * otherwise.
 * Expansion is no context state: it reads and changes neither the vocabulary, nor the index, nor the result of the last verify
 * call; its scratch (8 bytes per 64 rows of the selected candidates for the masks, 4 for the bases, 40 per selected candidate; in
 * the host form the staged rows and outputs as well) is released before the call returns, and without a call nothing is launched,
 * allocated or copied.
 * HESAFF_ERR_ARG, nothing changed, the outputs untouched, the context usable as before: ctx NULL; a required pointer NULL; a count or
 * bound outside the ranges above; a word >= K; signatures on one side only; a roi that is not finite, out of range or inverted; a
 * misaligned device pointer; a broken eligible candidate.  HESAFF_ERR_NOMEM: the device cannot hold the scratch. */
int hesaff_expand_query(hesaff_ctx *ctx, int nq, const void *query_rows, const uint64_t *query_sigs, int n_candidates, const int32_t *counts,
                        const void *candidate_rows, const uint64_t *candidate_sigs, const int32_t *verify_out, const float *hyp, int min_inliers,
                        int max_images, const float *roi, int vocabulary_size, int max_rows, void *rows_out, int32_t *words_out,
                        uint64_t *sigs_out, int *n_out, int32_t *info_out);
int hesaff_expand_query_device(hesaff_ctx *ctx, int nq, const void *d_query_rows, const void *d_query_sigs, int n_candidates, const int32_t *counts,
                               const void *d_candidate_rows, const void *d_candidate_sigs, const int32_t *verify_out, const float *hyp,
                               int min_inliers, int max_images, const float *roi, int vocabulary_size, int max_rows, void *d_rows_out,
                               void *d_words_out, void *d_sigs_out, int *n_out, int32_t *info_out);
int hesaff_get_expand_ms(const hesaff_ctx *ctx, float *flags_ms, float *scatter_ms);

/* Same path with inputs already resident in device memory (bench / pipelines that decode
 * on the GPU): d_gray = n contiguous height x width 8-bit grey planes (device pointer).
 * Results stay on the device; per-image counts are copied to the two host arrays.
 * d_keys_out (optional, may be NULL) receives a device pointer to the ordered
 * hesaff_keypoint array of the whole batch, total_out the number of records. */
int hesaff_detect_batch_device(hesaff_ctx *ctx, int n, const void *d_gray, int width, int height,
                               int32_t *count_hessian, int32_t *count_desc, const void **d_keys_out,
                               int64_t *total_out);
/* level 0: no events; 1: per-stage HIP events; 2: also one event pair per k_blur_hess launch */
int hesaff_set_profiling(hesaff_ctx *ctx, int level);
int hesaff_get_timings(const hesaff_ctx *ctx, hesaff_timings *t);

/* replaces: exportKeypoints hesaff.cpp:107-130 (text format README:27-44).
 * hesaff_ellipse: (a,b,c) of one region, closed form of the SVD expression hesaff.cpp:115-123. */
void hesaff_ellipse(const hesaff_keypoint *k, float mrSize, float *a, float *b, float *c);
int hesaff_write_sift(const char *path, const hesaff_keypoint *keys, int n, float mrSize);
/* the same file written by `threads` host threads (0 = auto); threads = 1 formats and writes block by block through a
 * cache-resident buffer (what the per-image workers of hesaff_write_sift_batch / hesaff_process_files do) */
int hesaff_write_sift_mt(const char *path, const hesaff_keypoint *keys, int n, float mrSize, int threads);
/* Binary sidecar of the same rows (no counterpart in the reference): the five floats unprinted and the
 * 128 descriptor bytes, 148 bytes per row instead of about 355 bytes of text.  Little-endian:
 *   char magic[8] = "HESAFFB1"; uint32 dim = 128; uint32 count; count x { float x, y, a, b, c; uint8 desc[128] } */
int hesaff_write_bin(const char *path, const hesaff_keypoint *keys, int n, float mrSize);
/* The same two files from rows that are already formatted / packed - hesaff_process_files formats them on the device
 * (kernels_export.h) so that its writer threads only write: `rows` = len bytes of "x y a b c d1 .. d128\n" lines (n of them) or
 * n rows of 148 bytes; the header lines (hesaff.cpp:109-110) / the 16-byte sidecar header are added here. */
int hesaff_write_sift_rows(const char *path, const char *rows, size_t len, int n);
int hesaff_write_bin_rows(const char *path, const char *rows, int n);
/* the row count of `path` when it is the complete output (format HESAFF_OUT_TEXT or HESAFF_OUT_BIN, optionally | HESAFF_OUT_STRICT, or
 * HESAFF_OUT_WORDS: magic and size == 16 + 24 * count) of an earlier run, -1 otherwise: what hesaff_set_resume goes by (on = 1: as given; on = 2: with HESAFF_OUT_STRICT) */
int hesaff_output_is_complete(const char *path, int format);
/* formats into a malloc'ed buffer (*out, *len); caller frees with hesaff_free */
int hesaff_format_sift(const hesaff_keypoint *keys, int n, float mrSize, char **out, size_t *len);
/* the same bytes, rows formatted by `threads` host threads (0 = one per core, at most 64);
 * hesaff_write_sift uses this form.  SURVEY.md 8(f) rank 1: at GPU rates the text export
 * (42 MB per UHD image, hesaff.cpp:107-130) is the bottleneck of the file path. */
int hesaff_format_sift_mt(const hesaff_keypoint *keys, int n, float mrSize, int threads, char **out, size_t *len);
/* replaces: the per-image exportKeypoints + ofstream of main() (hesaff.cpp:170-176) for a whole
 * batch: results[i] -> paths[i], images spread over `threads` host threads (0 = auto) */
int hesaff_write_sift_batch(int n_images, const char *const *paths, const hesaff_result *results, float mrSize, int threads);
/* what "threads = 0" means above: the CPUs this process may run on (affinity mask), capped by the
 * container's CPU-time limit (cgroup v2 cpu.max) when there is one, at most 64, at least 1.
 * (No counterpart in the reference, which is single-threaded: hesaff.cpp:133-180.) */
int hesaff_host_threads(void);
/* The ONE rule for "host threads per device" (the CLI's --batch, hesaff_process_files' "0 = auto", bench.py and tools/ all use it).
 * devices_sharing_host: how many devices are fed from the CPUs hesaff_host_threads() counts - 8 for one rank of an 8-GPU node,
 * 1 for a process that has the host to itself.
 *   cpus           = max(1, hesaff_host_threads() / devices_sharing_host)      the CPU share of one device, everything included:
 *                                                                                the caller's thread (kernel launches; it sleeps on events),
 *                                                                                the staging threads and the decode / write pool
 *   stage_threads  = clamp(cpus / 4, 1, 4)                                       threads that copy a chunk into pinned memory
 *   pool           = max(2, cpus - stage_threads)                                decode_threads + write_threads (ONE pool, see
 *   decode_threads = max(1, pool / 4) ; write_threads = pool - decode_threads    hesaff_process_files)
 * With 2 CPUs the pool is 2 and time-slices with the caller's and the staging thread, which are idle most of the time.
 * (No counterpart in the reference, which is single-threaded: hesaff.cpp:133-180.) */
typedef struct hesaff_host_plan {
   int cpus, decode_threads, write_threads, stage_threads;
} hesaff_host_plan;
int hesaff_host_plan_for(int devices_sharing_host, hesaff_host_plan *out);
/* the plan's stage_threads for a pool of decode_threads + write_threads (what hesaff_process_files derives from the two counts it is given) */
int hesaff_stage_threads_for_pool(int pool);
/* Page-locked read buffers of hesaff_process_files (the readers fill pinned memory of the context, the copy engine takes the image
 * from where it was read): at most max_bytes are out or parked at any time (default 4 GiB; a request beyond it takes the staging
 * copy), and at most keep_bytes stay pinned when hesaff_process_files returns (default 1 GiB: the next list of a long-lived
 * context starts with warm buffers; 0 releases everything).  No counterpart in the reference. */
int hesaff_set_pinned_read_budget(hesaff_ctx *ctx, size_t max_bytes, size_t keep_bytes);
/* The decode / write pool of hesaff_process_files lowers its threads' priority (nice 10) only when the host plan is CPU-starved
 * (CPUs of this process <= pool threads + 1), so that the caller's thread - which launches the next kernels when an event fires -
 * never queues behind threads that write() flat out.  mode: 0 = never, 1 = always, -1 = that rule (default). */
int hesaff_set_pool_priority(hesaff_ctx *ctx, int mode);
/* test hook: number of inputs on which the fast "%g" formatter and snprintf disagree (must be 0) */
int hesaff_test_fmt_g(const float *v, int n);
void hesaff_free(void *p);

/* replaces: cv::imread(argv[1]) hesaff.cpp:137 for PBM / PGM / PPM files, plain and binary (P1..P6), maxval 1..65535, the way
 * OpenCV's PxM decoder delivers them at imread's default flag: binary 8-bit samples as they are, plain samples scaled by
 * 255 / maxval, 16-bit samples reduced to the high byte, bitmaps as 255 / 0.
 * *data is malloc'ed (free with hesaff_free), tightly packed, channels 1 or 3. */
int hesaff_read_pnm(const char *path, uint8_t **data, int *width, int *height, int *channels);
/* the same for PNG files (decoded with zlib): what cv::imread returns with its default flag - 8 bits per
 * channel, alpha dropped, 16-bit samples reduced to the high byte, palette / 1-2-4-bit grey expanded;
 * channels = 1 for grey files, 3 (R,G,B order) otherwise.  Adam7-interlaced files are read too. */
int hesaff_read_png(const char *path, uint8_t **data, int *width, int *height, int *channels);
/* Huffman-coded 8-bit JPEG, sequential or progressive, grey or YCbCr: the integer algorithms of libjpeg at
 * cv::imread's settings (JDCT_ISLOW inverse DCT, "fancy" chroma up-sampling, JFIF colour conversion), pixel for pixel
 * the bytes libjpeg / libjpeg-turbo return for a complete file; channels = 1 for grey files, 3 (R,G,B order)
 * otherwise.  Arithmetic-coded, lossless, 12-bit and CMYK files: HESAFF_ERR_IO.  So is a file with an interleaved scan of more
 * than 10 blocks per MCU (luma 3x3 or more beside two chroma blocks), which libjpeg refuses too (JERR_BAD_MCU_SIZE) - from this
 * reader and from hesaff_read_jpeg_coefficients alike; scans of one component each are not bound by it. */
int hesaff_read_jpeg(const char *path, uint8_t **data, int *width, int *height, int *channels);
/* Windows bitmaps as OpenCV's BMP decoder delivers them at imread's default flag: 1 / 4 / 8 bits through the palette (uncompressed, RLE4, RLE8),
 * 16 bits (5-5-5, or 5-6-5 by bit fields; low bits left zero), 24 bits, 32 bits (fourth byte dropped), bottom-up or top-down, OS/2 core headers;
 * channels = 3 (R,G,B order), or 1 when the whole palette is grey. */
int hesaff_read_bmp(const char *path, uint8_t **data, int *width, int *height, int *channels);
/* Baseline TIFF the way cv::imread delivers it (libtiff's RGBA interface, alpha byte dropped): bilevel / 2 / 4 / 8-bit grey (MinIsBlack,
 * MinIsWhite), 8-bit palette, 8-bit RGB and RGB + alpha (unassociated alpha multiplied in: (v a + 127) / 255); strips or tiles, chunky or
 * planar, both byte orders; uncompressed, PackBits, LZW, Deflate, horizontal predictor.  16-bit / float samples, YCbCr / CMYK / Lab, JPEG-
 * or fax-compressed data and BigTIFF are refused (HESAFF_ERR_IO).  channels = 1 for grey files, 3 (R,G,B order) otherwise. */
int hesaff_read_tiff(const char *path, uint8_t **data, int *width, int *height, int *channels);
/* PBM/PGM/PPM, PNG, JPEG, BMP or TIFF by magic number */
int hesaff_read_image(const char *path, uint8_t **data, int *width, int *height, int *channels);
/* the same with the pixel buffer from the caller's allocator (only the PNM reader asks it; see hesaff_blob_alloc below):
 * hesaff_process_files reads straight into pinned host memory this way (no malloc'ed buffer, no staging copy) and recycles the
 * buffers.  A buffer the allocator handed out belongs to the caller whatever happens: when the call fails after the allocator was
 * asked, the buffer comes back through *data (NULL otherwise) and is never passed to free(). */
typedef void *(*hesaff_blob_alloc)(size_t bytes, int *zeroed, void *user);
int hesaff_read_pnm_alloc(const char *path, uint8_t **data, int *width, int *height, int *channels, hesaff_blob_alloc alloc, void *user);
int hesaff_read_image_alloc(const char *path, uint8_t **data, int *width, int *height, int *channels, hesaff_blob_alloc alloc, void *user);

/* The host half of cv::imread (hesaff.cpp:137) for a JPEG file when the pixels are made on the device (hesaff_process_files does this
 * for every JPEG of its list): markers and entropy decoding only - Huffman, sequential or progressive - which is the part of a JPEG
 * decoder that has to run in order.  The inverse DCT, the chroma up-sampling and the colour conversion of hesaff_read_jpeg (the same
 * integer algorithms, so the same bytes) run in kernels_jpeg.h over all blocks / pixels of a chunk of images at once.
 * layout: what images must share to travel in one chunk.  blob (malloc'ed, hesaff_free): HESAFF_JPEG_BLOB_HEADER bytes - the
 * components' quantisation tables, uint16[3][64] in natural order, at byte 0; int32 "YCbCr, convert to RGB" flag at byte 384 - then
 * the coefficients, int16, natural order, 64 per block, blocks row by row (bw x bh per component), component after component. */
#define HESAFF_JPEG_BLOB_HEADER 1024
typedef struct hesaff_jpeg_layout {
   int32_t width, height, channels;   /* channels: 1 (grey file) or 3 (R,G,B after conversion) */
   int32_t h[3], v[3];                /* sampling factors of the components */
   int32_t hx[3], vx[3];              /* up-sampling ratios to full resolution (hmax / h, vmax / v) */
   int32_t bw[3], bh[3];              /* blocks per row / column of a component's coefficient array (whole MCUs) */
   int32_t cw[3], chgt[3];            /* component size in samples: ceil(image size * factor / largest factor) */
} hesaff_jpeg_layout;
int hesaff_read_jpeg_coefficients(const char *path, hesaff_jpeg_layout *layout, uint8_t **blob, size_t *blob_bytes);
/* the same with the blob's memory from the caller: alloc(bytes, &zeroed, user) returns memory that free() accepts (or NULL) and says
 * whether it is already zero.  hesaff_process_files hands back the blobs of images that have gone to the device - a decoder thread
 * then writes into warm memory instead of 25 MB of fresh zero pages per photograph.  The blob's content does not depend on it. */
int hesaff_read_jpeg_coefficients_alloc(const char *path, hesaff_jpeg_layout *layout, uint8_t **blob, size_t *blob_bytes,
                                        hesaff_blob_alloc alloc, void *user);

/* ---- stage entry points (host pointers in/out; used by the parity tests and by callers
 *      that want one operator of the reference at a time) ---- */

/* gaussianBlur helpers.cpp:283-289 (cv::GaussianBlur, BORDER_REPLICATE, ksize from sigma) */
int hesaff_stage_gaussian_blur(hesaff_ctx *ctx, const float *in, int rows, int cols, float sigma, float *out);
/* HessianDetector::hessianResponse pyramid.cpp:63-114 (frame written as 0) */
int hesaff_stage_hessian_response(hesaff_ctx *ctx, const float *in, int rows, int cols, float norm, float *out);
/* halfImage helpers.cpp:331-339 */
int hesaff_stage_half_image(hesaff_ctx *ctx, const float *in, int rows, int cols, float *out);
/* Scale-space of one image: initial blur pyramid.cpp:276-280 + every octave's L0..L4 and
 * R0..R4 (pyramid.cpp:224-259).  planes receives, octave after octave, 5 blur planes then 5
 * response planes, each rows_o x cols_o tightly packed; returns the octave count in
 * *n_octaves.  Call with planes == NULL to get n_octaves and the float count in *n_floats. */
int hesaff_stage_pyramid(hesaff_ctx *ctx, const uint8_t *gray, int rows, int cols, float *planes,
                         int *n_octaves, size_t *n_floats);
/* the same for a float grey plane (tightly packed rows x cols, the accepted values of the _f32 entry points): the pixels of the BlurPlane
 * a callback receives when the input was float (hesaff.hpp) */
int hesaff_stage_pyramid_f32(hesaff_ctx *ctx, const float *plane, int rows, int cols, float *planes, int *n_octaves, size_t *n_floats);
/* detectPyramidKeypoints pyramid.cpp:261-292 up to the onHessianKeypointDetected callback
 * pyramid.h:46: fills f[n][5] = x,y,s,pixelDistance,response and i[n][5] =
 * type,octave,level,r0,c0 in reference order; returns n in *count (cap = array capacity). */
int hesaff_stage_hessian_keypoints(hesaff_ctx *ctx, const uint8_t *gray, int rows, int cols, int cap,
                                   float *f, int32_t *i, int *count);
/* The same chain - extrema scan (pyramid.cpp:206-222), localizeKeypoint (:122-204) with the octaveMap rule, getHessianPointType
 * (:24-37) and the ordering - on planes of the caller's instead of an image's: L and R are [n_images][5][rows][cols] floats each, tightly
 * packed, the blur planes L0..L4 and the response planes R0..R4 of ONE octave (L4 is not read).  They are taken as octave 0: the octave
 * index returned is 0 and pixelDistance is that of the first level.  f and i as above, image[n] = the index of the image; the order is the
 * reference's (image, level, r0, c0).  band: the rows one wavefront of the extrema scan marches down - 0 for the height the batch
 * path would choose for this size, or 32, 64 or 128 (every height gives the same list).
 * Domain: every value of L and R is finite.  NaN and infinities are outside it - the response of a finite blur plane is finite - and
 * what the chain makes of them is not specified.
 * HESAFF_ERR_ARG: rows or cols <= 2 * 5 + 2 (no octave, pyramid.cpp:283), another band, a NULL plane, a context with upscaleInputImage.
 * HESAFF_ERR_CAPACITY: more candidates or keypoints than the plan for this size holds, as for an image. */
int hesaff_stage_detect_planes(hesaff_ctx *ctx, int n_images, int rows, int cols, const float *L, const float *R, int band, int cap,
                               float *f, int32_t *i, int32_t *image, int *count);
/* AffineShape::findAffineShape affine.cpp:35-100 for n keypoints on one blur plane.
 * kp[n][4] = x,y,s,pixelDistance; out: converged[n], U[n][4] (a11,a12,a21,a22 as passed to
 * onAffineShapeFound affine.h:50-57), iters[n]. */
int hesaff_stage_find_affine_shape(hesaff_ctx *ctx, const float *blur, int rows, int cols, int n,
                                   const float *kp, int32_t *converged, float *U, int32_t *iters);
/* rectifyAffineTransformationUpIsUp helpers.cpp:90-97 for n matrices (in place, A[n][4]) */
int hesaff_stage_rectify(hesaff_ctx *ctx, int n, float *A);
/* One pass of findAffineShape's tail, affine.cpp:72-97 (invSqrt, the eigen ratio, the U update, getEigenvalues and the two decisions;
 * the device function k_affine calls), for n rows of operands, with the context's convergenceThreshold.  In and out, in place:
 * abc[n][3] (the three sums; out: as invSqrt leaves them), U[n][4], ratio[n] (in: eigen_ratio_act of the pass before; out: this pass's).
 * Out: l[n][4] = l1, l2 of invSqrt, then l1, l2 of getEigenvalues (invSqrt's again where it returns false); state[n] = 0 continue,
 * 1 break (no real eigenvalues, or l1 / l2 beyond 6), 2 converged.  Every float value is accepted. */
int hesaff_stage_affine_tail(hesaff_ctx *ctx, int n, float *abc, float *U, float *ratio, float *l, int32_t *state);
/* AffineShape::normalizeAffine affine.cpp:102-144 for n keypoints on one image.
 * kp[n][3] = x,y,s; A[n][4] rectified; out: rejected[n] (1 = reference returned true),
 * patches[n][41*41]. */
int hesaff_stage_normalize_affine(hesaff_ctx *ctx, const float *img, int rows, int cols, int n,
                                  const float *kp, const float *A, int32_t *rejected, float *patches);
/* SIFTDescriptor::computeSiftDescriptor siftdesc.cpp:115-140 for n 41x41 patches;
 * desc[n][128] = the values of `vec` cast as at hesaff.cpp:91. */
int hesaff_stage_sift(hesaff_ctx *ctx, int n, const float *patches, uint8_t *desc);
/* the same launch, additionally returning what the descriptor kernels hand to each other: meanvar[n][2] = the mean and `var` of
 * photometricallyNormalize (helpers.cpp:253-268), hist[n][128] = `vec` before the first normalizeVec (siftdesc.cpp:98).  A one-ulp
 * error in either almost never moves a descriptor byte; tests compare them as bits.
 * Patch domain of the descriptor kernels (both entry points): every value finite with |v| <= 2^20, the bound of the _f32 entry points'
 * pixels, which normalizeAffine's interpolation and smoothing do not exceed.  Within it a patch may be flat (var < 1e-4: it keeps its raw
 * pixels, gradients down to denormals and 0) or constant.  Infinities, NaN and larger magnitudes are outside the domain. */
int hesaff_stage_sift_parts(hesaff_ctx *ctx, int n, const float *patches, float *meanvar, float *hist, uint8_t *desc);
/* hesaff_stage_sift with the pipeline's per-keypoint flags: alive[n], 0 = a keypoint normalizeAffine rejected.  The descriptor kernels
 * write nothing for such a keypoint: desc[n][128] goes to the device as the caller filled it and comes back, the rows of dead
 * keypoints unchanged. */
int hesaff_stage_sift_alive(hesaff_ctx *ctx, int n, const float *patches, const int32_t *alive, uint8_t *desc);
/* the same launch with an explicit descriptor mode (hesaff_set_descriptor's definition; HESAFF_DESC_SIFT / HESAFF_DESC_ROOTSIFT, anything
 * else HESAFF_ERR_ARG).  alive NULL: every keypoint alive; otherwise as hesaff_stage_sift_alive. */
int hesaff_stage_sift_mode(hesaff_ctx *ctx, int n, const float *patches, const int32_t *alive, int mode, uint8_t *desc);
/* steps 1-6 of hesaff_set_orientation's definition (the production kernel, k_orientation) on n caller-supplied 41 x 41 patches:
 * theta[n]; optionally (NULL: not wanted) hist[n][36], the histogram after smoothing, and cs[n][2] = (cos theta, sin theta) */
int hesaff_stage_orientation(hesaff_ctx *ctx, int n, const float *patches, float *theta, float *hist, float *cs);
/* the peak rule of hesaff_set_orientation_count (the production kernel's multi form, k_orientation_peaks) on n caller-supplied 41 x 41
 * patches with orientation count k in 1..4: n_ori[n], and for every rank j the bin bins[n][4] and the angle theta[n][4]; beyond n_ori the
 * bin is -1 and the angle 0.  A flat histogram: n_ori 1, bin m (0), angle 0. */
int hesaff_stage_orientation_peaks(hesaff_ctx *ctx, int n, const float *patches, int k, int32_t *n_ori, int32_t *bins, float *theta);
/* exportKeypoints hesaff.cpp:107-130 on the device for n records in host memory (what hesaff_process_files runs per chunk):
 * format = HESAFF_OUT_TEXT: the bytes of the .hesaff.sift file, == hesaff_format_sift; HESAFF_OUT_BIN: the bytes of the sidecar,
 * == hesaff_write_bin's file.  *out is malloc'ed (hesaff_free). */
int hesaff_stage_export(hesaff_ctx *ctx, const hesaff_keypoint *keys, int n, float mrSize, int format, char **out, size_t *len);
/* the device's "%g" print of n floats: 16 bytes per value in text (unused bytes 0) and its length in lens; for testing that
 * it equals the host's over the whole binary32 range */
int hesaff_stage_fmt_g(hesaff_ctx *ctx, int n, const float *v, char *text, int32_t *lens);
/* the device half of the JPEG reader for n images of one layout (blobs back to back, blob_bytes each, from
 * hesaff_read_jpeg_coefficients): pixels[n][height][width][channels] == what hesaff_read_jpeg returns for the files */
int hesaff_stage_jpeg_pixels(hesaff_ctx *ctx, const hesaff_jpeg_layout *layout, int n, const uint8_t *blobs, size_t blob_bytes, uint8_t *pixels);
/* device evaluation of the pinned libm restatements (hmath.h) for testing */
int hesaff_stage_math(hesaff_ctx *ctx, int n, const float *a, const float *b, float *atan2_out, float *pow2_out);
/* the per-pixel forms of the descriptor gradient (helpers.cpp:269-280, siftdesc.cpp:123-137): orientation atan2f(gy, gx) and
 * magnitude sqrt(gx^2 + gy^2), each in the general form and in the form without range handling that the kernel uses on
 * photometrically normalised patches (operands zero or normal); for testing that the two agree bit for bit */
int hesaff_stage_math_sift(hesaff_ctx *ctx, int n, const float *gy, const float *gx, float *ori_general, float *ori_nd,
                           float *grad_general, float *grad_nd);
/* the forms the descriptor's gradient kernel takes for a flat patch (raw pixels: finite operands of any magnitude, denormals and zeros
 * included; no infinities or NaN), as the kernel calls them: ori = atan2f(gy, gx) in the table-driven general form, grad =
 * sqrt(gx^2 + gy^2), coord = the orientation coordinate 8 (ori + 2 pi) / (2 pi) of siftdesc.cpp:65 */
int hesaff_stage_math_sift_general(hesaff_ctx *ctx, int n, const float *gy, const float *gx, float *ori, float *grad, float *coord);

/* Host-side tables the kernels use (for known-answer tests): computeGaussMask
 * helpers.cpp:104, computeCircularGaussMask helpers.cpp:131, precomputeBinsAndWeights
 * siftdesc.cpp:18, OpenCV getGaussianKernel. */
int hesaff_table_gauss_mask(int size, float *mask);
int hesaff_table_circ_gauss_mask(int size, float *mask);
int hesaff_table_sift_bins(int32_t *bin0, int32_t *bin1, float *w0, float *w1);
int hesaff_table_gauss_kernel(float sigma, int cap, float *taps, int *ksize);

/* ---- multi-GPU: images of a batch shard across the devices of a node, no data-path collective ---- */
/* number of visible HIP devices (0 when there is none / no runtime) */
int hesaff_device_count(void);
/* contiguous block [*lo, *hi) of n items owned by `rank` of `world`: item i belongs to rank floor(i * world / n);
 * the same rule as hesaff_amd/shard.py:shard_range (bench.py, one process per GPU) */
int hesaff_shard_range(int n, int rank, int world, int *lo, int *hi);

const char *hesaff_version(void);

#ifdef __cplusplus
}
#endif
#endif /* HESAFF_AMD_H */
