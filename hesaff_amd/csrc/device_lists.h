// device_lists.h -- the pointer bundles the kernels take: the lists of a batch, the outputs of its stages, the records it leaves.
// Plain structs of pointers and counts, no HIP: the kernel headers include them, buffer_layouts.h says where in a device buffer each
// array lies, and tests/native/plan_check.cpp checks that on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define HS_LIST_HD __host__ __device__
#else
#define HS_LIST_HD
#endif

// Candidates of one octave: findLevelKeypoints pyramid.cpp:206-222 appends (img,level,r,c) for every pixel that
// passes isMax / isMin (:39-61); unordered here, the order is restored by the bitmask ranks in k_scatter_ordered.
// A candidate carries the 19 response values localizeKeypoint's first iteration reads (pyramid.cpp:132-150): k_extrema_march has
// them in registers when it finds the extremum, and 89 % of the candidates converge in that iteration - so k_localize reads one
// 96-byte record per candidate instead of nine scattered cache lines of three response planes (33 M candidates per 256 UHD
// images: 3 GB written + 3 GB read instead of 19-38 GB of line fetches).
struct CandRec {
   uint32_t id0, id1;   // img<<2 | level, r<<16 | c;  id0 == HS_CAND_HOLE: an unused slot of a wavefront's block of 64
   float v[19];         // cur 3x3 row-major (rows r-1..r+1, columns c-1..c+1) | low: centre, left, right, up, down | high: the same five
   uint32_t pad[3];
};
// (HS_CAND_BLOCK, the slots a wavefront reserves at a time: plan_consts.h)
struct CandList {
   uint32_t *count;   // device counter (slots handed out, holes included)
   CandRec *items;
   uint32_t cap;
   uint32_t *overflow;   // set to 1 when a list ran out of capacity
};

struct RecList {   // surviving localisations of the whole batch (unordered)
   uint32_t *count;
   uint32_t cap;
   float *x, *y, *s, *response;
   int32_t *meta;       // img<<8 | octave<<4 | level<<2 | type
   uint32_t *cell;      // final pixel index rf*cols+cf inside the octave plane (for the map)
   uint32_t *key;       // level*N + r0*cols + c0
   long long *word;     // bitmask word index of (img,octave,level,r0,c0>>6)
   uint32_t *bit;       // c0 & 63
};

struct HessList {   // ordered Hessian keypoints of the batch = onHessianKeypointDetected calls
   float *x, *y, *s, *response;
   int32_t *meta;    // img<<8 | octave<<4 | level<<2 | type
   int32_t *r0c0;    // r0<<16 | c0 (provenance, for the stage API)
   uint32_t cap;
};

// Two launches: the record goes to its rank as ONE 32-byte item (the six fields side by side) and a second, streaming kernel deals the items out to
// the six arrays of the Hessian list.  Scattering the six fields themselves (rounds 1-4) was six partial-line stores per record, 33 M records per
// 256 UHD images: 2.7 ms; a 32-byte store is one whole sector, and the second pass is coalesced on both sides.
struct __attribute__((aligned(32))) HessItem { float x, y, s, response; int32_t meta, r0c0; uint32_t pad0, pad1; };

struct AffineOut {
   int32_t *converged;   // 1 = onAffineShapeFound was called
   float *U;             // [n][4] a11,a12,a21,a22
   int32_t *iters;
};

struct PatchWork {
   float *A;            // [n][4] rectified a11,a12,a21,a22
   int32_t *P0;         // 2*int(mrScale)+1 ; 0 = dead before the patch stage
   int32_t *alive;      // 1 while the keypoint is still a candidate for output
   uint32_t *bin_count; // [HS_NBINS]
   uint32_t *bin_work;  // [HS_NBINS] next unclaimed item of each bin's list (dynamic scheduling of the patch kernels)
   uint32_t *bin_items; // [HS_NBINS][cap]
   uint32_t cap;
};

struct KeyRec {   // == hesaff_keypoint (include/hesaff_amd.h), 164 bytes
   float x, y, s, a11, a12, a21, a22, response;
   int32_t type;
   uint8_t desc[128];
};
#define HS_PACK_DW 41   // dwords per record
static_assert(sizeof(KeyRec) == 4 * HS_PACK_DW && offsetof(KeyRec, desc) == 36, "record layout");

// What the ranks j >= 1 of an orientation count K own, rank-major over the keypoint capacity: array[(j - 1) * cap + h].  Rank 0 lives in
// the PatchWork arrays and b_desc, as the one orientation does.
struct OrientRanks {
   int K;              // the orientation count, 2..HS_ORI_MAX_COUNT
   uint32_t cap;
   float *A;           // [K - 1][cap][4] the turned frames
   int32_t *P0;        // [K - 1][cap]
   int32_t *alive;     // [K - 1][cap] behind k_orientation_peaks: rank < n_ori; behind the rank's k_prepare_patch_second: the rank has a key
   uint8_t *desc;      // [K - 1][cap][128]
   // the stage entry point's outputs by h - h_lo (null in the pipeline): n_ori, and per rank the bin (-1 beyond n_ori) and theta (0 beyond it)
   int32_t *n_ori, *bins;
   float *thetas;
   HS_LIST_HD float *A_of(int j) const { return A + (size_t)(j - 1) * cap * 4; }
   HS_LIST_HD int32_t *P0_of(int j) const { return P0 + (size_t)(j - 1) * cap; }
   HS_LIST_HD int32_t *alive_of(int j) const { return alive + (size_t)(j - 1) * cap; }
   HS_LIST_HD uint8_t *desc_of(int j) const { return desc + (size_t)(j - 1) * cap * 128; }
};

struct SiftIO {
   const float *patches;     // [n][1681] (index = h - h_lo)
   const int32_t *alive;     // [n] flags, indexed by h
   float *meanvar;           // [n][2]
   float *vec;               // [n][128] un-normalised histogram: the stage API's test hook, null in the pipeline (not written)
   uint8_t *desc;            // [n][128] (index = h, absolute)
   uint32_t h_lo, h_hi;
};
