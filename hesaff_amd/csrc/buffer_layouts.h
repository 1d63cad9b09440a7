// buffer_layouts.h -- where the arrays of a device buffer lie, for every buffer that holds more than one: ONE function per layout, which
// both the allocation (its bytes) and the pointers the kernels receive (its offsets) come from.  Byte offsets, no pointers and no HIP: the
// base is added once, where a layout meets its buffer (pipeline.hip: make_lists, rank_arrays; capi_stage.h: StageArena), and
// tests/native/plan_check.cpp checks every layout on the CPU (tests/test_batch_plan.py) - inside the buffer, disjoint, aligned, and for
// the lists of a context byte for byte where they have always been.
#pragma once
#include <cstddef>
#include <cstdint>

#include "chunk_engine.h"   // HsError
#include "device_lists.h"
#include "plan_consts.h"

namespace hesaff_plan {

// A bump allocator over byte offsets: take<T>(count, align) is the offset of `count` T behind everything taken so far, bytes() the end of
// the last array.  An end beyond SIZE_MAX is HESAFF_ERR_ARG, never a wrapped offset.
struct Carver {
   size_t end = 0;
   template <class T> size_t take(size_t count, size_t align = alignof(T))
   {
      const size_t pad = (align - end % align) % align;
      if (pad > SIZE_MAX - end || count > (SIZE_MAX - end - pad) / sizeof(T))
         throw hesaff_engine::HsError(HESAFF_ERR_ARG, "a device buffer's layout exceeds the address space");
      const size_t at = end + pad;
      if (count) end = at + count * sizeof(T);   // (an empty array occupies nothing, not even its padding)
      return at;
   }
   size_t bytes() const { return end; }
};

// ---- the lists of a context over its keypoint capacity `cap` (a multiple of 64: every array starts 16-byte aligned) ----
constexpr size_t HS_LIST_ALIGN = 16;

// RecList: x, y, s, response in b_rec_f; meta, cell, key, bit in b_rec_i; word in b_rec_w
struct RecLayout { size_t x, y, s, response, f_bytes, meta, cell, key, bit, i_bytes, word, w_bytes; };
inline RecLayout rec_layout(size_t cap)
{
   RecLayout L;
   Carver f, i, w;
   L.x = f.take<float>(cap, HS_LIST_ALIGN); L.y = f.take<float>(cap, HS_LIST_ALIGN); L.s = f.take<float>(cap, HS_LIST_ALIGN);
   L.response = f.take<float>(cap, HS_LIST_ALIGN); L.f_bytes = f.bytes();
   L.meta = i.take<int32_t>(cap, HS_LIST_ALIGN); L.cell = i.take<uint32_t>(cap, HS_LIST_ALIGN); L.key = i.take<uint32_t>(cap, HS_LIST_ALIGN);
   L.bit = i.take<uint32_t>(cap, HS_LIST_ALIGN); L.i_bytes = i.bytes();
   L.word = w.take<long long>(cap, HS_LIST_ALIGN); L.w_bytes = w.bytes();
   return L;
}

// HessList: x, y, s, response in b_hess_f; meta, r0c0 in b_hess_i
struct HessLayout { size_t x, y, s, response, f_bytes, meta, r0c0, i_bytes; };
inline HessLayout hess_layout(size_t cap)
{
   HessLayout L;
   Carver f, i;
   L.x = f.take<float>(cap, HS_LIST_ALIGN); L.y = f.take<float>(cap, HS_LIST_ALIGN); L.s = f.take<float>(cap, HS_LIST_ALIGN);
   L.response = f.take<float>(cap, HS_LIST_ALIGN); L.f_bytes = f.bytes();
   L.meta = i.take<int32_t>(cap, HS_LIST_ALIGN); L.r0c0 = i.take<int32_t>(cap, HS_LIST_ALIGN); L.i_bytes = i.bytes();
   return L;
}

// AffineOut in b_aff: converged, iters, U[4]
struct AffineLayout { size_t converged, iters, U, bytes; };
inline AffineLayout affine_layout(size_t cap)
{
   AffineLayout L;
   Carver a;
   L.converged = a.take<int32_t>(cap, HS_LIST_ALIGN); L.iters = a.take<int32_t>(cap, HS_LIST_ALIGN); L.U = a.take<float>(4 * cap, HS_LIST_ALIGN);
   L.bytes = a.bytes();
   return L;
}

// PatchWork: P0, alive, A[4] in b_pw; the bins' lists [HS_NBINS][cap] are all of b_bins
struct PatchLayout { size_t P0, alive, A, pw_bytes, bin_items, bins_bytes; };
inline PatchLayout patch_layout(size_t cap)
{
   PatchLayout L;
   Carver p, b;
   L.P0 = p.take<int32_t>(cap, HS_LIST_ALIGN); L.alive = p.take<int32_t>(cap, HS_LIST_ALIGN); L.A = p.take<float>(4 * cap, HS_LIST_ALIGN);
   L.pw_bytes = p.bytes();
   L.bin_items = b.take<uint32_t>((size_t)HS_NBINS * cap, HS_LIST_ALIGN); L.bins_bytes = b.bytes();
   return L;
}

// OrientRanks in b_ori_ranks: the frames, window sides, flags and descriptor rows of the ranks 1 .. K - 1 of an orientation count K,
// each array rank-major over the capacity - 16 + 4 + 4 + 128 = 152 bytes per keypoint and rank
struct RankLayout { size_t A, P0, alive, desc, bytes; };
inline RankLayout rank_layout(int K, size_t cap)
{
   RankLayout L;
   Carver r;
   const size_t n = (size_t)(K - 1) * cap;
   L.A = r.take<float>(4 * n, HS_LIST_ALIGN); L.P0 = r.take<int32_t>(n, HS_LIST_ALIGN); L.alive = r.take<int32_t>(n, HS_LIST_ALIGN);
   L.desc = r.take<uint8_t>(128 * n, HS_LIST_ALIGN); L.bytes = r.bytes();
   return L;
}

// ---- the descriptor stage's scratch for n keypoints: the pipeline's per-group buffers and hesaff_stage_sift's arrays ----
// Floats of each (n is a 32-bit count: nothing here can wrap): the patches, n x 41 x 41; mean and variance, 2 n; the gradient pairs,
// n x HS_VO_PITCH float2 and 64 bytes.  Each is a buffer of its own in the pipeline, an array of the stage arena in the operator.
struct GroupScratch { size_t patch_floats, meanvar_floats, vo_floats; };
inline GroupScratch group_scratch(uint32_t n) { return {(size_t)n * HS_PATCH_PIX, (size_t)n * 2, (size_t)n * HS_VO_PITCH * 2 + 64 / sizeof(float)}; }

// ---- the arrays of a stage operator in the context's stage buffer (capi_stage.h: StageArena) ----
// Declared one after the other, each 256-byte aligned: add<T>(count) is the array's place, bytes() what the buffer must hold.
template <class T> struct Span {
   size_t off, count;
   size_t bytes() const { return count * sizeof(T); }
};
struct StagePlan {
   Carver cv;
   template <class T> Span<T> add(size_t count) { return {cv.take<T>(count, 256), count}; }
   size_t bytes() const { return cv.bytes(); }
};

} // namespace hesaff_plan
