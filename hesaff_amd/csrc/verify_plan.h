// verify_plan.h -- the host arithmetic of spatial verification (hesaff_verify_matches, include/hesaff_amd.h): which calls are refused,
// the frame of a key and the rule that makes it live, and where the arrays of a call and of its result lie in their buffers.  Pure
// functions and plain structs, no HIP: capi_verify.h and kernels_verify.h obtain their numbers here, and
// tests/native/verify_plan_check.cpp checks them on the CPU (tests/test_verify_host.py).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "buffer_layouts.h"   // StagePlan, Span
#include "index_plan.h"       // the (image, word) key and the hash table of the build: tf_r(w) is counted the same way

#if defined(__HIPCC__)
#define HS_VERIFY_HD __host__ __device__ __forceinline__
#else
#define HS_VERIFY_HD inline
#endif

namespace hesaff_plan {

constexpr int64_t HS_VERIFY_MAX_CANDIDATES = 1024;               // hesaff_index_query's `top`: one block ranks them
constexpr int64_t HS_VERIFY_MAX_WORDS = (int64_t)1 << 20;        // the word takes 20 bits of the hash key, the candidate the 20 above
constexpr int64_t HS_VERIFY_MAX_IMAGE_KEYS = (int64_t)1 << 18;   // of a candidate, and of the query
constexpr int64_t HS_VERIFY_MAX_KEYS = (int64_t)1 << 28;         // of all candidates: key positions are uint32
constexpr int HS_VERIFY_MAX_PAIRS = 16;                          // P: a group of query keys that is ever read holds at most this many
constexpr int HS_VERIFY_MAX_USED = 4096;                         // M_r <= 4096: the correspondences that make and judge hypotheses
constexpr float HS_VERIFY_MAX_TOL = 1048576.0f;                  // 2^20 pixels
constexpr float HS_VERIFY_MIN_AXIS = 9.5367431640625e-07f;       // 2^-20 <= p, r
constexpr float HS_VERIFY_MAX_AXIS = 1048576.0f;                 // p, r <= 2^20
constexpr float HS_VERIFY_MAX_A = 1099511627776.0f;              // a <= 2^40
constexpr float HS_VERIFY_MAX_COORD = 1048576.0f;                // |x|, |y| <= 2^20

// one row of a words file ("HESAFFW1")
struct VerifyRow { float x, y, a, b, c; uint32_t word; };
static_assert(sizeof(VerifyRow) == 24, "24 bytes per row");

inline bool verify_counts_ok(int64_t n_candidates, int64_t k) { return n_candidates >= 1 && n_candidates <= HS_VERIFY_MAX_CANDIDATES && k >= 1 && k <= HS_VERIFY_MAX_WORDS; }
inline bool verify_image_keys_ok(int64_t count) { return count >= 0 && count <= HS_VERIFY_MAX_IMAGE_KEYS; }
inline bool verify_total_ok(int64_t total) { return total >= 0 && total <= HS_VERIFY_MAX_KEYS; }
inline bool verify_pairs_ok(int64_t max_pairs) { return max_pairs >= 1 && max_pairs <= HS_VERIFY_MAX_PAIRS; }
inline bool verify_tolerance_ok(float tol) { return tol > 0.0f && tol <= HS_VERIFY_MAX_TOL; }   // (false for a NaN; an infinity is above the bound)
inline bool verify_used_ok(int64_t m) { return m >= 0 && m <= HS_VERIFY_MAX_USED; }
// counts[n_candidates] -> the number of keys, or -1 where a candidate or the sum is out of bounds
inline int64_t verify_total_keys(const int32_t *counts, int64_t n_candidates)
{
   int64_t total = 0;
   for (int64_t i = 0; i < n_candidates; i++) {
      if (!verify_image_keys_ok(counts[i])) return -1;
      total += counts[i];
   }
   return verify_total_ok(total) ? total : -1;
}

// The frame of a key, step 1 of the definition: N = [[p, 0], [q, r]] with N^T N = [[a, b], [b, c]].  One operation per statement, so
// that no compiler contracts a product into the subtraction; sqrtf and / are the IEEE operations.  Every comparison is false for a
// NaN, so a row with a NaN in any field is not live.
struct VerifyFrame { float x, y, p, q, r; bool live; };
HS_VERIFY_HD VerifyFrame verify_frame(float x, float y, float a, float b, float c)
{
   VerifyFrame f;
   f.x = x; f.y = y;
   f.r = sqrtf(c);
   f.q = b / f.r;
   const float qq = f.q * f.q;
   const float t = a - qq;
   f.p = sqrtf(t);
   f.live = c > 0.0f && t > 0.0f && f.p >= HS_VERIFY_MIN_AXIS && f.p <= HS_VERIFY_MAX_AXIS && f.r >= HS_VERIFY_MIN_AXIS && f.r <= HS_VERIFY_MAX_AXIS &&
            a <= HS_VERIFY_MAX_A && fabsf(x) <= HS_VERIFY_MAX_COORD && fabsf(y) <= HS_VERIFY_MAX_COORD;
   return f;
}

// hypothesis h of step 3 from the frames of its two keys
struct VerifyMap { float L11, L21, L22; };
HS_VERIFY_HD VerifyMap verify_map(float pq, float qq, float rq, float pd, float qd, float rd)
{
   VerifyMap m;
   m.L11 = pq / pd;
   m.L22 = rq / rd;
   const float s = qd * m.L11;
   const float d = qq - s;
   m.L21 = d / rd;
   return m;
}

// the best hypothesis as one integer that orders as (inliers descending, h ascending) does: inl(h) >= 1, so 0 is "no hypothesis"
HS_VERIFY_HD unsigned long long verify_best_key(uint32_t inliers, uint32_t h) { return ((unsigned long long)inliers << 32) | (unsigned long long)(0xffffffffu - h); }
HS_VERIFY_HD uint32_t verify_best_inliers(unsigned long long key) { return (uint32_t)(key >> 32); }
HS_VERIFY_HD int32_t verify_best_h(unsigned long long key) { return key == 0ull ? -1 : (int32_t)(0xffffffffu - (uint32_t)(key & 0xffffffffull)); }

// ---- the result of a call: stays in the context until the next call (hesaff_verify_get_pairs reads `pairs`) ----
constexpr int HS_VERIFY_PAIR_FLOATS = 10;   // xq, yq, pq, qq, rq, xd, yd, pd, qd, rd: hesaff_stage_verify_pairs' row
struct VerifyResultArrays {
   Span<int32_t> pairs;    // [R][4096][2]: the used correspondences (i, j) in definition order
   Span<int32_t> out;      // [R][6]
   Span<float> hyp;        // [R][3]
   Span<int32_t> order;    // [R]
   Span<uint32_t> qinert;  // [1]: the query's inert keys
};
inline VerifyResultArrays verify_result_arrays(StagePlan &p, int64_t n_candidates)
{
   VerifyResultArrays a;
   a.pairs = p.add<int32_t>((size_t)n_candidates * HS_VERIFY_MAX_USED * 2);
   a.out = p.add<int32_t>((size_t)n_candidates * 6);
   a.hyp = p.add<float>((size_t)n_candidates * 3);
   a.order = p.add<int32_t>((size_t)n_candidates);
   a.qinert = p.add<uint32_t>(1);
   return a;
}

// ---- the scratch of a call, released before the call returns ----
struct VerifyScratchArrays {
   Span<unsigned long long> hash_keys;   // [slots]: HS_INDEX_EMPTY or index_key(candidate, word)
   Span<uint32_t> hash_tf;               // [slots]: tf_r(w) over the live keys
   Span<uint32_t> starts;                // [R + 1]: candidate r's keys are rows[starts[r] .. starts[r + 1])
   Span<uint32_t> tfq;                   // [k]: live query keys per word
   Span<uint32_t> offsets;               // [k + 1]: word w's live query keys are members[offsets[w] .. offsets[w + 1])
   Span<uint32_t> cursor;                // [k]
   Span<uint32_t> members;               // [nq]
   Span<uint32_t> block_sums;            // the scan's
   Span<uint32_t> inert;                 // [R]
   Span<uint32_t> found;                 // [R]
   Span<uint32_t> used;                  // [R]: M_r
   Span<unsigned long long> best;        // [R]: verify_best_key, 0 where M_r = 0
   Span<float> corr;                     // [R][4096][10]: the used correspondences as the hypothesis kernel reads them
   uint64_t slots;
   int bits;
};
inline VerifyScratchArrays verify_scratch_arrays(StagePlan &p, int64_t n_candidates, int64_t k, int64_t nq, int64_t total_keys)
{
   VerifyScratchArrays s;
   s.bits = index_hash_bits(total_keys);
   s.slots = (uint64_t)1 << s.bits;
   s.hash_keys = p.add<unsigned long long>((size_t)s.slots);
   s.hash_tf = p.add<uint32_t>((size_t)s.slots);
   s.starts = p.add<uint32_t>((size_t)n_candidates + 1);
   s.tfq = p.add<uint32_t>((size_t)k);
   s.offsets = p.add<uint32_t>((size_t)k + 1);
   s.cursor = p.add<uint32_t>((size_t)k);
   s.members = p.add<uint32_t>((size_t)(nq > 0 ? nq : 1));
   s.block_sums = p.add<uint32_t>(((size_t)k + 4095) / 4096 + 1);
   s.inert = p.add<uint32_t>((size_t)n_candidates);
   s.found = p.add<uint32_t>((size_t)n_candidates);
   s.used = p.add<uint32_t>((size_t)n_candidates);
   s.best = p.add<unsigned long long>((size_t)n_candidates);
   s.corr = p.add<float>((size_t)n_candidates * HS_VERIFY_MAX_USED * HS_VERIFY_PAIR_FLOATS);
   return s;
}
// the bytes a call holds at its peak beside the caller's rows (R = 1024, k = 2^20, nq = 2^18, T = 2^28: 6.2 GiB, of which the hash
// table is 6; the host form adds the staged rows, 24 (T + nq) bytes)
inline size_t verify_working_set_bytes(int64_t n_candidates, int64_t k, int64_t nq, int64_t total_keys)
{
   StagePlan a, b;
   verify_result_arrays(a, n_candidates);
   verify_scratch_arrays(b, n_candidates, k, nq, total_keys);
   return a.bytes() + b.bytes();
}

} // namespace hesaff_plan
