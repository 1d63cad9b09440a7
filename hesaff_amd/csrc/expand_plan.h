// expand_plan.h -- the host arithmetic of query expansion (hesaff_expand_query, include/hesaff_amd.h): which calls are refused, which
// candidates are selected and in which order, the back-projection of a key and the rule that keeps it - ONE function, which the
// kernels of kernels_expand.h, the host and tests/native/expand_plan_check.cpp all call - the table of 64-row tiles the kernels walk,
// and where the arrays of a call lie in its buffer.  Pure functions and plain structs, no HIP (tests/test_query_expansion_host.py).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "buffer_layouts.h"   // StagePlan, Span
#include "verify_plan.h"      // VerifyRow, verify_frame and the bounds of a verify call

namespace hesaff_plan {

constexpr int64_t HS_EXPAND_MAX_IMAGES = 1024;              // max_images: at most every candidate of a verify call
constexpr int64_t HS_EXPAND_MAX_ROWS = (int64_t)1 << 18;    // max_rows: the query limit of the index and of the verifier
constexpr float HS_EXPAND_MAX_ROI = 0x1p20f;                // |roi[i]| <= 2^20: the coordinate bound of a live key
constexpr float HS_EXPAND_MIN_SCALE = 0x1p-40f;             // 2^-40 <= L11, L22 <= 2^40 and |L21| <= 2^81: the range of the maps that
constexpr float HS_EXPAND_MAX_SCALE = 0x1p40f;              // hesaff_verify_matches can return (its Range paragraph)
constexpr float HS_EXPAND_MAX_SHEAR = 0x1p81f;
constexpr int HS_EXPAND_TILE = 64;                          // rows of a tile: one wavefront, one 64-bit mask

inline bool expand_finite(float v) { return v - v == 0.0f; }   // (false for a NaN and for an infinity)
inline bool expand_min_inliers_ok(int64_t v) { return v >= 1; }
inline bool expand_max_images_ok(int64_t v) { return v >= 1 && v <= HS_EXPAND_MAX_IMAGES; }
inline bool expand_max_rows_ok(int64_t nq, int64_t max_rows) { return nq >= 0 && nq <= max_rows && max_rows <= HS_EXPAND_MAX_ROWS; }
// roi = (x0, y0, x1, y1): finite, inside the coordinate bound, not inverted (every test false for a NaN)
inline bool expand_roi_ok(const float *roi)
{
   for (int i = 0; i < 4; i++)
      if (!(expand_finite(roi[i]) && std::fabs(roi[i]) <= HS_EXPAND_MAX_ROI)) return false;
   return roi[0] <= roi[2] && roi[1] <= roi[3];
}
HS_VERIFY_HD bool expand_map_ok(float L11, float L21, float L22)
{
   return L11 >= HS_EXPAND_MIN_SCALE && L11 <= HS_EXPAND_MAX_SCALE && L22 >= HS_EXPAND_MIN_SCALE && L22 <= HS_EXPAND_MAX_SCALE && fabsf(L21) <= HS_EXPAND_MAX_SHEAR;
}

// what a selected candidate's keys are back-projected with: its two anchors and its map
struct ExpandAnchor { float xq, yq, xd, yd, L11, L21, L22; };
struct ExpandRoi { float x0, y0, x1, y1; };

// Steps 2 and 3 of the definition for one key of a selected candidate: the row it becomes in the query's frame, and whether it is
// live and kept.  One operation per statement, left to right, so that nothing is contracted; / is the IEEE division.  u is finite
// (|dx| <= 2^21, L11 >= 2^-40); t, s, v and y may be infinite, never NaN; a and b may be NaN, which verify_frame calls not live.
struct ExpandKey { float x, y, a, b, c; bool live, kept; };
HS_VERIFY_HD ExpandKey expand_key(const VerifyRow &k, const ExpandAnchor &A, const ExpandRoi &roi)
{
   ExpandKey e;
   e.live = verify_frame(k.x, k.y, k.a, k.b, k.c).live;
   const float dx = k.x - A.xd;
   const float dy = k.y - A.yd;
   const float u = dx / A.L11;
   const float t = A.L21 * u;
   const float s = dy - t;
   const float v = s / A.L22;
   e.x = A.xq + u;
   e.y = A.yq + v;
   const float m0 = k.a * A.L11;
   const float m1 = k.b * A.L21;
   const float e00 = m0 + m1;
   const float m2 = k.b * A.L11;
   const float m3 = k.c * A.L21;
   const float e10 = m2 + m3;
   const float e01 = k.b * A.L22;
   const float e11 = k.c * A.L22;
   const float n0 = A.L11 * e00;
   const float n1 = A.L21 * e10;
   e.a = n0 + n1;
   const float n2 = A.L11 * e01;
   const float n3 = A.L21 * e11;
   e.b = n2 + n3;
   e.c = A.L22 * e11;
   e.kept = e.live && e.x >= roi.x0 && e.x <= roi.x1 && e.y >= roi.y0 && e.y <= roi.y1 && verify_frame(e.x, e.y, e.a, e.b, e.c).live;
   return e;
}

// Step 1.  verify_out[R][6] and hyp[R][3] as hesaff_verify_matches returns them; rows(r, query_key, candidate_key, q, d) hands out the
// two anchor rows of candidate r (called with keys inside their ranges only).  `r` and `anchor` list the selected candidates in rank
// order; bad is the lowest eligible r that breaks a condition, or -1.  Of a candidate that is not eligible only the inlier count is read.
struct ExpandSelection {
   std::vector<int32_t> r;
   std::vector<ExpandAnchor> anchor;
   int64_t eligible = 0;
   int64_t bad = -1;
};
template <class ROWS>
ExpandSelection expand_select(const int32_t *verify_out, const float *hyp, const int32_t *counts, int64_t n_candidates, int64_t nq, int64_t min_inliers, int64_t max_images,
                              ROWS rows)
{
   ExpandSelection s;
   std::vector<int32_t> eligible;
   std::vector<ExpandAnchor> anchors((size_t)n_candidates);
   for (int64_t r = 0; r < n_candidates; r++) {
      const int32_t *o = verify_out + r * 6;
      if ((int64_t)o[0] < min_inliers) continue;
      const float *L = hyp + r * 3;
      if (o[3] < 0 || (int64_t)o[3] >= nq || o[4] < 0 || o[4] >= counts[r] || !expand_map_ok(L[0], L[1], L[2])) { s.bad = r; return s; }
      VerifyRow q, d;
      rows(r, o[3], o[4], q, d);
      if (!verify_frame(q.x, q.y, q.a, q.b, q.c).live || !verify_frame(d.x, d.y, d.a, d.b, d.c).live) { s.bad = r; return s; }
      anchors[(size_t)r] = {q.x, q.y, d.x, d.y, L[0], L[1], L[2]};
      eligible.push_back((int32_t)r);
   }
   s.eligible = (int64_t)eligible.size();
   std::stable_sort(eligible.begin(), eligible.end(), [&](int32_t a, int32_t b) { return verify_out[(int64_t)a * 6] > verify_out[(int64_t)b * 6]; });
   if ((int64_t)eligible.size() > max_images) eligible.resize((size_t)max_images);
   s.r = eligible;
   for (int32_t r : s.r) s.anchor.push_back(anchors[(size_t)r]);
   return s;
}

// The tiles of the selected candidates in rank order: candidate s owns the tiles prefix[s] .. prefix[s + 1) of HS_EXPAND_TILE
// consecutive rows each, the last one partly filled; its rows begin at row start[s] of the array the kernels read - the caller's
// concatenation (packed = false), or the selected candidates' rows alone, one behind the other in rank order (packed = true).
struct ExpandCand { ExpandAnchor a; uint32_t start, count, r; };
static_assert(sizeof(ExpandCand) == 40, "ten 4-byte words");
struct ExpandTiles {
   std::vector<ExpandCand> cand;    // [E]
   std::vector<uint32_t> prefix;    // [E + 1]
   uint32_t tiles = 0;              // prefix[E]: at most 1024 * 4096 = 2^22
   uint64_t rows = 0;               // the rows of the selected candidates: at most 2^28
};
inline uint32_t expand_tiles_of(int64_t count) { return (uint32_t)((count + HS_EXPAND_TILE - 1) / HS_EXPAND_TILE); }
inline ExpandTiles expand_tiles(const ExpandSelection &sel, const int32_t *counts, int64_t n_candidates, bool packed)
{
   ExpandTiles t;
   std::vector<uint64_t> starts((size_t)n_candidates + 1, 0);
   for (int64_t r = 0; r < n_candidates; r++) starts[(size_t)r + 1] = starts[(size_t)r] + (uint64_t)counts[r];
   t.prefix.push_back(0);
   for (size_t s = 0; s < sel.r.size(); s++) {
      const int32_t r = sel.r[s];
      ExpandCand c;
      c.a = sel.anchor[s];
      c.start = (uint32_t)(packed ? t.rows : starts[(size_t)r]);
      c.count = (uint32_t)counts[r];
      c.r = (uint32_t)r;
      t.cand.push_back(c);
      t.rows += (uint64_t)counts[r];
      t.tiles += expand_tiles_of(counts[r]);
      t.prefix.push_back(t.tiles);
   }
   return t;
}
// the candidate of a tile: the s with prefix[s] <= tile < prefix[s + 1] (a candidate without rows repeats a prefix and is never found);
// tile < prefix[n_selected]
HS_VERIFY_HD uint32_t expand_tile_owner(const uint32_t *prefix, uint32_t n_selected, uint32_t tile)
{
   uint32_t lo = 0, hi = n_selected;
   while (hi - lo > 1u) {
      const uint32_t mid = (lo + hi) >> 1;
      if (prefix[mid] <= tile) lo = mid; else hi = mid;
   }
   return lo;
}
// the rows a call's outputs must hold: what it can write at most
inline int64_t expand_output_rows(int64_t nq, uint64_t selected_rows, int64_t max_rows) { return (int64_t)std::min<uint64_t>((uint64_t)max_rows, (uint64_t)nq + selected_rows); }

// ---- the scratch of a call, released before the call returns ----
constexpr int HS_EXPAND_INFO = 3;   // live, kept, written per selected candidate
struct ExpandScratchArrays {
   Span<ExpandCand> cand;             // [E]
   Span<uint32_t> prefix;             // [E + 1]
   Span<unsigned long long> mask;     // [tiles]: bit l = row l of the tile is kept
   Span<uint32_t> base;               // [tiles + 1]: the kept rows before the tile; the last entry is kept_total
   Span<uint32_t> block_sums;         // the scan's
   Span<uint32_t> info;               // [E][3]
};
inline ExpandScratchArrays expand_scratch_arrays(StagePlan &p, int64_t n_selected, uint32_t tiles)
{
   ExpandScratchArrays s;
   s.cand = p.add<ExpandCand>((size_t)std::max<int64_t>(n_selected, 1));
   s.prefix = p.add<uint32_t>((size_t)n_selected + 1);
   s.mask = p.add<unsigned long long>((size_t)std::max<uint32_t>(tiles, 1u));
   s.base = p.add<uint32_t>((size_t)tiles + 1);
   s.block_sums = p.add<uint32_t>(((size_t)tiles + 4095) / 4096 + 1);
   s.info = p.add<uint32_t>((size_t)std::max<int64_t>(n_selected, 1) * HS_EXPAND_INFO);
   return s;
}
// what the host form stages beside the scratch: the selected candidates' rows (and signatures), and the three outputs
struct ExpandStagedArrays {
   Span<VerifyRow> rows;              // [selected rows]
   Span<unsigned long long> sigs;     // [selected rows] or empty
   Span<VerifyRow> rows_out;          // [out_rows]
   Span<int32_t> words_out;           // [out_rows]
   Span<unsigned long long> sigs_out; // [out_rows] or empty
};
inline ExpandStagedArrays expand_staged_arrays(StagePlan &p, uint64_t selected_rows, int64_t out_rows, bool with_sigs)
{
   ExpandStagedArrays a;
   a.rows = p.add<VerifyRow>((size_t)selected_rows);
   a.sigs = p.add<unsigned long long>(with_sigs ? (size_t)selected_rows : 0);
   a.rows_out = p.add<VerifyRow>((size_t)out_rows);
   a.words_out = p.add<int32_t>((size_t)out_rows);
   a.sigs_out = p.add<unsigned long long>(with_sigs ? (size_t)out_rows : 0);
   return a;
}
// the bytes a device-form call holds at its peak beside the caller's arrays (E = 1024 candidates of 2^18 rows: 2^22 tiles, 48.1 MiB,
// of which the masks are 32); the host form adds expand_staged_arrays: 24 (+ 8) bytes per selected row and 28 (+ 8) per output row
inline size_t expand_working_set_bytes(int64_t n_selected, uint32_t tiles)
{
   StagePlan p;
   expand_scratch_arrays(p, n_selected, tiles);
   return p.bytes();
}

} // namespace hesaff_plan
