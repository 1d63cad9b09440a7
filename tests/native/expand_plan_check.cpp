// expand_plan_check.cpp -- the host arithmetic of query expansion (hesaff_amd/csrc/expand_plan.h) on the CPU: every bound on both sides,
// the selection with ties, equality and the max_images cut, a broken eligible candidate named and a broken one that is not eligible
// accepted, the back-projection at its extremes, the tile table, the layouts and the working set of the largest call.
// tests/test_query_expansion_host.py builds it with AddressSanitizer + UBSan and runs it.
#include <cfenv>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../hesaff_amd/csrc/expand_plan.h"

using namespace hesaff_plan;

static int g_failed = 0;
#define CHECK(cond, ...)                                  \
   do {                                                   \
      if (!(cond)) {                                      \
         g_failed++;                                      \
         fprintf(stderr, "FAILED %s:%d: %s  ", __FILE__, __LINE__, #cond); \
         fprintf(stderr, __VA_ARGS__);                    \
         fprintf(stderr, "\n");                           \
      }                                                   \
   } while (0)

static const float INF = std::numeric_limits<float>::infinity(), NaN = std::numeric_limits<float>::quiet_NaN();
static float up(float v) { return std::nextafterf(v, INF); }
static float down(float v) { return std::nextafterf(v, -INF); }

static void check_bounds()
{
   CHECK(expand_min_inliers_ok(1) && expand_min_inliers_ok(1 << 30) && !expand_min_inliers_ok(0) && !expand_min_inliers_ok(-1), "min_inliers >= 1");
   CHECK(expand_max_images_ok(1) && expand_max_images_ok(1024) && !expand_max_images_ok(0) && !expand_max_images_ok(1025) && !expand_max_images_ok(-1), "max_images in 1 .. 1024");
   const int64_t M = (int64_t)1 << 18;
   CHECK(expand_max_rows_ok(0, 0) && expand_max_rows_ok(5, 5) && expand_max_rows_ok(0, M) && expand_max_rows_ok(M, M), "nq <= max_rows <= 2^18");
   CHECK(!expand_max_rows_ok(5, 4) && !expand_max_rows_ok(0, M + 1) && !expand_max_rows_ok(-1, 4) && !expand_max_rows_ok(0, -1), "max_rows below nq or above 2^18");
   const float B = 1048576.0f;
   const float ok[4] = {-B, -B, B, B}, point[4] = {3, 4, 3, 4};
   CHECK(expand_roi_ok(ok) && expand_roi_ok(point), "the largest region and a single point");
   for (int i = 0; i < 4; i++) {
      for (float bad : {NaN, INF, -INF, up(B), down(-B)}) {
         float r[4] = {-1, -1, 1, 1};
         r[i] = bad;
         CHECK(!expand_roi_ok(r), "roi[%d] = %g", i, (double)bad);
      }
   }
   const float xinv[4] = {up(1.0f), 0, 1, 1}, yinv[4] = {0, up(1.0f), 1, 1};
   CHECK(!expand_roi_ok(xinv) && !expand_roi_ok(yinv), "an inverted region");
   const float lo = std::ldexp(1.0f, -40), hi = std::ldexp(1.0f, 40), sh = std::ldexp(1.0f, 81);
   CHECK(HS_EXPAND_MIN_SCALE == lo && HS_EXPAND_MAX_SCALE == hi && HS_EXPAND_MAX_SHEAR == sh && HS_EXPAND_MAX_ROI == B, "the powers of two of the definition");
   CHECK(expand_map_ok(lo, sh, hi) && expand_map_ok(hi, -sh, lo) && expand_map_ok(1, 0, 1), "the map at its bounds");
   CHECK(!expand_map_ok(down(lo), 0, 1) && !expand_map_ok(up(hi), 0, 1) && !expand_map_ok(1, 0, down(lo)) && !expand_map_ok(1, 0, up(hi)) && !expand_map_ok(1, up(sh), 1) &&
            !expand_map_ok(1, -up(sh), 1),
         "the map one step outside");
   CHECK(!expand_map_ok(NaN, 0, 1) && !expand_map_ok(1, NaN, 1) && !expand_map_ok(1, 0, NaN) && !expand_map_ok(0, 0, 1) && !expand_map_ok(-1, 0, 1) && !expand_map_ok(1, INF, 1),
         "a NaN, a zero, a negative scale, an infinite shear");
}

static VerifyRow row(float x, float y, float a = 1, float b = 0, float c = 1, uint32_t w = 0) { return {x, y, a, b, c, w}; }

static void check_selection()
{
   // six candidates of three rows; the query has four rows; row 2 of every array is inert
   const int R = 6, nq = 4;
   std::vector<VerifyRow> q = {row(0, 0), row(1, 1), row(2, 2, NaN), row(3, 3)};
   std::vector<VerifyRow> c = {row(5, 5), row(6, 6), row(7, 7, 1, 0, 0)};
   const int32_t counts[R] = {3, 3, 3, 3, 0, 3};
   auto rows = [&](int64_t, int32_t qk, int32_t ck, VerifyRow &a, VerifyRow &d) { a = q[(size_t)qk]; d = c[(size_t)ck]; };
   //                          inliers, used, found, query_key, candidate_key, inert
   std::vector<int32_t> out = {5, 9, 9, 0, 0, 1,   7, 9, 9, 1, 1, 1,   5, 9, 9, 3, 0, 1,   2, 9, 9, 0, 0, 1,   0, 0, 0, -1, -1, 0,   7, 9, 9, 0, 1, 1};
   std::vector<float> hyp = {1, 0, 1,   2, 0.5f, 2,   1, 0, 1,   NaN, NaN, NaN,   NaN, INF, -1,   0.5f, -3, 4};
   ExpandSelection s = expand_select(out.data(), hyp.data(), counts, R, nq, 3, 1024, rows);
   CHECK(s.bad == -1 && s.eligible == 4 && s.r == std::vector<int32_t>({1, 5, 0, 2}), "ties by position; the candidates below min_inliers may hold NaN maps and -1 keys");
   CHECK(s.anchor.size() == 4 && s.anchor[0].xq == 1 && s.anchor[0].xd == 6 && s.anchor[0].L21 == 0.5f && s.anchor[3].xq == 3 && s.anchor[3].yd == 5, "the anchors in rank order");
   s = expand_select(out.data(), hyp.data(), counts, R, nq, 5, 1024, rows);
   CHECK(s.bad == -1 && s.r == std::vector<int32_t>({1, 5, 0, 2}), "min_inliers equal to a count: eligible");
   s = expand_select(out.data(), hyp.data(), counts, R, nq, 6, 1024, rows);
   CHECK(s.bad == -1 && s.r == std::vector<int32_t>({1, 5}), "min_inliers one above");
   s = expand_select(out.data(), hyp.data(), counts, R, nq, 3, 3, rows);
   CHECK(s.bad == -1 && s.eligible == 4 && s.r == std::vector<int32_t>({1, 5, 0}), "max_images cuts the weakest, of equals the later one");
   s = expand_select(out.data(), hyp.data(), counts, R, nq, 8, 1, rows);
   CHECK(s.bad == -1 && s.r.empty() && s.anchor.empty(), "nothing eligible");
   s = expand_select(out.data(), hyp.data(), counts, R, nq, 2, 1024, rows);
   CHECK(s.bad == 3 && s.r.empty(), "candidate 3 becomes eligible with its NaN map: named");
   // every way an eligible candidate can be broken, on candidate 2; candidate 0 stays sound
   struct Bad { int field; int32_t key; int hfield; float h; };
   const Bad bads[] = {{3, -1, -1, 0}, {3, nq, -1, 0}, {4, -1, -1, 0}, {4, 3, -1, 0}, {3, 2, -1, 0}, {4, 2, -1, 0},
                       {-1, 0, 0, NaN}, {-1, 0, 0, down(std::ldexp(1.0f, -40))}, {-1, 0, 2, up(std::ldexp(1.0f, 40))}, {-1, 0, 1, -up(std::ldexp(1.0f, 81))}, {-1, 0, 2, 0.0f}};
   for (const Bad &b : bads) {
      std::vector<int32_t> o = out;
      std::vector<float> h = hyp;
      if (b.field >= 0) o[2 * 6 + (size_t)b.field] = b.key;
      if (b.hfield >= 0) h[2 * 3 + (size_t)b.hfield] = b.h;
      s = expand_select(o.data(), h.data(), counts, R, nq, 3, 1, rows);
      CHECK(s.bad == 2, "field %d key %d hyp %d: bad %lld (an eligible candidate is checked even where max_images cuts it)", b.field, b.key, b.hfield, (long long)s.bad);
   }
   {  // an eligible candidate without rows has no key inside its range
      std::vector<int32_t> o = out;
      o[4 * 6] = 9; o[4 * 6 + 3] = 0; o[4 * 6 + 4] = 0;
      std::vector<float> h = hyp;
      h[4 * 3] = 1; h[4 * 3 + 1] = 0; h[4 * 3 + 2] = 1;
      s = expand_select(o.data(), h.data(), counts, R, nq, 3, 1024, rows);
      CHECK(s.bad == 4, "candidate_key 0 of no rows");
   }
}

static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

static void check_back_projection()
{
   const ExpandRoi all = {-1048576.0f, -1048576.0f, 1048576.0f, 1048576.0f};
   {  // the anchor maps onto the query's anchor exactly, under any map; a dyadic map by hand
      const ExpandAnchor A = {10.5f, -3.25f, 100, 200, 0.5f, 0.25f, 2};
      ExpandKey e = expand_key(row(100, 200, 4, 1, 2), A, all);
      CHECK(e.live && e.kept && same(e.x, 10.5f) && same(e.y, -3.25f), "the anchor: %g %g", (double)e.x, (double)e.y);
      // E' = L^T E L, L = [[.5, 0], [.25, 2]], E = [[4, 1], [1, 2]]: e00 = 2.25, e10 = 1, e01 = 2, e11 = 4 -> a' = 1.375, b' = 2, c' = 8
      CHECK(e.a == 1.375f && e.b == 2.0f && e.c == 8.0f, "the ellipse: %g %g %g", (double)e.a, (double)e.b, (double)e.c);
      // dx = 3, dy = 5: u = 6, t = 1.5, s = 3.5, v = 1.75
      e = expand_key(row(103, 205, 4, 1, 2), A, all);
      CHECK(e.kept && e.x == 16.5f && e.y == -1.5f, "a key: %g %g", (double)e.x, (double)e.y);
   }
   {  // the region's edges are inside, the next float is outside
      const ExpandAnchor I = {0, 0, 0, 0, 1, 0, 1};
      const ExpandRoi roi = {2, 3, 7, 9};
      CHECK(expand_key(row(2, 3), I, roi).kept && expand_key(row(7, 9), I, roi).kept && expand_key(row(2, 9), I, roi).kept, "on the edges");
      CHECK(!expand_key(row(down(2), 3), I, roi).kept && !expand_key(row(up(7), 3), I, roi).kept && !expand_key(row(2, down(3)), I, roi).kept &&
               !expand_key(row(2, up(9)), I, roi).kept,
            "one step outside");
      const ExpandKey e = expand_key(row(down(2), 3), I, roi);
      CHECK(e.live && !e.kept, "dropped by the region, still live");
      CHECK(!expand_key(row(4, 4, NaN), I, roi).live && !expand_key(row(NaN, 4), I, roi).kept && !expand_key(row(4, 4, 1, 0, NaN), I, roi).kept, "an inert key is not kept");
   }
   // the extremes: none traps (the floating-point exceptions are masked; UBSan watches the rest), none is kept, x is finite
   std::feclearexcept(FE_ALL_EXCEPT);
   const float B = 1048576.0f, lo = std::ldexp(1.0f, -40), sh = std::ldexp(1.0f, 81), A40 = std::ldexp(1.0f, 40);
   for (float shear : {sh, -sh}) {
      for (float dx : {2 * B, -2 * B}) {
         const ExpandAnchor X = {0, 0, dx > 0 ? -B : B, B, lo, shear, lo};
         const ExpandKey e = expand_key(row(dx > 0 ? B : -B, -B), X, all);
         CHECK(e.live && !e.kept, "L11 = 2^-40, |dx| = 2^21, L21 = +-2^81");
         CHECK(std::fabs(e.x) == std::ldexp(1.0f, 61) && std::isinf(e.y) && !std::isnan(e.y), "u = 2^61, v infinite, no NaN: %g %g", (double)e.x, (double)e.y);
      }
   }
   {  // a' = n0 + n1 with n0 = +inf and n1 = -inf: NaN, not kept
      const ExpandAnchor X = {0, 0, 0, 0, A40, -sh, 1};
      const ExpandKey e = expand_key(row(0, 0, A40, 1000, 1000000), X, all);
      CHECK(e.live && !e.kept && std::isnan(e.a), "an a' that overflows to NaN: %g", (double)e.a);
      CHECK(e.x == 0 && e.y == 0, "its centre is the anchor");
   }
   {  // the largest ellipse under the largest scale: a' = 2^120 is finite and beyond the verifier's bound, not kept
      const ExpandAnchor X = {0, 0, 0, 0, A40, 0, A40};
      const ExpandKey e = expand_key(row(0, 0, A40, 0, A40), X, all);
      CHECK(e.live && !e.kept && e.a == std::ldexp(1.0f, 120) && e.c == std::ldexp(1.0f, 120), "a' = c' = 2^120: %g %g", (double)e.a, (double)e.c);
   }
}

static void check_tiles()
{
   const int32_t counts[7] = {0, 1, 63, 64, 65, 7, 262144};
   ExpandSelection sel;
   sel.r = {4, 0, 3, 1, 2, 6};   // candidate 5 is not selected
   sel.anchor.resize(6, ExpandAnchor{0, 0, 0, 0, 1, 0, 1});
   for (bool packed : {false, true}) {
      const ExpandTiles t = expand_tiles(sel, counts, 7, packed);
      CHECK(t.prefix == std::vector<uint32_t>({0, 2, 2, 3, 4, 5, 4101}) && t.tiles == 4101 && t.rows == 65 + 0 + 64 + 1 + 63 + 262144, "tiles of 65, 0, 64, 1, 63, 2^18 rows");
      const uint32_t unpacked[6] = {128, 0, 64, 0, 1, 200}, pk[6] = {0, 65, 65, 129, 130, 193};
      for (int s = 0; s < 6; s++) {
         CHECK(t.cand[s].start == (packed ? pk[s] : unpacked[s]) && t.cand[s].count == (uint32_t)counts[sel.r[s]] && t.cand[s].r == (uint32_t)sel.r[s], "candidate %d", s);
      }
      const uint32_t owner[8] = {0, 0, 2, 3, 4, 5, 5, 5}, tile[8] = {0, 1, 2, 3, 4, 5, 6, 4100};
      for (int i = 0; i < 8; i++) CHECK(expand_tile_owner(t.prefix.data(), 6, tile[i]) == owner[i], "the owner of tile %u (the candidate without rows owns none)", tile[i]);
   }
   CHECK(expand_tiles_of(0) == 0 && expand_tiles_of(1) == 1 && expand_tiles_of(63) == 1 && expand_tiles_of(64) == 1 && expand_tiles_of(65) == 2, "tiles of 0, 1, 63, 64, 65 rows");
   ExpandSelection none;
   const ExpandTiles e = expand_tiles(none, counts, 7, false);
   CHECK(e.tiles == 0 && e.rows == 0 && e.prefix == std::vector<uint32_t>({0}) && e.cand.empty(), "nothing selected");
   CHECK(expand_output_rows(5, 100, 50) == 50 && expand_output_rows(5, 10, 50) == 15 && expand_output_rows(5, 0, 5) == 5 &&
            expand_output_rows(1 << 18, (uint64_t)1 << 28, 1 << 18) == 1 << 18,
         "the rows of the outputs");
}

template <class T> static void inside(const Span<T> &s, size_t bytes, std::vector<std::pair<size_t, size_t>> &seen)
{
   if (s.count == 0) return;   // (an empty array occupies nothing)
   CHECK(s.off % 256 == 0 && s.off + s.bytes() <= bytes, "aligned and inside");
   for (const auto &o : seen) CHECK(s.bytes() == 0 || o.second == o.first || s.off >= o.second || s.off + s.bytes() <= o.first, "disjoint");
   seen.push_back({s.off, s.off + s.bytes()});
}

static void check_layouts()
{
   for (bool sigs : {false, true}) {
      StagePlan p;
      const ExpandScratchArrays s = expand_scratch_arrays(p, 3, 70);
      const ExpandStagedArrays h = expand_staged_arrays(p, 4000, 300, sigs);
      std::vector<std::pair<size_t, size_t>> seen;
      inside(s.cand, p.bytes(), seen); inside(s.prefix, p.bytes(), seen); inside(s.mask, p.bytes(), seen); inside(s.base, p.bytes(), seen);
      inside(s.block_sums, p.bytes(), seen); inside(s.info, p.bytes(), seen); inside(h.rows, p.bytes(), seen); inside(h.sigs, p.bytes(), seen);
      inside(h.rows_out, p.bytes(), seen); inside(h.words_out, p.bytes(), seen); inside(h.sigs_out, p.bytes(), seen);
      CHECK(s.cand.count == 3 && s.prefix.count == 4 && s.mask.count == 70 && s.base.count == 71 && s.info.count == 9 && s.block_sums.count == 2, "the scratch");
      CHECK(h.rows.count == 4000 && h.rows_out.count == 300 && h.words_out.count == 300 && h.sigs.count == (sigs ? 4000u : 0u) && h.sigs_out.count == (sigs ? 300u : 0u), "the staged arrays");
   }
   StagePlan p;
   const ExpandScratchArrays z = expand_scratch_arrays(p, 0, 0);
   CHECK(z.cand.count == 1 && z.prefix.count == 1 && z.mask.count == 1 && z.base.count == 1 && z.info.count == 3, "nothing selected: every array still has a place");
   // the largest call: 1024 candidates of 2^18 rows
   const uint32_t tiles = 1024u * 4096u;
   const size_t ws = expand_working_set_bytes(1024, tiles);
   CHECK(ws >= (size_t)tiles * 12 && ws <= (size_t)tiles * 12 + ((size_t)1 << 20), "the working set of the largest call: %zu bytes", ws);
}

int main()
{
   check_bounds();
   check_selection();
   check_back_projection();
   check_tiles();
   check_layouts();
   if (g_failed) { fprintf(stderr, "%d check(s) failed\n", g_failed); return 1; }
   printf("expand_plan_check ok\n");
   return 0;
}
