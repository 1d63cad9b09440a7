// CPU check of the batch plan's host arithmetic (hesaff_amd/csrc/batch_plan.h, and the device buffers' layouts of buffer_layouts.h; built and run by tests/test_batch_plan.py with
// g++ -fsanitize=address,undefined).  Three kinds of checks: properties that pin the behaviour without reference to the code under test
// (what the kernels read and write, taken from kernels_patch.h / kernels_keypoint.h and stated at each check), a few values worked
// out by hand, and the blur steps of an octave against the loops the step table replaced.  Prints "plan_check ok"; the first failed check prints a message and ends the program with exit code 1.
#include <cstdio>
#include <cstdlib>
#include <random>
#include "../../hesaff_amd/csrc/batch_plan.h"
#include "../../hesaff_amd/csrc/buffer_layouts.h"
#include "../../hesaff_amd/csrc/host_tables.h"

using namespace hesaff_plan;

#define CHECK(cond, ...)                                                     \
   do {                                                                      \
      if (!(cond)) {                                                         \
         fprintf(stderr, "plan_check: %s:%d: %s failed: ", __FILE__, __LINE__, #cond); \
         fprintf(stderr, __VA_ARGS__);                                       \
         fprintf(stderr, "\n");                                              \
         exit(1);                                                            \
      }                                                                      \
   } while (0)

static void check_octaves()
{
   {
      const PyramidGeom p = pyramid_geometry(120, 160, 0);
      const int rows[4] = {120, 60, 30, 15}, cols[4] = {160, 80, 40, 20}, pitch[4] = {192, 128, 64, 64}, wpr[4] = {3, 2, 1, 1};
      CHECK(p.oct.size() == 4, "160x120: %zu octaves", p.oct.size());
      long long base = 0;
      for (int o = 0; o < 4; o++) {
         const OctGeom &g = p.oct[o];
         CHECK(g.rows == rows[o] && g.cols == cols[o] && g.pitch == pitch[o] && g.words_per_row == wpr[o] && g.word_base == base,
               "octave %d: %dx%d pitch %d words %d base %lld", o, g.rows, g.cols, g.pitch, g.words_per_row, g.word_base);
         base += 3ll * rows[o] * wpr[o];
      }
      CHECK(p.words_per_image == 1575, "words_per_image %lld", p.words_per_image);   // 3 * (120*3 + 60*2 + 30 + 15)
   }
   CHECK(pyramid_geometry(120, 160, 1).oct.size() == 5, "160x120 upscaled");
   {
      const PyramidGeom p = pyramid_geometry(2160, 3840, 0);
      CHECK(p.oct.size() == 8 && p.oct.back().rows == 16 && p.oct.back().cols == 30, "UHD: %zu octaves", p.oct.size());
   }
   CHECK(pyramid_geometry(12, 12, 0).oct.empty() && pyramid_geometry(12, 13, 0).oct.empty() && pyramid_geometry(13, 12, 0).oct.empty(), "12x12, 13x12");
   CHECK(pyramid_geometry(13, 13, 0).oct.size() == 1, "13x13");
}

static void check_capacity()
{
   const uint32_t cap = keypoint_capacity(1, 120, 160, 40000.0);
   CHECK(cap == 4096, "cap %u", cap);
   CHECK(candidate_capacity(cap, 1, 120, 160) == 4864, "cand_cap %u", candidate_capacity(cap, 1, 120, 160));   // 4096 + 512 + 64 * (1 strip * 4 bands)
   CHECK(order_key_bits(120, 160) == 16, "key bits %d", order_key_bits(120, 160));                              // 3 * 19200 = 57600 <= 2^16
   const int Bs[3] = {1, 64, 256}, Hs[3] = {120, 1080, 2160}, Ws[3] = {160, 1920, 3840};
   for (int B : Bs)
      for (int i = 0; i < 3; i++) {
         const uint32_t c = keypoint_capacity(B, Hs[i], Ws[i], 40000.0);
         CHECK(c % 64 == 0 && candidate_capacity(c, B, Hs[i], Ws[i]) >= c, "B %d %dx%d cap %u", B, Ws[i], Hs[i], c);
      }
   int code = 0;
   try { (void)keypoint_capacity(256, 2160, 3840, 1.0e6); }   // 2.1e9 keypoints
   catch (const HsError &e) { code = e.code; }
   CHECK(code == HESAFF_ERR_ARG, "a request above 2e9 keypoints: code %d", code);
}

// ---- buffer_layouts.h: the carver, the lists of a context, the rank arrays, the descriptor scratch, the stage arenas ----
// One array of a buffer as the kernels index it: bytes [at, at + len).
struct Extent { const char *name; size_t at, len; };
// every array inside [0, bytes), at a multiple of `align`, and no two of one buffer overlapping
static void check_extents(const char *what, size_t size, const std::vector<Extent> &e, size_t bytes, size_t align)
{
   for (size_t i = 0; i < e.size(); i++) {
      CHECK(e[i].at <= bytes && e[i].len <= bytes - e[i].at, "%s (%zu): %s [%zu, +%zu) leaves the buffer's %zu bytes", what, size, e[i].name, e[i].at, e[i].len, bytes);
      CHECK(e[i].at % align == 0, "%s (%zu): %s at %zu is not %zu-byte aligned", what, size, e[i].name, e[i].at, align);
      for (size_t j = i + 1; j < e.size(); j++)
         CHECK(e[i].at + e[i].len <= e[j].at || e[j].at + e[j].len <= e[i].at, "%s (%zu): %s and %s overlap", what, size, e[i].name, e[j].name);
   }
}

static int carver_error(size_t end, size_t count, size_t align)
{
   Carver c;
   c.end = end;
   try { (void)c.take<float>(count, align); }
   catch (const HsError &e) { return e.code; }
   return 0;
}
static void check_carver()
{
   Carver c;
   CHECK(c.bytes() == 0 && c.take<uint8_t>(3) == 0 && c.bytes() == 3, "the first array starts at 0 and ends the carver");
   CHECK(c.take<float>(5) == 4 && c.bytes() == 24, "a float behind 3 bytes: at 4, its natural alignment");
   CHECK(c.take<float>(5, 256) == 256 && c.bytes() == 276, "an alignment request is honoured, bytes() is the end of the last array");
   CHECK(c.take<double>(0, 64) == 320 && c.bytes() == 276 && c.take<uint8_t>(0) == 276 && c.bytes() == 276, "a zero-count take occupies nothing");
   CHECK(c.take<uint8_t>(1) == 276 && c.bytes() == 277, "the array behind an empty one");
   // an end beyond SIZE_MAX: the count, the padding, or both
   CHECK(carver_error(0, SIZE_MAX / 4 + 1, 4) == HESAFF_ERR_ARG, "count * sizeof(T) wraps");
   CHECK(carver_error(SIZE_MAX - 10, 4, 4) == HESAFF_ERR_ARG, "end + bytes wraps");
   CHECK(carver_error(SIZE_MAX - 10, 0, 256) == HESAFF_ERR_ARG, "the padding wraps");
   CHECK(carver_error(SIZE_MAX - 19, 4, 4) == 0, "an array that ends at SIZE_MAX - 3 fits");
}

// The lists of a context over a keypoint capacity.  Extents: what the kernels index with h, slot, r < cap (cap itself is what the lists carry:
// RecList::cap, HessList::cap, PatchWork::cap).  Parent: the sizes plan_buffers wrote and the offsets make_lists wrote as literals before
// the layouts existed (pipeline.hip of commit 2c74b82, the lines named at each value) - equality with them is "nothing moved".
static void check_list_layouts(size_t cap)
{
   CHECK(cap % 64 == 0, "cap %zu: keypoint_capacity makes multiples of 64", cap);
   const RecLayout r = rec_layout(cap);
   // k_localize: rl.x[slot] .. rl.bit[slot], rl.word[slot] (long long), slot < rl.cap (kernels_pyramid.h:405-413)
   check_extents("b_rec_f", cap, {{"x", r.x, cap * 4}, {"y", r.y, cap * 4}, {"s", r.s, cap * 4}, {"response", r.response, cap * 4}}, r.f_bytes, 16);
   check_extents("b_rec_i", cap, {{"meta", r.meta, cap * 4}, {"cell", r.cell, cap * 4}, {"key", r.key, cap * 4}, {"bit", r.bit, cap * 4}}, r.i_bytes, 16);
   check_extents("b_rec_w", cap, {{"word", r.word, cap * 8}}, r.w_bytes, 16);
   CHECK(r.f_bytes == cap * 16, "b_rec_f %zu bytes", r.f_bytes);                                                            // :600  cap * 4 * 4
   CHECK(r.i_bytes == cap * 16, "b_rec_i %zu bytes", r.i_bytes);                                                            // :601  cap * 4 * 4
   CHECK(r.w_bytes == cap * 8, "b_rec_w %zu bytes", r.w_bytes);                                                             // :602  cap * 8
   CHECK(r.x == 0 && r.y == cap * 4 && r.s == cap * 8 && r.response == cap * 12, "RecList floats moved");                   // :735  rf, rf + cap, rf + 2 * cap, rf + 3 * cap
   CHECK(r.meta == 0 && r.cell == cap * 4 && r.key == cap * 8 && r.bit == cap * 12 && r.word == 0, "RecList integers moved");   // :737-738  ri, ri + cap, ri + 2 * cap, ri + 3 * cap; word alone

   const HessLayout h = hess_layout(cap);
   // k_hess_deal: hl.x[r] .. hl.r0c0[r], r < hl.cap (kernels_pyramid.h:597-598)
   check_extents("b_hess_f", cap, {{"x", h.x, cap * 4}, {"y", h.y, cap * 4}, {"s", h.s, cap * 4}, {"response", h.response, cap * 4}}, h.f_bytes, 16);
   check_extents("b_hess_i", cap, {{"meta", h.meta, cap * 4}, {"r0c0", h.r0c0, cap * 4}}, h.i_bytes, 16);
   CHECK(h.f_bytes == cap * 16, "b_hess_f %zu bytes", h.f_bytes);                                                           // :603  cap * 4 * 4
   CHECK(h.i_bytes == cap * 8, "b_hess_i %zu bytes", h.i_bytes);                                                            // :604  cap * 2 * 4
   CHECK(h.x == 0 && h.y == cap * 4 && h.s == cap * 8 && h.response == cap * 12, "HessList floats moved");                  // :740  hf, hf + cap, hf + 2 * cap, hf + 3 * cap
   CHECK(h.meta == 0 && h.r0c0 == cap * 4, "HessList integers moved");                                                      // :742  hi, hi + cap

   const AffineLayout a = affine_layout(cap);
   // hs_affine_groups: out.converged[h], out.iters[h], out.U[4 * h + 3], h < cap (kernels_keypoint.h:124-125, 264-266)
   check_extents("b_aff", cap, {{"converged", a.converged, cap * 4}, {"iters", a.iters, cap * 4}, {"U", a.U, cap * 16}}, a.bytes, 16);
   CHECK(a.bytes == cap * 24, "b_aff %zu bytes", a.bytes);                                                                  // :605  cap * 6 * 4
   CHECK(a.converged == 0 && a.iters == cap * 4 && a.U == cap * 8, "AffineOut moved");                                      // :744  ai, ai + cap, ai + 2 * cap

   const PatchLayout p = patch_layout(cap);
   // hs_prepare_patch_body: pw.A[4 * h + 3], pw.alive[h], pw.P0[h], h < cap (kernels_keypoint.h:352, 366-367); the bins' lists
   // pw.bin_items[bq * cap + base + ..] below bin_items[(HS_NBINS - 1) * cap + cap - 1] (kernels_keypoint.h:385, kernels_patch.h:936)
   check_extents("b_pw", cap, {{"P0", p.P0, cap * 4}, {"alive", p.alive, cap * 4}, {"A", p.A, cap * 16}}, p.pw_bytes, 16);
   check_extents("b_bins", cap, {{"bin_items", p.bin_items, ((size_t)(HS_NBINS - 1) * cap + cap - 1 + 1) * 4}}, p.bins_bytes, 16);
   CHECK(p.pw_bytes == cap * 24, "b_pw %zu bytes", p.pw_bytes);                                                             // :606  cap * 6 * 4
   CHECK(p.bins_bytes == cap * HS_NBINS * 4, "b_bins %zu bytes", p.bins_bytes);                                             // :607  cap * HS_NBINS * 4
   CHECK(p.P0 == 0 && p.alive == cap * 4 && p.A == cap * 8 && p.bin_items == 0, "PatchWork moved");                         // :746-747  pi, pi + cap, pi + 2 * cap; b_bins whole
}

// The rank arrays of an orientation count K: OrientRanks' accessors reach rank K - 1, (K - 2) * cap entries in, and the kernels index a rank
// with h < cap - A_of(j) + 4 * h as one float4 (kernels_orient.h:197), alive_of(j)[h] (:188), P0_of(j) as PatchWork::P0 of the rank's pass
// (pipeline.hip: GroupDevice::lists), desc_of(j) + 128 * h as 32 words (:252) - so desc_of(K - 1) + cap * 128 is the end of the buffer.
static void check_rank_layout(int K, size_t cap)
{
   const RankLayout L = rank_layout(K, cap);
   const size_t n = (size_t)(K - 1) * cap, last = (size_t)(K - 2) * cap;
   check_extents("b_ori_ranks", cap, {{"A", L.A, (last + cap) * 16}, {"P0", L.P0, (last + cap) * 4}, {"alive", L.alive, (last + cap) * 4}, {"desc", L.desc, (last + cap) * 128}}, L.bytes, 16);
   CHECK(L.bytes == n * 152, "K %d cap %zu: %zu bytes", K, cap, L.bytes);                                                   // :860  (K - 1) * cap * 152
   CHECK(L.A == 0 && L.P0 == n * 16 && L.alive == n * 20 && L.desc == n * 24, "K %d cap %zu: the rank arrays moved", K, cap);   // :857  base, base + n * 16, + n * 20, + n * 24
}

// The descriptor stage's scratch for n keypoints: k_sift_meanvar reads io.patches + kp * HS_PATCH_PIX, HS_PATCH_PIX floats (kernels_sift.h:65),
// and writes io.meanvar[2 * kp + 1] (:86), kp < n; k_sift_grad writes HS_VO_ITEMS float4 = HS_VO_PITCH float2 at vo + k * HS_VO_PITCH (:199).
static void check_group_scratch(uint32_t n)
{
   const GroupScratch g = group_scratch(n);
   const size_t N = n;
   CHECK(g.patch_floats * 4 >= ((N - 1) * HS_PATCH_PIX + HS_PATCH_PIX) * 4, "n %u: patches", n);
   CHECK(g.meanvar_floats * 4 >= (2 * (N - 1) + 2) * 4, "n %u: mean / variance", n);
   CHECK(g.vo_floats * 4 >= ((N - 1) * HS_VO_PITCH + HS_VO_PITCH) * 8, "n %u: gradient pairs", n);
   CHECK(g.patch_floats * 4 == N * HS_PATCH_PIX * 4, "n %u: patches %zu floats", n, g.patch_floats);        // :1112  n * HS_PATCH_PIX * 4
   CHECK(g.meanvar_floats * 4 == N * 2 * 4, "n %u: mean / variance %zu floats", n, g.meanvar_floats);        // :1113  n * 2 * 4
   CHECK(g.vo_floats * 4 == N * HS_VO_PITCH * 8 + 64, "n %u: gradient pairs %zu floats", n, g.vo_floats);    // :1117  n * HS_VO_PITCH * 8 + 64
}

// The stage arenas (capi_stage.h: StageArena over StagePlan): the arrays every converted operator declares, restated here as {element
// size, count} from what its kernel indexes, against the bytes the operator asked of the stage buffer before the arena (capi_impl.h of
// commit 2c74b82): disjoint, 256-byte aligned, and at most 256 bytes per array more.  The plane operators run on 13 x 13.
struct ArenaArray { size_t elem, count; };
static void check_arena(const char *what, size_t n, const std::vector<ArenaArray> &arrays, size_t parent_bytes)
{
   StagePlan plan;
   std::vector<Extent> e;
   for (const ArenaArray &a : arrays) {
      const size_t at = a.elem == 1 ? plan.add<uint8_t>(a.count).off : plan.add<float>(a.count).off;
      CHECK(a.elem == 1 || a.elem == 4, "%s: element size %zu", what, a.elem);
      e.push_back({what, at, a.elem * a.count});
      CHECK(plan.bytes() == at + a.elem * a.count, "%s (%zu): bytes() is not the end of the last array", what, n);
   }
   check_extents(what, n, e, plan.bytes(), 256);
   CHECK(plan.bytes() <= parent_bytes + 256 * arrays.size(), "%s (%zu): %zu bytes, %zu before the arena", what, n, plan.bytes(), parent_bytes);
}
static void check_stage_arenas(size_t N)
{
   const size_t rows = 13, cols = 13, px = rows * 64 /* pitch: round_up(13, 64) */, np = rows * cols, K = 9;
   const size_t PIX = HS_PATCH_PIX, VO = HS_VO_PITCH;
   check_arena("gaussian_blur", N, {{4, px}, {4, px}, {4, px}, {4, K}}, px * 4 * 3 + (K + 16) * 4);           // in | tmp | out | taps
   check_arena("hessian_response", N, {{4, px}, {4, px}, {4, px}, {4, px}, {4, 9}}, px * 4 * 4 + 64);         // in | R0 | L1 | R1 | taps
   check_arena("half_image", N, {{4, np}, {4, (rows / 2) * (cols / 2)}}, np * 4 * 2);                         // in | out (k_half: rows / 2 x cols / 2)
   // k_affine_stage: the plane rows x cols tight, kp[4 * i + 3], converged[i], iters[i], U[4 * i + 3], i < n
   check_arena("find_affine_shape", N, {{4, np}, {4, 4 * N}, {4, N}, {4, N}, {4, 4 * N}}, np * 4 + N * (4 + 6) * 4 + 64);
   check_arena("rectify", N, {{4, 4 * N}}, N * 16);
   // launch_sift on n patches: group_scratch's three arrays, the flags, the histogram SiftIO::vec[128 * k + 127], the descriptors desc[128 * k + 127]
   const GroupScratch g = group_scratch((uint32_t)N);
   check_arena("sift", N, {{4, g.patch_floats}, {4, N}, {4, g.meanvar_floats}, {4, 128 * N}, {1, 128 * N}, {4, g.vo_floats}},
               ((N * PIX * 4 + N * 4 + N * 8 + N * 128 * 4 + N * 128 + 63) & ~(size_t)63) + N * VO * 8 + 64);
   // k_orientation: patches, theta[k], hist[36 * k + 35], cs[2 * k + 1]; k_orientation_peaks: patches, n_ori[k], bins[4 * k + 3], thetas[4 * k + 3]
   check_arena("orientation", N, {{4, N * PIX}, {4, N}, {4, 36 * N}, {4, 2 * N}}, N * PIX * 4 + N * 4 + N * 36 * 4 + N * 8);
   check_arena("orientation_peaks", N, {{4, N * PIX}, {4, N}, {4, 4 * N}, {4, 4 * N}}, N * PIX * 4 + N * 4 + N * 4 * 4 + N * 4 * 4);
   check_arena("fmt_g", N, {{4, N}, {4, N}, {1, 16 * N}}, N * (4 + 16 + 4));                                   // values | lengths | 16 characters each
   check_arena("math", N, {{4, N}, {4, N}, {4, N}, {4, N}}, N * 16);
   check_arena("math_sift", N, {{4, N}, {4, N}, {4, N}, {4, N}, {4, N}, {4, N}}, N * 24);
   check_arena("math_sift_general", N, {{4, N}, {4, N}, {4, N}, {4, N}, {4, N}}, N * 20);
   check_arena("assign_words", N, {{1, 128 * N}, {4, 2 * N}}, ((N * 128 + 255) & ~(size_t)255) + N * 8);       // descriptors | (word, dist2) per key
   check_arena("check_device_f32", N, {{4, N}}, N * 4);                                                        // one flag per image
}

static void check_layouts()
{
   const int Bs[4] = {1, 2, 64, 256};
   for (int B : Bs) {
      std::vector<uint32_t> mem(starts_block((uint32_t *)nullptr, B).words_allocated());
      const StartsBlock<uint32_t> sb = starts_block(mem.data(), B);
      // the four regions and their sizes: B + 1 starts twice, B row sums and the word behind them, one word
      const size_t at[4] = {(size_t)(sb.hess() - mem.data()), (size_t)(sb.desc() - mem.data()), (size_t)(sb.large_rows() - mem.data()),
                            (size_t)(sb.largest_window() - mem.data())};
      const size_t len[4] = {(size_t)B + 1, (size_t)B + 1, (size_t)B + 1, 1};
      for (int i = 0; i < 4; i++) {
         for (int j = i + 1; j < 4; j++) CHECK(at[i] + len[i] <= at[j] || at[j] + len[j] <= at[i], "B %d: regions %d and %d overlap", B, i, j);
         CHECK(at[i] + len[i] <= sb.words_to_copy(), "B %d: region %d lies outside the copied prefix", B, i);
      }
      CHECK(sb.largest_window() == sb.large_rows() + B + 1, "B %d: largest_window", B);
      CHECK(sb.words_to_copy() <= sb.words_allocated(), "B %d: the copy reads past the allocation", B);
      CHECK(sb.words_final() == at[2], "B %d: the end-of-batch copy is hess() and desc()", B);
      CHECK(at[2] + sb.words_to_clear() == at[3] + 1, "B %d: the clear ends with largest_window()", B);
   }
   // (the counter block's words are pinned by the static_asserts of batch_plan.h)
   CHECK(describe_records_offset(1) == 256 && describe_records_offset(63) == 256 && describe_records_offset(64) == 512, "describe_records_offset");
   check_carver();
   const size_t caps[3] = {64, 4096, keypoint_capacity(256, 2160, 3840, 40000.0)};
   for (size_t cap : caps) {
      check_list_layouts(cap);
      check_rank_layout(2, cap);
      check_rank_layout(4, cap);
   }
   const uint32_t ns[4] = {1, 3, 65, 1200000};
   for (uint32_t n : ns) check_group_scratch(n);
   for (size_t n : {(size_t)1, (size_t)3, (size_t)65}) check_stage_arenas(n);
}

// the properties of form_groups' result; they determine the greedy result
static void check_groups_of(const char *what, const std::vector<int32_t> &hs, const std::vector<uint32_t> &lrows, uint32_t trows_rows, size_t min_groups,
                            uint32_t kpts_lo, uint32_t kpts_hi)
{
   const int B = (int)lrows.size();
   const GroupPlan p = form_groups(hs.data(), lrows.data(), B, trows_rows);
   const uint32_t total = (uint32_t)hs[B];
   const uint32_t kpts = total / 16u < 300000u ? 300000u : (total / 16u > 1200000u ? 1200000u : total / 16u);
   CHECK(kpts >= kpts_lo && kpts <= kpts_hi, "%s: the case is meant for a keypoint limit in [%u, %u], not %u", what, kpts_lo, kpts_hi, kpts);
   std::vector<int> ne;   // images with keypoints
   for (int b = 0; b < B; b++)
      if (hs[b + 1] > hs[b]) ne.push_back(b);
   size_t k = 0;
   uint32_t max_n = 0;
   for (size_t gi = 0; gi < p.groups.size(); gi++) {
      const ImageGroup &g = p.groups[gi];
      CHECK(k < ne.size() && g.lo == (uint32_t)hs[ne[k]], "%s: group %zu does not start where the one before ended", what, gi);
      unsigned long long rows = 0;
      int count = 0;
      while (k < ne.size() && (uint32_t)hs[ne[k] + 1] <= g.hi) { rows += lrows[ne[k]]; count++; k++; }
      CHECK(count >= 1 && (uint32_t)hs[ne[k - 1] + 1] == g.hi, "%s: group %zu does not end at an image boundary", what, gi);
      CHECK(g.large_rows == rows, "%s: group %zu large_rows %u, its images' %llu", what, gi, g.large_rows, rows);
      CHECK(count == 1 || (g.hi - g.lo <= kpts && rows <= trows_rows), "%s: group %zu of %d images exceeds a limit", what, gi, count);
      if (k < ne.size())
         CHECK((uint32_t)hs[ne[k] + 1] - g.lo > kpts || rows + lrows[ne[k]] > trows_rows, "%s: group %zu could have taken the next image", what, gi);
      max_n = std::max(max_n, g.hi - g.lo);
   }
   CHECK(k == ne.size(), "%s: the groups end before the last image with keypoints", what);
   CHECK(p.max_n == max_n, "%s: max_n %u, largest group %u", what, p.max_n, max_n);
   CHECK(p.groups.size() >= min_groups, "%s: %zu groups, the case is meant to make %zu at least", what, p.groups.size(), min_groups);
}

static void check_groups()
{
   // counts[b] keypoints and rows[b] window rows per image (an image without keypoints has no rows)
   auto run = [](const char *what, const std::vector<uint32_t> &counts, std::vector<uint32_t> rows, uint32_t trows_rows, size_t min_groups,
                 uint32_t kpts_lo = 300000, uint32_t kpts_hi = 1200000) {
      std::vector<int32_t> hs(counts.size() + 1, 0);
      for (size_t b = 0; b < counts.size(); b++) {
         hs[b + 1] = hs[b] + (int32_t)counts[b];
         if (counts[b] == 0) rows[b] = 0;
      }
      check_groups_of(what, hs, rows, trows_rows, min_groups, kpts_lo, kpts_hi);
   };
   const uint32_t trows = 4u << 20;
   std::mt19937 rng(20261017);
   auto uni = [&](uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rng() % (hi - lo + 1)); };
   for (int round = 0; round < 20; round++) {
      {
         // 256 images, about 7 M keypoints (the limit is total / 16, between its clamps), images without keypoints at the front, in the middle, at the end
         std::vector<uint32_t> c(256), r(256);
         for (int b = 0; b < 256; b++) { c[b] = uni(0, 60000); r[b] = uni(0, 600000); }
         c[0] = c[1] = c[100] = c[101] = c[102] = c[254] = c[255] = 0;
         for (int z = 0; z < 10; z++) c[uni(0, 255)] = 0;
         run("empty images", c, r, trows, 8, 300001, 1199999);
      }
      {
         // one image above the limit's lower clamp (300 000) among small ones
         std::vector<uint32_t> c(64), r(64);
         for (int b = 0; b < 64; b++) { c[b] = uni(0, 20000); r[b] = uni(0, 2000); }
         c[uni(0, 63)] = 300001 + uni(0, 400000);
         run("one image above group_kpts", c, r, trows, 2, 300000, 300000);
      }
      {
         // one image whose rows alone exceed the row buffer
         std::vector<uint32_t> c(32), r(32);
         for (int b = 0; b < 32; b++) { c[b] = uni(1, 5000); r[b] = uni(0, 300000); }
         r[uni(0, 31)] = trows + 1 + uni(0, 1000000);
         run("one image above trows_rows", c, r, trows, 2);
      }
      {
         // above 19.2 M keypoints the limit is its upper clamp (1 200 000)
         std::vector<uint32_t> c(256), r(256);
         for (int b = 0; b < 256; b++) { c[b] = uni(60000, 140000); r[b] = uni(0, 100000); }
         run("upper clamp", c, r, trows, 16, 1200000, 1200000);
      }
   }
   // both limits are inclusive: three images with exactly 300 000 keypoints and exactly trows_rows rows are one group
   run("limits met exactly", {100000, 100000, 100000, 1}, {trows / 2, trows / 2, 0, 0}, trows, 2, 300000, 300000);
   run("no keypoints at all", std::vector<uint32_t>(7, 0), std::vector<uint32_t>(7, 0), trows, 0);
   run("one image", std::vector<uint32_t>(1, 123), std::vector<uint32_t>(1, 4000), trows, 1);
   run("one image, rows near 2^32", std::vector<uint32_t>(3, 10), std::vector<uint32_t>(3, 0xfffffff0u), trows, 3);
}

// What k_patch_large_rows needs of a launch that serves a window of side P (kernels_patch.h):
//  * each wavefront owns nrow * srow_stride + tap_stride floats of the dynamic LDS, its rows srow_stride apart;
//  * hs_row_stream / 2 / 3 store the P samples of a row at srow[r .. r + P), r = K / 2 replicated samples on either side
//    (srow[0 .. r) and srow[r + P .. r + P + r)), and read srow[x0 + jt + 1] for x0 <= P - 2, jt < K, i.e. up to index P + 2 r - 1:
//    a row needs P + 2 (K / 2) floats;
//  * K = tb.patch_tap_k[(P0 - 1) / 2], P0 = P - 2: gauss_ksize(1.5f * P0 / 41) (build_patch_taps, context_tables.h); the tap area holds K floats at most.
static void check_large_launch(int max_p0, int P, int batch_max_p, size_t optin)
{
   const LargeSplit sp = large_rows_split(max_p0, batch_max_p);
   int serves = -1;
   for (int i = 0; i < sp.n; i++)
      if (P > sp.p_lo[i] && P <= sp.p_hi[i]) { CHECK(serves < 0, "max_p0 %d P %d: two launches serve the window", max_p0, P); serves = i; }
   CHECK(serves >= 0, "max_p0 %d batch_max_p %d: no launch serves P %d", max_p0, batch_max_p, P);
   const LargeLaunch ll = large_rows_launch(sp.p_hi[serves], max_p0, (uint32_t)P);
   const int K = hesaff::gauss_ksize(1.5f * ((float)(P - 2) / (float)HS_PATCH));
   CHECK(ll.srow_stride >= P + 2 * (K / 2), "max_p0 %d P %d (launch up to %d): srow_stride %d < %d", max_p0, P, sp.p_hi[serves], ll.srow_stride, P + 2 * (K / 2));
   CHECK(ll.tap_stride >= K, "max_p0 %d P %d: tap_stride %d < K %d", max_p0, P, ll.tap_stride, K);
   CHECK(ll.lds_bytes <= 160 * 1024 && ll.lds_bytes <= optin, "max_p0 %d P %d: %zu bytes of LDS, opt-in %zu", max_p0, P, ll.lds_bytes, optin);
   CHECK(ll.wavefronts == 1 || ll.wavefronts == 2 || ll.wavefronts == 4, "max_p0 %d P %d: %u wavefronts", max_p0, P, ll.wavefronts);
   CHECK(ll.nrow == 1 || ll.nrow == 3, "max_p0 %d P %d: nrow %d", max_p0, P, ll.nrow);
   const size_t per_wave = ((size_t)ll.nrow * ll.srow_stride + ll.tap_stride) * 4;
   if (ll.nrow == 3) CHECK(ll.wavefronts <= HS_LARGE_NW && 6 * per_wave <= 160 * 1024, "max_p0 %d P %d: three-row form with %u wavefronts of %zu bytes", max_p0, P, ll.wavefronts, per_wave);
   CHECK(ll.lds_bytes == ll.wavefronts * per_wave, "max_p0 %d P %d: %zu bytes for %u wavefronts of %zu", max_p0, P, ll.lds_bytes, ll.wavefronts, per_wave);
   CHECK(ll.grid_blocks >= 1, "max_p0 %d P %d: empty grid", max_p0, P);
}

static void check_large()
{
   // the plan's refusal: exactly where one row of the largest window no longer fits the 160 KB of a CU
   int largest = 0;
   for (int max_p0 = 515; max_p0 <= 40000; max_p0++) {
      int code = 0;
      try { (void)large_rows_lds_optin(max_p0); }
      catch (const HsError &e) { code = e.code; }
      const LargeLaunch one = large_rows_launch(max_p0 + 2, max_p0, 1);   // of the largest window: one wavefront with one row at the least
      if (code == 0) {
         CHECK(largest == max_p0 - 1 || max_p0 == 515, "max_p0 %d accepted above a refused one", max_p0);
         CHECK(one.lds_bytes <= 160 * 1024, "max_p0 %d accepted, a row needs %zu bytes", max_p0, one.lds_bytes);
         largest = max_p0;
      } else {
         CHECK(code == HESAFF_ERR_ARG, "max_p0 %d: code %d", max_p0, code);
         CHECK(one.wavefronts == 1 && one.nrow == 1 && one.lds_bytes > 160 * 1024, "max_p0 %d refused, yet a row fits (%zu bytes)", max_p0, one.lds_bytes);
      }
   }
   CHECK(largest > 20000 && largest < 40000, "largest accepted max_p0 %d", largest);
   // every tap-table bound up to 3000, every 37th above, the largest; every window side each
   for (int max_p0 = 515; max_p0 <= largest; max_p0 += (max_p0 < 3000 || max_p0 + 37 > largest) ? 1 : 37) {
      const size_t optin = large_rows_lds_optin(max_p0);
      for (int P = HS_BIN3_PMAX + 1; P <= max_p0 + 2; P++) {
         check_large_launch(max_p0, P, P, optin);             // the window is the batch's largest
         check_large_launch(max_p0, P, max_p0 + 2, optin);    // the batch holds the largest the image allows
         check_large_launch(max_p0, P, 0, optin);             // the stage entry point before it knows
      }
   }
   // the host's row bound (hesaff_stage_normalize_affine): P = 2 ceil(s * mrSize) + 3 for windows above 512 whose taps are tabulated
   const float s[5] = {10.0f, 255.0f, 255.5f, 1000.0f, 3.0e6f};
   const LargeRows lr = host_large_rows(s, 5, 1.0f, 2001);   // P = 23, 513, 515, 2003, none
   CHECK(lr.rows == 513 + 515 + 2003 && lr.max_p == 2003, "host_large_rows: %u rows, largest %d", lr.rows, lr.max_p);
   CHECK(host_large_rows(s, 5, 1.0f, 2000).rows == 513 + 515, "host_large_rows: a window beyond the tap table counts");
}

static void check_bands()
{
   const int Bs[5] = {1, 2, 16, 64, 256};
   for (int rows = 1; rows <= 4400; rows += (rows < 300 ? 1 : 41))
      for (int cols = 1; cols <= 7700; cols += (cols < 300 ? 7 : 247))
         for (int B : Bs) {
            const MarchBands m = march_bands(rows, cols, B);
            CHECK(m.bands >= 1 && m.bands <= std::max(1, rows / 8) && (long long)m.band * m.bands >= rows, "march %dx%d B %d: %d bands of %d", cols, rows, B, m.bands, m.band);
            CHECK(m.strip_blocks == (cols + 4 * BM_STRIP - 1) / (4 * BM_STRIP), "march %d columns: %d blocks across", cols, m.strip_blocks);
         }
   // the 4096-wavefront rule: 128 rows per band where that leaves 4096 wavefronts (one per 248-column strip, band and image), else 64, else 32
   CHECK(extrema_band(15, 20, 1) == 32, "extrema 20x15");                 // 1 wavefront whatever the band
   CHECK(extrema_band(2160, 3840, 1) == 32, "extrema UHD B = 1");         // 16 strips x 17 / 34 bands = 272 / 544
   CHECK(extrema_band(2160, 3840, 256) == 128, "extrema UHD B = 256");    // 16 x 17 x 256 = 69632
   CHECK(extrema_band(2160, 3840, 8) == 64, "extrema UHD B = 8");         // 16 x 17 x 8 = 2176, 16 x 34 x 8 = 4352
}

// octave_steps against the two blur loops run_detection had before the table, restated literally: which steps they launched, from which
// level, with which outputs, and the bytes they told the stage timer (N pixels: B * rows * cols of a batch of 256 UHD images and of one small one)
struct Launched {
   int i, in;
   bool wl, wr, wh, wr0;
   double bytes;
};
static void check_octave_steps()
{
   const OctaveWant wants[3] = {OctaveWant::Detect, OctaveWant::DetectKeepL4, OctaveWant::BlursOnly};
   const double Ns[2] = {256.0 * 2160 * 3840, 1.0 * 131 * 77};
   for (int w = 0; w < 3; w++)
      for (int hn = 0; hn < 2; hn++)
         for (int pm = 0; pm < 2; pm++)
            for (double N : Ns) {
               const bool detect = wants[w] != OctaveWant::BlursOnly, keep_l4 = wants[w] == OctaveWant::DetectKeepL4;
               const bool has_next = hn != 0, fuse_r0 = pm != 0;
               std::vector<Launched> old;
               const bool old_hess_first = !fuse_r0 && detect;
               for (int i = 1; i <= 4 && !detect; i++) {
                  if (i == 4 || (i == 3 && !has_next)) break;
                  const double bytes = (i == 3 ? 5.0 : 8.0) * N;
                  if (i < 3) old.push_back({i, i - 1, true, false, false, false, bytes});
                  else old.push_back({i, 2, false, false, true, false, bytes});
               }
               for (int i = 1; i <= 4 && detect; i++) {
                  double bytes = 12.0 * N;
                  if (i == 1 && fuse_r0) bytes += 8.0 * N;
                  if (i == 3 && has_next) bytes += 2.0 * N;
                  if (i == 1 && fuse_r0) old.push_back({1, 0, true, true, false, true, bytes});
                  else if (i < 3) old.push_back({i, i - 1, true, true, false, false, bytes});
                  else if (i == 3) {
                     if (has_next) old.push_back({3, 2, true, true, true, false, bytes});
                     else old.push_back({3, 2, true, true, false, false, bytes});
                  } else {
                     if (keep_l4) old.push_back({4, 3, true, true, false, false, bytes});
                     else old.push_back({4, 3, false, true, false, false, bytes});
                  }
               }
               const OctaveSteps s = octave_steps(wants[w], has_next, fuse_r0);
               CHECK(s.hess_first == old_hess_first, "want %d next %d march %d: hess_first %d", w, hn, pm, (int)s.hess_first);
               CHECK(!s.step[0].launch, "want %d: step 0 is launched", w);
               size_t k = 0;
               for (int i = 1; i <= 4; i++) {
                  const BlurStep &b = s.step[i];
                  if (!b.launch) continue;
                  CHECK(k < old.size() && old[k].i == i, "want %d next %d march %d: step %d is launched, the loops did not", w, hn, pm, i);
                  const Launched &q = old[k++];
                  CHECK(b.in == q.in && b.write_L == q.wl && b.write_R == q.wr && b.write_half == q.wh && b.write_R0 == q.wr0,
                        "want %d next %d march %d step %d: L%d -> (%d, %d, %d, %d)", w, hn, pm, i, b.in, (int)b.write_L, (int)b.write_R, (int)b.write_half, (int)b.write_R0);
                  CHECK(b.bytes_per_px * N == q.bytes, "want %d next %d march %d step %d: %g bytes, the loops %g", w, hn, pm, i, b.bytes_per_px * N, q.bytes);
               }
               CHECK(k == old.size(), "want %d next %d march %d: %zu launches, the loops %zu", w, hn, pm, k, old.size());
            }
}

int main()
{
   check_octaves();
   check_octave_steps();
   check_capacity();
   check_layouts();
   check_groups();
   check_large();
   check_bands();
   printf("plan_check ok\n");
   return 0;
}
