// CPU check of context setup's host arithmetic (hesaff_amd/csrc/context_tables.h, and OrderMapEpochs of batch_plan.h; built and run by
// tests/test_context_tables.py with g++ -fsanitize=address,undefined).  Every table entry is an index, an offset or a weight that a
// kernel follows without a bounds check: the bounds are taken from the kernels (kernels_sift.h, kernels_pyramid.h) and stated at each
// check.  The tables' bytes are pinned by FNV-1a hashes that were made from the text of build_tables / ensure_patch_taps as pipeline.hip
// had it before the arithmetic moved here (each upload replaced by the hash), not from this code.
// Prints "tables_check ok"; the first failed check prints a message and ends the program with exit code 1.
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <random>
#include <set>
#include "../../hesaff_amd/csrc/batch_plan.h"
#include "../../hesaff_amd/csrc/context_tables.h"

using namespace hesaff_plan;

#define CHECK(cond, ...)                                                     \
   do {                                                                      \
      if (!(cond)) {                                                         \
         fprintf(stderr, "tables_check: %s:%d: %s failed: ", __FILE__, __LINE__, #cond); \
         fprintf(stderr, __VA_ARGS__);                                       \
         fprintf(stderr, "\n");                                              \
         exit(1);                                                            \
      }                                                                      \
   } while (0)

// hesaff_default_params (include/hesaff_amd.h documents the values)
static hesaff_params params(float initialSigma = 1.6f, int upscale = 0)
{
   hesaff_params p;
   memset(&p, 0, sizeof p);
   p.threshold = 16.0f / 3.0f;
   p.edgeEigenValueRatio = 10.0f;
   p.initialSigma = initialSigma;
   p.maxIterations = 16;
   p.convergenceThreshold = 0.05f;
   p.mrSize = 3.0f * sqrtf(3.0f);
   p.maxBinValue = 0.2f;
   p.upscaleInputImage = upscale;
   p.max_batch = 64;
   p.max_kpts_per_mpx = 40000;
   p.fast = 0;
   return p;
}

static void check_default()
{
   const ContextTables t = build_context_tables(params());
   const int K[5] = {11, 9, 11, 13, 15};
   for (int i = 0; i < 5; i++) CHECK(t.pyr_K[i] == K[i], "pyr_K[%d] = %d", i, t.pyr_K[i]);
   CHECK(t.pyr_march, "the default blurs take the marching kernel");
   CHECK(t.up == 0 && t.consts.pd0 == 1.0f, "up %d pd0 %g", t.up, (double)t.consts.pd0);
   CHECK(t.n_masked == 1245 && t.mask_idx.size() == 1245, "n_masked %d, %zu indices", t.n_masked, t.mask_idx.size());
   CHECK(t.n_masked <= 256 * 5, "HS_SIFT_MSK_IT: five masked pixels per thread of k_sift_grad's 256");
   for (size_t s = 0; s < t.mask_idx.size(); s++) {
      const int i = t.mask_idx[s];
      CHECK(i >= 0 && i < HS_PATCH_PIX && i / HS_PATCH < 40 && i % HS_PATCH < 40, "masked pixel %zu at %d", s, i);
      CHECK(s == 0 || t.mask_idx[s - 1] < i, "mask_idx is not in raster order at %zu", s);
      CHECK(t.sift_mask[(size_t)i] > 0.0f, "masked pixel %d has no weight", i);
   }
   CHECK(t.smm.size() == HS_SMM_PIX && t.sift_mask.size() == HS_PATCH_PIX, "mask sizes");
   CHECK(t.bin0.size() == HS_PATCH && t.bin1.size() == HS_PATCH && t.w0.size() == HS_PATCH && t.w1.size() == HS_PATCH, "bin table sizes");
   for (int i = 0; i < HS_PATCH; i++)   // k_sift_hist adds bin0 / bin1 (x 8 orientation bins) into 4 x 4 x 8 cells
      CHECK(t.bin0[i] >= 0 && t.bin0[i] <= 24 && t.bin0[i] % 8 == 0 && t.bin1[i] >= 0 && t.bin1[i] <= 24 && t.bin1[i] % 8 == 0, "bins of %d: %d %d", i, t.bin0[i], t.bin1[i]);

   // ---- k_sift_grad's per-slot constants: 1280 slots of {4 neighbour byte offsets into the 1681-float patch in LDS} and {output slot of the 40 x 40 tile, mask bits}
   CHECK(t.sgrad_nb.size() == 4 * 1280 && t.sgrad_om.size() == 2 * 1280, "sgrad sizes %zu %zu", t.sgrad_nb.size(), t.sgrad_om.size());
   std::set<int> slots;
   for (size_t s = 0; s < 1280; s++) {
      const int32_t *nb = &t.sgrad_nb[4 * s];
      const int om = t.sgrad_om[2 * s];
      for (int q = 0; q < 4; q++) CHECK(nb[q] >= 0 && nb[q] < 4 * HS_PATCH_PIX && nb[q] % 4 == 0, "slot %zu neighbour %d: %d", s, q, nb[q]);
      CHECK(om >= -1 && om < HS_VO_DIM * HS_VO_DIM, "slot %zu output %d", s, om);
      if (s >= (size_t)t.n_masked) CHECK(nb[0] == 0 && nb[1] == 0 && nb[2] == 0 && nb[3] == 0 && om == -1, "unused slot %zu: %d %d %d %d -> %d", s, nb[0], nb[1], nb[2], nb[3], om);
      if (om >= 0) {
         CHECK(slots.insert(om).second, "output slot %d twice", om);
         const int i = t.mask_idx[s], r = i / HS_PATCH, c = i % HS_PATCH;
         CHECK(om == r * HS_VO_DIM + c, "slot %zu: pixel (%d, %d) -> %d", s, r, c, om);
         float w;
         memcpy(&w, &t.sgrad_om[2 * s + 1], 4);
         CHECK(w == t.sift_mask[(size_t)i], "slot %zu: weight %g, mask %g", s, (double)w, (double)t.sift_mask[(size_t)i]);
      }
   }

   // ---- the gradient-pair layout: 40 rows of {first item - f_lo, f_lo, f_hi, 0}, rows back to back, HS_VO_ZERO items in all
   CHECK(t.vo_rows.size() == 4 * HS_VO_DIM && t.vo_src.size() == HS_VO_ITEMS, "vo sizes %zu %zu", t.vo_rows.size(), t.vo_src.size());
   int cursor = 0, empty = 0;
   for (int r = 0; r < HS_VO_DIM; r++) {
      const int x = t.vo_rows[4 * r], f_lo = t.vo_rows[4 * r + 1], f_hi = t.vo_rows[4 * r + 2];
      CHECK(t.vo_rows[4 * r + 3] == 0, "row %d: fourth word", r);
      if (f_lo > f_hi) { empty++; continue; }
      CHECK(f_lo >= 0 && f_hi < HS_VO_DIM / 2, "row %d: span %d..%d", r, f_lo, f_hi);
      CHECK(x + f_lo == cursor, "row %d starts at item %d, the row before ended at %d", r, x + f_lo, cursor);
      for (int f = f_lo; f <= f_hi; f++) {
         CHECK(x + f >= 0 && x + f < HS_VO_ZERO, "row %d item %d at %d", r, f, x + f);
         CHECK(t.vo_src[(size_t)(x + f)] == r * (HS_VO_DIM / 2) + f, "item %d is a copy of tile item %d, not of row %d item %d", x + f, t.vo_src[(size_t)(x + f)], r, f);
      }
      cursor = x + f_hi + 1;
   }
   CHECK(cursor == HS_VO_ZERO, "the layout ends at item %d", cursor);
   CHECK(empty == 1, "%d empty rows", empty);
   for (int i = 0; i < HS_VO_ITEMS; i++) {
      CHECK(t.vo_src[(size_t)i] < HS_VO_DIM * (HS_VO_DIM / 2), "vo_src[%d] = %d", i, t.vo_src[(size_t)i]);
      if (i >= HS_VO_ZERO) CHECK(t.vo_src[(size_t)i] == 0, "padding item %d copies tile item %d", i, t.vo_src[(size_t)i]);
   }
   // every pixel with an output slot lies in its row's span
   for (int om : slots) {
      const int r = om / HS_VO_DIM, f = (om % HS_VO_DIM) / 2;
      CHECK(f >= t.vo_rows[4 * r + 1] && f <= t.vo_rows[4 * r + 2], "output slot %d outside the span of row %d", om, r);
   }
}

// each level owns 256 floats of the tap table (the kernels read taps[0 .. K) from pyr_tap_off[i])
static void check_pyramid_taps(const ContextTables &t, const char *what)
{
   CHECK(t.pyr_taps.size() == 5 * 256, "%s: %zu taps", what, t.pyr_taps.size());
   for (int i = 0; i < 5; i++) {
      CHECK(t.pyr_tap_off[i] == 256 * i, "%s: pyr_tap_off[%d] = %d", what, i, t.pyr_tap_off[i]);
      const int K = t.pyr_K[i];
      CHECK(K >= 0 && K <= 255 && (K == 0 ? i == 0 : K % 2 == 1), "%s: K[%d] = %d", what, i, K);
      const float *tp = t.pyr_taps.data() + t.pyr_tap_off[i];
      double sum = 0.0;
      for (int j = 0; j < K; j++) sum += tp[j];
      if (K > 0) CHECK(fabs(sum - 1.0) <= 1e-6, "%s: taps of level %d sum to %.9f", what, i, sum);
      for (int j = K; j < 256; j++) CHECK(tp[j] == 0.0f, "%s: level %d tap %d beyond K = %d is %g", what, i, j, K, (double)tp[j]);
   }
}

static void check_parameter_sets()
{
   check_pyramid_taps(build_context_tables(params()), "default");
   struct Case { float sigma; int up; int K[5]; };
   const Case cases[5] = {{1.0f, 0, {7, 5, 7, 9, 11}}, {2.0f, 0, {13, 11, 13, 15, 19}}, {0.45f, 0, {0, 3, 3, 5, 5}}, {3.1f, 0, {19, 15, 19, 23, 29}},
                          {1.6f, 1, {9, 9, 11, 13, 15}}};
   for (const Case &cs : cases) {
      char what[64];
      snprintf(what, sizeof what, "initialSigma %g upscale %d", (double)cs.sigma, cs.up);
      const ContextTables t = build_context_tables(params(cs.sigma, cs.up));
      for (int i = 0; i < 5; i++) CHECK(t.pyr_K[i] == cs.K[i], "%s: K[%d] = %d", what, i, t.pyr_K[i]);
      CHECK(t.pyr_march == (cs.K[1] == 9 && cs.K[2] == 11 && cs.K[3] == 13 && cs.K[4] == 15), "%s: pyr_march", what);
      check_pyramid_taps(t, what);
   }
   {
      const ContextTables t = build_context_tables(params(0.9f, 1));   // below the up-sampled input's own blur of 1.0
      CHECK(t.pyr_K[0] == 0 && t.up == 1 && t.consts.pd0 == 0.5f, "0.9 upscaled: K0 %d up %d pd0 %g", t.pyr_K[0], t.up, (double)t.consts.pd0);
      check_pyramid_taps(t, "initialSigma 0.9 upscale 1");
   }
   int code = 0;
   try { (void)build_context_tables(params(100.0f, 0)); }
   catch (const HsError &e) { code = e.code; }
   CHECK(code == HESAFF_ERR_ARG, "initialSigma 100: code %d", code);
}

// the kernels read taps[off[h] .. off[h] + k[h]) for h = (P0 - 1) / 2, P0 odd and <= max_p0 (KpTables::patch_tap_off / _k)
static void check_patch_taps_of(int request, size_t n_taps, int largest_k)
{
   const PatchTaps t = build_patch_taps(request);
   CHECK(t.max_p0 == (request | 1), "request %d: max_p0 %d", request, t.max_p0);
   CHECK(t.off.size() == (size_t)(t.max_p0 + 1) / 2 && t.k.size() == t.off.size(), "request %d: %zu offsets, %zu sizes", request, t.off.size(), t.k.size());
   CHECK(t.taps.size() == n_taps, "request %d: %zu taps", request, t.taps.size());
   int kmax = 0;
   size_t next = 0;
   for (int P0 = 1; P0 <= t.max_p0; P0 += 2) {
      const size_t h = (size_t)(P0 - 1) / 2;
      const int K = t.k[h];
      CHECK(K == hesaff::gauss_ksize(1.5f * ((float)P0 / (float)HS_PATCH)) && K >= 1 && K % 2 == 1, "P0 %d: K %d", P0, K);
      CHECK(t.off[h] >= 0 && (size_t)t.off[h] == next && (size_t)t.off[h] + (size_t)K <= t.taps.size(), "P0 %d: taps at %d + %d of %zu", P0, t.off[h], K, t.taps.size());
      next += (size_t)K;
      double sum = 0.0;
      for (int j = 0; j < K; j++) sum += t.taps[(size_t)t.off[h] + j];
      CHECK(fabs(sum - 1.0) <= 1e-6, "P0 %d: taps sum to %.9f", P0, sum);
      kmax = std::max(kmax, K);
   }
   CHECK(next == t.taps.size(), "request %d: %zu taps, the sizes add up to %zu", request, t.taps.size(), next);
   CHECK(kmax == largest_k, "request %d: largest K %d", request, kmax);
}

static void check_patch_taps()
{
   check_patch_taps_of(3, 2, 1);
   check_patch_taps_of(163, 1560, 37);
   check_patch_taps_of(1443, 115168, 317);
   check_patch_taps_of(162, 1560, 37);    // an even request is rounded up
   check_patch_taps_of(1442, 115168, 317);
   check_patch_taps_of(1, 1, 1);
}

// ---- OrderMapEpochs against the statements run_detection and plan_buffers had before the struct (the fills and the epochs of a pass) ----
struct Before {
   bool map_clean = false;
   int map_kbits = 32;
   uint32_t map_epoch = 0;
   void plan(int kb) { if (kb != map_kbits) { map_kbits = kb; map_clean = false; } }
   bool prelude()
   {
      if (!map_clean) { map_epoch = map_kbits < 32 ? (0xffffffffu >> map_kbits) : 0u; map_clean = true; return true; }
      return false;
   }
   bool pass(uint32_t *bits)
   {
      bool fill = false;
      if (map_epoch == 0) { fill = true; map_epoch = map_kbits < 32 ? (0xffffffffu >> map_kbits) : 0u; }
      if (map_epoch > 0) map_epoch--;
      *bits = map_kbits < 32 ? (map_epoch << map_kbits) : 0u;
      return fill;
   }
};

static void check_epochs()
{
   const int widths[4] = {8, 20, 31, 32};
   for (int kb : widths) {
      OrderMapEpochs e;
      Before b;
      CHECK(e.kbits == 32 && e.epoch == 0 && !e.clean, "a new context's map is not clean");
      e.set_key_bits(kb); b.plan(kb);
      CHECK(e.begin_batch(), "kbits %d: a new map is filled before its first batch", kb);
      CHECK(b.prelude(), "kbits %d", kb);
      CHECK(!e.begin_batch(), "kbits %d: a clean map is not filled again", kb);
      e.set_key_bits(kb);
      CHECK(!e.begin_batch(), "kbits %d: the same key width does not invalidate", kb);
      const uint32_t all_ones = kb < 32 ? (0xffffffffu >> kb) : 0u;   // the fill value's epoch; a fill serves this many passes (one at least)
      // two full wrap-arounds; at 8 bits (16.7 M passes per fill) a few thousand passes around one forced wrap
      unsigned long long passes = 2ull * all_ones + 5;
      if (kb == 8) { e.epoch = b.map_epoch = 1500; passes = 4000; }
      unsigned long long since_fill = kb == 8 ? all_ones - 1500 : 0, refills = 0;
      uint32_t last = 0;
      bool have_last = false;
      for (unsigned long long n = 0; n < passes; n++) {
         if (n % 7 == 3) CHECK(!e.begin_batch() && !b.prelude(), "kbits %d pass %llu: a batch begins on a clean map", kb, n);
         uint32_t want = 0;
         const bool want_fill = b.pass(&want);
         const OrderMapEpochs::Pass p = e.next_pass();
         CHECK(p.refill_first == want_fill && p.epoch_bits == want, "kbits %d pass %llu: fill %d epoch %08x, before the struct %d %08x", kb, n, (int)p.refill_first, p.epoch_bits, (int)want_fill, want);
         // exhausted: the fill before served all_ones passes (epochs all_ones - 1 .. 0), or - 32 bits, no epoch field - its one pass at most
         CHECK(p.refill_first == (since_fill >= all_ones), "kbits %d pass %llu: refill %d after %llu passes on one fill", kb, n, (int)p.refill_first, since_fill);
         if (p.refill_first) { since_fill = 0; have_last = false; refills++; }
         since_fill++;
         if (kb < 32) {
            CHECK((p.epoch_bits >> kb) != all_ones, "kbits %d pass %llu: the fill value's epoch was handed out", kb, n);
            CHECK((p.epoch_bits & ((1u << kb) - 1u)) == 0, "kbits %d pass %llu: epoch %08x reaches into the key", kb, n, p.epoch_bits);
         } else {
            CHECK(p.refill_first && p.epoch_bits == 0, "32 bits pass %llu: every pass refills, epoch 0", n);
         }
         CHECK(!have_last || p.epoch_bits < last, "kbits %d pass %llu: epoch %08x after %08x", kb, n, p.epoch_bits, last);
         last = p.epoch_bits; have_last = true;
      }
      CHECK(refills >= (kb == 8 ? 1u : 2u), "kbits %d: %llu refills", kb, refills);
      // invalidate(): the next batch fills, and its passes start over
      e.invalidate(); b.map_clean = false;
      CHECK(e.begin_batch() && b.prelude(), "kbits %d: an invalidated map is filled", kb);
      uint32_t want = 0;
      const bool want_fill = b.pass(&want);
      const OrderMapEpochs::Pass p = e.next_pass();
      CHECK(p.refill_first == want_fill && p.epoch_bits == want && p.refill_first == (all_ones == 0), "kbits %d: first pass after invalidate()", kb);
      if (kb < 32) CHECK(p.epoch_bits == ((all_ones - 1) << kb), "kbits %d: first epoch %08x", kb, p.epoch_bits);
   }
   // random sequences of plans (key widths), failed plans, batches and passes: fill for fill and epoch for epoch what the statements did
   std::mt19937 rng(20261017);
   OrderMapEpochs e;
   Before b;
   const int kbs[6] = {8, 20, 30, 31, 32, 20};
   for (int step = 0; step < 200000; step++) {
      const unsigned r = rng() % 100;
      if (r < 3) { const int kb = kbs[rng() % 6]; e.set_key_bits(kb); b.plan(kb); }
      else if (r < 5) { e.invalidate(); b.map_clean = false; }
      else if (r < 20) CHECK(e.begin_batch() == b.prelude(), "step %d: begin_batch", step);
      else if (e.clean) {   // (passes follow a batch's prelude)
         uint32_t want = 0;
         const bool want_fill = b.pass(&want);
         const OrderMapEpochs::Pass p = e.next_pass();
         CHECK(p.refill_first == want_fill && p.epoch_bits == want, "step %d: pass", step);
      }
      CHECK(e.clean == b.map_clean && e.kbits == b.map_kbits && e.epoch == b.map_epoch, "step %d: state", step);
   }
}

// ---- bit identity with the tables as pipeline.hip built them before this header (see the head of this file) ----
static uint64_t fnv(const void *p, size_t n)
{
   uint64_t h = 0xcbf29ce484222325ull;
   const unsigned char *b = (const unsigned char *)p;
   for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 0x100000001b3ull; }
   return h;
}
template <class T> static uint64_t fnv(const std::vector<T> &v) { return fnv(v.data(), v.size() * sizeof(T)); }

static void check_hashes()
{
   // the same for every parameter set: the masks, the bins, k_sift_grad's constants, the gradient-pair layout
   const char *names[11] = {"mask_idx", "sgrad_nb", "sgrad_om", "vo_rows", "vo_src", "smm", "sift_mask", "bin0", "bin1", "w0", "w1"};
   const uint64_t fixed[11] = {0x13fe5e5505e29fabull, 0x2039afc1a44d05e3ull, 0x5d58215c6feae5fcull, 0x702aed903599cf49ull, 0x3fd5e4ad257a8954ull, 0x4fa73068d840e7a8ull,
                               0xafc025eaea1ff798ull, 0x6d58f794a705230dull, 0x5f9d288f9156e18dull, 0xa23017308964c275ull, 0xa6550522f15f4075ull};
   // per parameter set: pyr_taps, sched, consts, pyr_K, pyr_tap_off
   struct Set { float sigma; int up; uint64_t h[5]; };
   const Set sets[4] = {
      {1.6f, 0, {0x2cd4e6941b9eab23ull, 0xb52e6ed49d7ac61bull, 0x70ad758bc474cb33ull, 0x4e6bbea2c8241e2eull, 0x987f837ea51b86c9ull}},
      {1.0f, 0, {0x58a9b80469a6cd27ull, 0x78d061753a4b3337ull, 0x70ad758bc474cb33ull, 0xd513e5f3a75bfe62ull, 0x987f837ea51b86c9ull}},
      {0.45f, 0, {0x3c9bd08630a9ae20ull, 0x04b19d059ef443abull, 0x70ad758bc474cb33ull, 0xcd40062165f224f5ull, 0x987f837ea51b86c9ull}},
      {1.6f, 1, {0x362231d9564d56bdull, 0xcfd41e424579716aull, 0x7260758bc5e65fb3ull, 0xdf35a53e8a171d0cull, 0x987f837ea51b86c9ull}}};
   static_assert(sizeof(hesaff::OctaveSchedule) == 16 * 4 && sizeof(DConsts) == 10 * 4, "no padding in what is hashed");
   for (const Set &s : sets) {
      const ContextTables t = build_context_tables(params(s.sigma, s.up));
      const uint64_t got[11] = {fnv(t.mask_idx), fnv(t.sgrad_nb), fnv(t.sgrad_om), fnv(t.vo_rows), fnv(t.vo_src), fnv(t.smm), fnv(t.sift_mask), fnv(t.bin0), fnv(t.bin1),
                                fnv(t.w0), fnv(t.w1)};
      for (int i = 0; i < 11; i++)
         CHECK(got[i] == fixed[i], "initialSigma %g upscale %d: %s hashes to %016llx", (double)s.sigma, s.up, names[i], (unsigned long long)got[i]);
      const uint64_t var[5] = {fnv(t.pyr_taps), fnv(&t.sched, sizeof t.sched), fnv(&t.consts, sizeof t.consts), fnv(t.pyr_K, sizeof t.pyr_K), fnv(t.pyr_tap_off, sizeof t.pyr_tap_off)};
      const char *vn[5] = {"pyr_taps", "sched", "consts", "pyr_K", "pyr_tap_off"};
      for (int i = 0; i < 5; i++)
         CHECK(var[i] == s.h[i], "initialSigma %g upscale %d: %s hashes to %016llx", (double)s.sigma, s.up, vn[i], (unsigned long long)var[i]);
   }
   const PatchTaps pt = build_patch_taps(163);
   CHECK(fnv(pt.taps) == 0x43752deab9dffd2eull && fnv(pt.off) == 0x341b4f1fd4a5d52aull && fnv(pt.k) == 0xb340751cbd14b80bull, "patch taps up to 163: %016llx %016llx %016llx",
         (unsigned long long)fnv(pt.taps), (unsigned long long)fnv(pt.off), (unsigned long long)fnv(pt.k));
   // hesaff_stage_hessian_response's blur: the first octave blur of the default schedule, once the literal 1.2262737f
   const float s1 = hesaff::make_schedule(1.6f, false).blur_sigma[1];
   uint32_t bits;
   memcpy(&bits, &s1, 4);
   CHECK(bits == 0x3f9cf689u && s1 == 1.2262737f, "blur_sigma[1] is %08x", bits);
}

int main()
{
   check_default();
   check_parameter_sets();
   check_patch_taps();
   check_epochs();
   check_hashes();
   printf("tables_check ok\n");
   return 0;
}
