// batch_plan.h -- the host arithmetic of a batch plan: everything that decides what the kernels may touch and that needs no device to be
// worked out.  Octave geometry, capacities, the layouts of the counter block and of the starts block, image groups, the launch shape of the
// large-window row kernel, band heights.  Pure functions and plain structs, no HIP: pipeline.hip and capi_impl.h obtain their numbers here,
// and tests/native/plan_check.cpp checks them on the CPU (tests/test_batch_plan.py), launch shapes included, before they meet a GPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "chunk_engine.h"   // HsError
#include "host_tables.h"
#include "plan_consts.h"

namespace hesaff_plan {

using hesaff_engine::HsError;

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// ---- octave geometry (pyramid.cpp:283-291) ----
struct OctGeom {
   int rows, cols, pitch;
   long long word_base;   // first bitmask word of this octave inside one image
   int words_per_row;
};
struct PyramidGeom {
   std::vector<OctGeom> oct;
   long long words_per_image = 0;   // bitmask words (64 pixels each) of one image: HS_NSCALES levels of every octave
};
// the octaves of an H x W image, the first at (H << up) x (W << up)
inline PyramidGeom pyramid_geometry(int H, int W, int up)
{
   PyramidGeom p;
   int r = H << up, cc = W << up;
   const int minSize = 2 * HS_BORDER + 2;   // pyramid.cpp:283
   while (r > minSize && cc > minSize) {
      OctGeom g;
      g.rows = r; g.cols = cc; g.pitch = round_up(cc, 64);
      g.words_per_row = (cc + 63) / 64;
      g.word_base = p.words_per_image;
      p.words_per_image += (long long)HS_NSCALES * r * g.words_per_row;
      p.oct.push_back(g);
      r /= 2; cc /= 2;
      if ((int)p.oct.size() >= HS_MAX_OCTAVES) break;
   }
   return p;
}

// ---- the blur launches of an octave (pyramid.cpp:224-259) ----
// What a caller wants of an octave whose first level L0 exists: the planes detection reads (L0..L3, R0..R4), those and L4 (the stage
// operator that returns every plane), or the blurs alone (describe_regions: L1, L2 and the next octave's first level, no response plane).
enum class OctaveWant { Detect, DetectKeepL4, BlursOnly };
// Step i = 1..4 blurs level `in` into level i: write_L keeps the blurred level, write_R its response plane R[i], write_half its 2x decimation,
// the next octave's first level, write_R0 the response of the input level as well.  bytes_per_px: the algorithmic bytes the stage timer is
// told: 12, + 8 with R0 (read L0 + write R0 of the stand-alone pass), + 2 with the decimation; the blurs alone 8 and 5.
struct BlurStep { bool launch; int in; bool write_L, write_R, write_half, write_R0; double bytes_per_px; };
// hess_first: R0 = hessianResponse(L0) (pyramid.cpp:230) as a pass of its own before step 1.  step[1..4]; step[0] is never launched.
struct OctaveSteps { bool hess_first; BlurStep step[5]; };
// has_next: an octave follows.  pyr_march: the marching kernel serves the octave's tap counts (default sigmas) and fuses R0 into step 1.
inline OctaveSteps octave_steps(OctaveWant want, bool has_next, bool pyr_march)
{
   const bool detect = want != OctaveWant::BlursOnly;
   OctaveSteps s = {detect && !pyr_march, {}};
   for (int i = 1; i <= 4; i++) {
      const bool half = i == 3 && has_next, r0 = i == 1 && pyr_march;
      // L4 is never read by detection (getHessianPointType reads L1..L3); without detection L3 is only the source of the next octave
      if (detect) s.step[i] = {true, i - 1, i < 4 || want == OctaveWant::DetectKeepL4, true, half, r0, 12.0 + (r0 ? 8.0 : 0.0) + (half ? 2.0 : 0.0)};
      else if (i < 3) s.step[i] = {true, i - 1, true, false, false, false, 8.0};
      else if (half) s.step[i] = {true, 2, false, false, true, false, 5.0};
   }
   return s;
}

// ---- capacities of a batch of B images whose first pyramid level is PH x PW ----
// keypoints: max_kpts_per_mpx per megapixel of the first pyramid level, 4096 at least
inline uint32_t keypoint_capacity(int B, int PH, int PW, double max_kpts_per_mpx)
{
   double mpx = (double)B * PH * PW / 1.0e6;
   double capd = mpx * max_kpts_per_mpx;
   if (capd < 4096) capd = 4096;
   if (capd > 2.0e9) throw HsError(HESAFF_ERR_ARG, "batch too large for 32-bit keypoint indices");
   return ((uint32_t)capd + 63u) & ~63u;   // a multiple of 64: the arrays carved out of one buffer (cap entries each) stay 16-byte aligned
}
// candidate slots of one octave: the keypoint capacity + what the wavefronts of k_extrema_march may leave unused of their blocks of 64
// (octave 0 has the most wavefronts: one per 248-column strip and 32-row band at least)
inline uint32_t candidate_capacity(uint32_t cap, int B, int PH, int PW)
{
   const unsigned long long waves0 = (unsigned long long)((PW + EXM_STRIP - 1) / EXM_STRIP) * (unsigned long long)(PH / 32 + 1) * (unsigned long long)B;
   // + cap / 8: a wavefront also abandons the rest of its block whenever a ballot group does not fit (holes grow with the number of
   // blocks, not only with the number of wavefronts).  96 bytes per slot: 11 GB per 256 UHD images at the default max_kpts_per_mpx
   const unsigned long long cc = (unsigned long long)cap + (unsigned long long)cap / 8 + HS_CAND_BLOCK * waves0;
   if (cc > 0xfffffff0ull) throw HsError(HESAFF_ERR_ARG, "batch too large for 32-bit candidate indices");
   return (uint32_t)cc;
}
// bits of an order key: 3 x pixels of the first pyramid level
inline int order_key_bits(int PH, int PW)
{
   int kb = 1;
   while (kb < 32 && (3ull * (unsigned long long)PH * PW) > (1ull << kb)) kb++;
   return kb;
}

// ---- the epochs of the order-key map (b_map; OctaveCtx::map_epoch, kernels_pyramid.h) ----
// The map is filled with "free" (all ones) when it is new; every pass over an octave then bids with keys of a fresh, smaller epoch in the
// bits above the key, so what earlier passes left behind never wins - no fill and no reset per octave.  This is the bookkeeping: when
// the map must be filled, and which epoch a pass bids with.  run_detection issues the fills exactly when told to.
struct OrderMapEpochs {
   int kbits = 32;       // bits of an order key (order_key_bits)
   uint32_t epoch = 0;   // the last epoch handed out; 0: the next pass refills the map first
   bool clean = false;   // the map holds nothing but all-ones words and bids of epochs above `epoch`
   // the all-ones epoch, which the fill value carries and no pass gets (none at all when the key takes the whole word)
   uint32_t fill_epoch() const { return kbits < 32 ? (0xffffffffu >> kbits) : 0u; }
   // the block is new or resized, or a plan failed half-way: nothing is known of its contents
   void invalidate() { clean = false; }
   void set_key_bits(int kb) { if (kb != kbits) { kbits = kb; clean = false; } }   // (another key width: epochs of the old one mean nothing)
   // before the first pass of a batch: true when the map must be filled now
   bool begin_batch()
   {
      if (clean) return false;
      epoch = fill_epoch(); clean = true;
      return true;
   }
   // a fresh epoch for a pass (counting down): refill_first when they have run out - the map is then filled before the pass
   struct Pass { bool refill_first; uint32_t epoch_bits; };
   Pass next_pass()
   {
      const bool refill = epoch == 0;
      if (refill) epoch = fill_epoch();
      if (epoch > 0) epoch--;
      return {refill, kbits < 32 ? (epoch << kbits) : 0u};
   }
};

// ---- the counter block: 64 words of device memory (b_counters) ----
// The kernels take pointers to single words; the host names them here.  CounterHead is what the host reads back at the end of a batch.
struct CounterHead {
   uint32_t cand;           // candidates of the octave being scanned (k_extrema_march -> k_localize)
   uint32_t rec;            // localised records of the batch so far
   uint32_t overflow;       // a candidate or a record did not fit
   uint32_t hess_total;     // Hessian keypoints of the batch
   uint32_t desc_total;     // descriptors of the batch
   uint32_t hess_detected;  // with a keypoint limit: the Hessian keypoints detection found, hess_total being those kept (0 otherwise)
   uint32_t row_overflow;   // the T' rows of the large windows exceeded their buffer (k_patch_large_rows)
   uint32_t pad7;
};
struct CounterBlock {
   CounterHead head;
   uint32_t bin_count[16];       // [HS_NBINS] keypoints per window-size bin ...
   uint32_t bin_work[8];         // [HS_NBINS] ... and the next unclaimed item of each bin's list: cleared together, once per image group
   uint32_t oct_rec_start[32];   // [HS_MAX_OCTAVES] value of `rec` when the octave's scan began
   static constexpr size_t bins_bytes() { return sizeof(uint32_t) * (16 + 8); }   // bin_count and bin_work, from offsetof(bin_count)
};
static_assert(sizeof(CounterHead) == 8 * 4 && sizeof(CounterBlock) == 64 * 4, "counter block: 64 words, the first 8 read back");
static_assert(offsetof(CounterHead, cand) == 0 * 4 && offsetof(CounterHead, rec) == 1 * 4 && offsetof(CounterHead, overflow) == 2 * 4 &&
              offsetof(CounterHead, hess_total) == 3 * 4 && offsetof(CounterHead, desc_total) == 4 * 4 && offsetof(CounterHead, row_overflow) == 6 * 4,
              "counter words stay where the kernels' callers have always put them");
static_assert(offsetof(CounterBlock, head) == 0 && offsetof(CounterBlock, bin_count) == 8 * 4 && offsetof(CounterBlock, bin_work) == 24 * 4 &&
              offsetof(CounterBlock, oct_rec_start) == 32 * 4 && CounterBlock::bins_bytes() == 24 * 4,
              "bin counts at word 8, bin work counters at 24, octave record starts at 32");
static_assert(HS_NBINS <= 8 && HS_MAX_OCTAVES <= 32, "the bins and the octaves fit their words");

// ---- the starts block (b_starts, and its copies in pinned host memory), T = int32_t or uint32_t, const or not ----
//   hess()            B + 1 Hessian starts: image b owns [hess()[b], hess()[b + 1])
//   desc()            B + 1 descriptor starts
//   large_rows()      per image, the T' rows its huge windows (P > HS_BIN3_PMAX) need at most; B words and one that stays 0
//   largest_window()  the largest such P of the batch (0: none).  k_image_large_rows writes it as `rows + nimg + 1`.
template <class T> struct StartsBlock {
   T *base;
   int B;
   T *hess() const { return base; }
   T *desc() const { return base + (B + 1); }
   T *large_rows() const { return base + 2 * (B + 1); }
   T *largest_window() const { return large_rows() + B + 1; }
   size_t words_final() const { return (size_t)2 * (B + 1); }          // hess() and desc(): what the end of a batch copies out
   size_t words_to_clear() const { return (size_t)(B + 2); }           // large_rows() .. largest_window(), before k_image_large_rows
   size_t words_to_copy() const { return (size_t)3 * (B + 1) + 1; }    // all four: what the round trip after detection copies out
   size_t words_allocated() const { return ((size_t)(B + 1) * 3 + 2); }   // (one spare word)
};
template <class T> inline StartsBlock<T> starts_block(T *base, int B) { return StartsBlock<T>{base, B}; }

// hesaff_describe_regions: a chunk's block is B + 1 record starts, then - this many bytes in - its hesaff_region records
inline size_t describe_records_offset(int B) { return (((size_t)B + 1) * 4 + 255) & ~(size_t)255; }

// hesaff_set_next_masks: a chunk's block is B "present" bytes (0: image b has no mask), then - this many bytes in - B tight H x W planes
inline size_t mask_planes_offset(int B) { return ((size_t)B + 255) & ~(size_t)255; }
inline size_t mask_block_bytes(int B, int H, int W) { return mask_planes_offset(B) + (size_t)B * (size_t)H * (size_t)W; }

// ---- image groups ----
// Images are processed in groups [lo, hi) of Hessian keypoints so that the patch buffers stay bounded: about 16 groups per batch keep
// the three-stage pipeline full, between 300 k (launch overheads) and 1.2 M keypoints (buffer size).
// (the group size itself hardly matters: 0.6 / 0.9 / 1.2 / 1.8 / 2.4 M keypoints per group at B = 256, shuffled: 810 / 823 / 816 /
//  818 / 816 ms; what matters is that the buffers of a group stay modest: 33 KB per keypoint of a group)
inline uint32_t group_keypoint_limit(uint32_t n_hess) { return std::min<uint32_t>(std::max<uint32_t>(n_hess / 16u, 300000u), 1200000u); }
struct ImageGroup { uint32_t lo, hi, large_rows; };
struct GroupPlan {
   std::vector<ImageGroup> groups;
   uint32_t max_n = 0;   // keypoints of the largest group
};
// hs: B + 1 Hessian starts; lrows: the images' large-window rows (StartsBlock::large_rows).  Greedy: a group takes images while it stays
// within group_keypoint_limit(hs[B]) keypoints and trows_rows T' rows (the row buffer; a single image may exceed either: the buffers
// grow).  Groups without keypoints are dropped.
inline GroupPlan form_groups(const int32_t *hs, const uint32_t *lrows, int B, uint32_t trows_rows)
{
   GroupPlan p;
   const uint32_t group_kpts = group_keypoint_limit((uint32_t)hs[B]);
   for (int g0 = 0; g0 < B;) {
      int g1 = g0 + 1;
      // (64 bits for the comparison below.  The sum itself fits 32: it starts as one 32-bit word and grows only while it stays <= trows_rows.)
      unsigned long long rows = lrows[g0];
      while (g1 < B && (uint32_t)(hs[g1 + 1] - hs[g0]) <= group_kpts && rows + lrows[g1] <= trows_rows) { rows += lrows[g1]; g1++; }
      if (hs[g1] > hs[g0]) {
         p.groups.push_back({(uint32_t)hs[g0], (uint32_t)hs[g1], (uint32_t)rows});
         p.max_n = std::max(p.max_n, (uint32_t)(hs[g1] - hs[g0]));
      }
      g0 = g1;
   }
   return p;
}

// ---- the large-window row kernel (k_patch_large_rows, P > HS_BIN3_PMAX) ----
#define HS_LARGE_NW 2      // wavefronts per block of k_patch_large_rows' three-row form at most: blocks of 40 KB find room beside the other
                           // stages' kernels where blocks of 80 KB wait (against as many as fit: dense step 786 -> 773 ms, photographs 393 -> 383)
#define HS_LARGE_SPLIT 1280   // windows up to this side in a launch of their own when the batch holds larger ones (k_patch_large_rows: split at
                              // 1024 / 1280 / 1536: 7.23 / 7.15 / 7.94 ms per 32 photograph mosaics, profiles/r06_notes.md)
constexpr size_t HS_LDS_PER_CU = 160 * 1024;

// LDS per wavefront for windows up to pmax: window row + replicated borders + taps
struct LargeGeom { int srow_stride, tap_stride; size_t lds; };   // lds: bytes for a block of FOUR wavefronts
inline LargeGeom large_geom(int pmax)
{
   LargeGeom g;
   // window row + r replicated border samples on each side, r = K/2 <= (6 * 1.5 * P0/41 + 2) / 2
   g.srow_stride = round_up((int)(pmax * 1.23) + 16, 64);
   g.tap_stride = round_up((int)(pmax * 0.22) + 8, 64);   // K = odd(int(6 * 1.5 * P0/41 + 1))
   g.lds = (size_t)4 * (g.srow_stride + g.tap_stride) * 4;
   return g;
}

// The dynamic-LDS opt-in of the kernel for images whose tap table reaches max_p0.  It keeps one window row (+ borders, + taps) per
// wavefront in LDS: blocks of four wavefronts while four rows of the batch's largest window fit the CU's 160 KB, of two or one beyond
// that (large_rows_launch); a row that does not fit alone - a window above ~27 900 pixels a side, i.e. an image of more than 780 Mpx -
// is refused here.
inline size_t large_rows_lds_optin(int max_p0)
{
   const LargeGeom lg = large_geom(max_p0 + 2);
   if (lg.lds / 4 > HS_LDS_PER_CU) throw HsError(HESAFF_ERR_ARG, "image too large for the large-window row kernel (sqrt(width x height) above about 27900)");
   // (three rows per wavefront where they fit: the launches ask for up to the whole LDS of a CU)
   return std::min<size_t>(lg.lds + (size_t)8 * lg.srow_stride * 4, HS_LDS_PER_CU);
}

// One launch, for the windows with sides up to p_hi.  The kernel lays out, per wavefront, nrow rows of srow_stride floats and
// tap_stride floats behind them: lds_bytes == wavefronts * (nrow * srow_stride + tap_stride) * 4.
struct LargeLaunch {
   int srow_stride, tap_stride, nrow;
   uint32_t wavefronts;   // per block: 4, 2 or 1
   size_t lds_bytes;      // dynamic LDS of a block
   uint32_t grid_blocks;
};
inline LargeLaunch large_rows_launch(int p_hi, int max_p0, uint32_t large_rows_bound)
{
   // LDS per wavefront for the largest window of the launch, rounded up so that few distinct launch shapes occur
   const LargeGeom lg = large_geom(std::min(max_p0 + 2, (p_hi + 255) / 256 * 256));
   const size_t wave1 = lg.lds / 4;                                        // one row + taps
   const size_t wave3 = wave1 + (size_t)2 * lg.srow_stride * 4;            // three rows + taps
   // the three-row form only where six wavefronts of it fit a CU (windows up to about 1700): below that occupancy the kernel
   // is all exposed gather latency (measured: 3.5x slower at two wavefronts per CU, profiles/r06_notes.md)
   const int nrow = wave3 * 6 <= HS_LDS_PER_CU ? 3 : 1;
   const size_t per_wave = nrow == 3 ? wave3 : wave1;
   // wavefronts per block: four while their rows fit the CU's LDS (large_rows_lds_optin made sure one row fits); blocks of two where two
   // such blocks pack the CU's LDS more tightly than one block of four
   uint32_t nw = 4;
   while (nw > 1 && per_wave * nw > HS_LDS_PER_CU) nw >>= 1;
   if (nw == 4 && (HS_LDS_PER_CU / (per_wave * 2)) * 2 > (HS_LDS_PER_CU / (per_wave * 4)) * 4) nw = 2;
   if (nrow == 3) nw = std::min<uint32_t>(nw, HS_LARGE_NW);
   const uint32_t gblocks = std::min<uint32_t>((large_rows_bound + nw * HS_LARGE_CHUNK - 1) / (nw * HS_LARGE_CHUNK), 256 * 16 * (4 / nw));
   return {lg.srow_stride, lg.tap_stride, nrow, nw, per_wave * nw, gblocks};
}

// The launches of a group: sized for the largest window that exists in the batch (batch_max_p; 0: unknown), not for the largest the image
// could hold.  A batch whose largest window is above HS_LARGE_SPLIT runs as two launches - windows up to HS_LARGE_SPLIT with the LDS, i.e.
// the occupancy, of such a window, the rest with that of the batch's largest.  Launch i serves the sides in (p_lo[i], p_hi[i]].
struct LargeSplit { int n; int p_lo[2], p_hi[2]; };
inline LargeSplit large_rows_split(int max_p0, int batch_max_p)
{
   const int pmax = std::min(max_p0 + 2, std::max(HS_BIN3_PMAX + 1, (batch_max_p > 0 ? batch_max_p : max_p0 + 2)));
   if (pmax > HS_LARGE_SPLIT) return {2, {0, HS_LARGE_SPLIT}, {HS_LARGE_SPLIT, pmax}};
   return {1, {0, 0}, {pmax, 0}};
}

// What k_image_large_rows works out on the device, for keypoints the host holds (hesaff_stage_normalize_affine): the T' rows of the
// windows of the last bin, bounded by the sum of their sides, and the largest such side.  Mirrors hs_window_p0 and hs_patch_bin
// (kernels_keypoint.h): P = 2 * int(ceil(s * mrSize)) + 3, counted when it is above HS_BIN3_PMAX and its taps are tabulated.
struct LargeRows { uint32_t rows; int max_p; };
inline LargeRows host_large_rows(const float *s, int n, float mrSize, int max_p0)
{
   unsigned long long large_rows = 0;
   int max_p = 0;
   for (int i = 0; i < n; i++) {
      const float mrScale = ceilf(s[i] * mrSize);
      const long long P = (mrScale < 1.0e6f) ? 2 * (long long)mrScale + 3 : 0;
      if (P > HS_BIN3_PMAX && P <= max_p0 + 2) { large_rows += (unsigned long long)P; max_p = std::max(max_p, (int)P); }
   }
   if (large_rows > 0xffffffffull) throw HsError(HESAFF_ERR_NOMEM, "too many huge windows in one call");
   return {(uint32_t)large_rows, max_p};
}

// ---- band heights ----
// k_blur_hess_march over B planes of rows x cols: 16 bands per octave is the measured optimum for 16 x 4K at every octave
// (sweeps in profiles/r01_notes.md); small batches get proportionally more bands to keep ~1000 blocks in flight.
struct MarchBands {
   int strip_blocks;   // blocks of four strips across a row: the grid's x
   int bands, band;    // bands asked for, and the rows of one
};
inline MarchBands march_bands(int rows, int cols, int B)
{
   const int strips = (cols + BM_STRIP - 1) / BM_STRIP;
   const long long blocks_per_band = (long long)((strips + 3) / 4) * B;
   int best_nb = 16 * (int)std::max<long long>(1, std::min<long long>(4, 64 / std::max<long long>(1, blocks_per_band)));
   best_nb = std::max(1, std::min(best_nb, std::max(1, rows / 8)));
   return {(strips + 3) / 4, best_nb, (rows + best_nb - 1) / best_nb};
}
// k_extrema_march: bands of 128 rows (a band re-reads 4 rows of halo and starts with two row loads nothing overlaps: 32 / 64 / 128 / 256
// rows measured 25.0 / 23.4 / 22.2 / 23.5 ms for the detection stage of 256 UHD images); shorter bands when that would leave the chip
// short of wavefronts
inline int extrema_band(int rows, int cols, int B)
{
   const int strips = (cols + EXM_STRIP - 1) / EXM_STRIP;
   auto waves_at = [&](int rows_per_band) { return (long long)strips * ((rows + rows_per_band - 1) / rows_per_band) * B; };
   return waves_at(128) >= 4096 ? 128 : (waves_at(64) >= 4096 ? 64 : 32);
}

} // namespace hesaff_plan
