// cells_plan.h -- the host arithmetic of vocabulary cells (hesaff_set_vocabulary_cells, include/hesaff_amd.h): when a `first` array is
// a cell layer over K rows, how many work items n keys in C cells make at most, which cell a work item belongs to, which rows of an
// edge tile lie outside a cell, how a long source is cut into slices, and where the working arrays lie in the context's cells buffer;
// and the same numbers with probes (hesaff_set_vocabulary_probes): entries instead of keys.
// Pure functions and plain structs, no HIP: capi_cells.h and kernels_cells.h obtain their numbers here, and
// tests/native/cells_plan_check.cpp and probes_plan_check.cpp check them on the CPU (tests/test_vocabulary_cells_host.py,
// tests/test_vocabulary_probes_host.py).
#pragma once
#include <cstddef>
#include <cstdint>

#include "train_plan.h"   // StagePlan, Span, accumulate_slots, HS_TRAIN_TILE, HS_VOCAB_MAX_ROWS, HS_TRAIN_MAX_KEYS

namespace hesaff_plan {

constexpr int HS_CELLS_ITEM_KEYS = 64;                            // keys of a work item: one wavefront of k_assign_words_cells
constexpr int64_t HS_CELLS_SLICE_KEYS = HS_TRAIN_MAX_KEYS;        // keys of a slice at most: what the scratch is ever sized for

// first[0 .. c]: first[0] = 0, first[c] = k, strictly increasing - cell j owns rows first[j] .. first[j + 1] - 1 and none is empty
inline bool cells_first_ok(const uint32_t *first, int64_t c, int64_t k)
{
   if (!first || c < 1 || k < 1 || c > k || k > HS_VOCAB_MAX_ROWS) return false;
   if (first[0] != 0 || (int64_t)first[c] != k) return false;
   for (int64_t j = 0; j < c; j++)
      if (first[j] >= first[j + 1]) return false;
   return true;
}

// work items of a cell with m keys, and the most that n keys in c cells can make: sum ceil(m_j / 64) <= floor(n / 64) + c, because
// ceil(m / 64) <= m / 64 + 63 / 64 over c cells adds up to less than n / 64 + c.  Known to the host without a synchronisation.
HS_TRAIN_HD uint32_t cells_items_of(uint32_t m) { return (m + (uint32_t)HS_CELLS_ITEM_KEYS - 1u) / (uint32_t)HS_CELLS_ITEM_KEYS; }
inline int64_t cells_item_bound(int64_t n, int64_t c) { return n / HS_CELLS_ITEM_KEYS + c; }

// item_first[0 .. c]: the exclusive scan of the cells' item counts, item_first[c] the total.  The cell of work item `item`
// (item < item_first[c]): the LAST j with item_first[j] <= item - behind a run of cells without keys, whose entries are equal, that is
// the one cell of the run that has items.
HS_TRAIN_HD int cells_item_cell(const uint32_t *item_first, int c, uint32_t item)
{
   int lo = 0, hi = c;   // item_first[lo] <= item < item_first[hi]
   while (hi - lo > 1) {
      const int mid = lo + (hi - lo) / 2;
      if (item_first[mid] <= item) lo = mid;
      else hi = mid;
   }
   return lo;
}

// the tiles a cell [lo, hi) streams, and whether a row of one of them lies outside the cell (its score is forced to 0x7fffffff)
HS_TRAIN_HD int cells_first_tile(uint32_t lo) { return (int)(lo / (uint32_t)HS_TRAIN_TILE); }
HS_TRAIN_HD int cells_last_tile(uint32_t hi) { return (int)((hi - 1u) / (uint32_t)HS_TRAIN_TILE); }
HS_TRAIN_HD bool cells_row_masked(uint32_t row, uint32_t lo, uint32_t hi) { return row < lo || row >= hi; }
// a tile needs the mask only where it holds a row outside the cell: the first tile of a cell that does not start on a tile boundary
// and the last of one that does not end on one (a cell inside one tile: both)
HS_TRAIN_HD bool cells_tile_is_edge(int tile, uint32_t lo, uint32_t hi)
{
   const uint32_t t0 = (uint32_t)tile * (uint32_t)HS_TRAIN_TILE;
   return t0 < lo || t0 + (uint32_t)HS_TRAIN_TILE > hi;
}

// a source of n keys in slices of at most `slice` keys: their number, and slice s's first key and length
inline int64_t cells_slice_count(int64_t n, int64_t slice) { return n <= 0 ? 0 : (n + slice - 1) / slice; }
inline int64_t cells_slice_begin(int64_t s, int64_t slice) { return s * slice; }
inline int64_t cells_slice_keys(int64_t s, int64_t n, int64_t slice) { return n - s * slice < slice ? n - s * slice : slice; }

// The layer as the device holds it (the context's cells.layer buffer): the coarse rows packed as k_assign_words reads a vocabulary, and
// first[c + 1].
struct CellLayerArrays {
   Span<uint8_t> tiles;
   Span<int32_t> norms;
   Span<uint32_t> first;
   int n_tiles;
};
inline CellLayerArrays cell_layer_arrays(StagePlan &p, int64_t c)
{
   CellLayerArrays a;
   a.n_tiles = (int)((c + HS_TRAIN_TILE - 1) / HS_TRAIN_TILE);
   a.tiles = p.add<uint8_t>((size_t)a.n_tiles * HS_TRAIN_TILE * 128);
   a.norms = p.add<int32_t>((size_t)a.n_tiles * HS_TRAIN_TILE);
   a.first = p.add<uint32_t>((size_t)c + 1);
   return a;
}

// The working arrays of an assignment through c cells, for `cap` keys of capacity, in the context's cells.scratch buffer (grow only):
// 12 bytes per key and arrays of size c.
struct CellScratch {
   Span<int32_t> coarse;        // [cap][2]: (cell, dist2 to the coarse row) per key
   Span<uint32_t> perm;         // [cap]: the key indices grouped by cell
   Span<uint32_t> sub;          // [c][slots]: the histogram's sub-counters (kernels_train.h)
   Span<uint32_t> cursor;       // [c][slots]: their scan, then each entry's end: cell j's keys are perm[end of j - 1 .. end of j)
   Span<uint32_t> item_first;   // [c + 1]: each cell's first work item, and the total
   Span<uint32_t> block_sums;   // the scans', one per 4096 entries and one more
   Span<uint32_t> total;        // the first scan's total (the keys)
   int slots;                   // accumulate_slots(c)
};
inline CellScratch cell_scratch(StagePlan &p, int64_t cap, int64_t c)
{
   CellScratch s;
   s.slots = accumulate_slots(c);
   const size_t entries = (size_t)c * (size_t)s.slots;
   s.coarse = p.add<int32_t>((size_t)cap * 2);
   s.perm = p.add<uint32_t>((size_t)cap);
   s.sub = p.add<uint32_t>(entries);
   s.cursor = p.add<uint32_t>(entries);
   s.item_first = p.add<uint32_t>((size_t)c + 1);
   s.block_sums = p.add<uint32_t>((entries + 4095) / 4096 + 1);
   s.total = p.add<uint32_t>(1);
   return s;
}

// ---- vocabulary probes (hesaff_set_vocabulary_probes): a key is searched in its P' = min(P, C) nearest cells ----
// The grouping and the search inside the cells then run over ENTRIES, e = key * P' + p for probe rank p, each with the cell of that
// rank: n keys make n * P' entries, at most 2^24 of them in a slice - what the grouping is sized for - so a slice holds
// floor(2^24 / P') keys, and the work items are bounded by the rule above over the entries, floor(n * P' / 64) + c.
constexpr int HS_CELLS_MAX_PROBES = 8;
inline bool cells_probes_ok(int64_t probes) { return probes >= 1 && probes <= HS_CELLS_MAX_PROBES; }
inline int cells_probes_used(int64_t probes, int64_t c) { return (int)(probes < c ? probes : c); }
inline int64_t cells_probe_slice_keys(int64_t used) { return HS_CELLS_SLICE_KEYS / used; }
inline int64_t cells_probe_entries(int64_t n, int64_t used) { return n * used; }
inline int64_t cells_probe_item_bound(int64_t n, int64_t used, int64_t c) { return cells_item_bound(cells_probe_entries(n, used), c); }
HS_TRAIN_HD uint32_t cells_entry_key(uint32_t entry, uint32_t used) { return entry / used; }

// The working arrays with probes, for `cap` keys of capacity: CellScratch over cap * P' entries - coarse holds (cell, dist2 to its
// coarse row) per entry, perm the entries grouped by cell - and, with P' > 1, fine: (row, dist2) per entry, which the merge reduces
// to the key's 8 bytes.  (8 + 4 + 8) P' bytes per key; with P' = 1 nothing is added and the layout is cell_scratch's byte for byte.
struct ProbeScratch {
   CellScratch s;
   Span<int32_t> fine;          // [cap * P'][2]; P' = 1: empty, the fine search writes to the caller's array
   int used;                    // P'
};
inline ProbeScratch probe_scratch(StagePlan &p, int64_t cap, int64_t c, int used)
{
   ProbeScratch q;
   q.used = used;
   q.s = cell_scratch(p, cells_probe_entries(cap, used), c);
   q.fine.off = 0; q.fine.count = 0;
   if (used > 1) q.fine = p.add<int32_t>((size_t)cells_probe_entries(cap, used) * 2);
   return q;
}

// Sorting K rows by cell (hesaff_build_vocabulary_cells): cell[k] in 0 .. c - 1 -> order[new] = old row, stable; the cells that received
// a row, in order, as kept[] (old cell indices) and first[0 .. kept]; returns the number kept.  order: k entries, kept: c, first: c + 1.
inline int cells_group_rows(const int32_t *cell, int64_t k, int64_t c, int32_t *order, int32_t *kept, uint32_t *first)
{
   for (int64_t j = 0; j <= c; j++) first[j] = 0;
   for (int64_t r = 0; r < k; r++) first[cell[r] + 1]++;
   for (int64_t j = 0; j < c; j++) first[j + 1] += first[j];   // first[j]: where old cell j's rows begin
   for (int64_t r = 0; r < k; r++) order[first[cell[r]]++] = (int32_t)r;   // (stable: rows in increasing r; first[j] is now cell j's end)
   int n = 0;
   uint32_t begin = 0;
   for (int64_t j = 0; j < c; j++) {
      const uint32_t end = first[j];
      if (end > begin) { kept[n] = (int32_t)j; first[n] = begin; n++; }
      begin = end;
   }
   first[n] = (uint32_t)k;
   return n;
}

} // namespace hesaff_plan
