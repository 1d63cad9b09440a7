// cells_plan_check.cpp -- the host arithmetic of vocabulary cells (hesaff_amd/csrc/cells_plan.h) on the CPU: which `first` arrays are a
// layer, the work-item bound against the items of every distribution tried, the wave -> cell search against a linear walk, the edge-tile
// mask against the rows of a cell, the slices of a long source, the stable grouping of rows, and the layout of the working arrays.
// tests/test_vocabulary_cells_host.py builds it with AddressSanitizer + UBSan and runs it.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../hesaff_amd/csrc/cells_plan.h"

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

static uint32_t g_seed = 12345u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

static void check_first()
{
   const uint32_t one[] = {0, 1}, flat[] = {0, 257}, three[] = {0, 5, 9, 33}, each[] = {0, 1, 2, 3};
   CHECK(cells_first_ok(one, 1, 1) && cells_first_ok(flat, 1, 257) && cells_first_ok(three, 3, 33) && cells_first_ok(each, 3, 3), "layers");
   const uint32_t not0[] = {1, 5, 33}, notk[] = {0, 5, 32}, flatrun[] = {0, 5, 5, 33}, down[] = {0, 9, 5, 33}, beyond[] = {0, 40, 33};
   CHECK(!cells_first_ok(not0, 2, 33), "first[0] != 0");
   CHECK(!cells_first_ok(notk, 2, 33), "first[c] != k");
   CHECK(!cells_first_ok(flatrun, 3, 33), "an empty cell");
   CHECK(!cells_first_ok(down, 3, 33) && !cells_first_ok(beyond, 2, 33), "not increasing");
   CHECK(!cells_first_ok(nullptr, 1, 1) && !cells_first_ok(one, 0, 1) && !cells_first_ok(one, -1, 1) && !cells_first_ok(three, 3, 0), "no array, no cell, no row");
   CHECK(!cells_first_ok(each, 4, 3), "more cells than rows (never reads first[4])");
   std::vector<uint32_t> big(((size_t)1 << 20) + 1);
   for (size_t i = 0; i < big.size(); i++) big[i] = (uint32_t)i;
   CHECK(cells_first_ok(big.data(), (int64_t)1 << 20, (int64_t)1 << 20), "2^20 cells of one row");
   big.back() = (1u << 20) + 1;
   CHECK(!cells_first_ok(big.data(), (int64_t)1 << 20, ((int64_t)1 << 20) + 1), "k beyond 2^20");
}

// item offsets of the key counts m[], as the device's scan makes them
static std::vector<uint32_t> item_offsets(const std::vector<uint32_t> &m)
{
   std::vector<uint32_t> f(m.size() + 1, 0);
   for (size_t j = 0; j < m.size(); j++) f[j + 1] = f[j] + cells_items_of(m[j]);
   return f;
}

static void check_items()
{
   CHECK(cells_items_of(0) == 0 && cells_items_of(1) == 1 && cells_items_of(64) == 1 && cells_items_of(65) == 2 && cells_items_of(257) == 5, "ceil(m / 64)");
   CHECK(cells_items_of(1u << 24) == (1u << 18), "a whole slice in one cell");
   CHECK(cells_item_bound(0, 1) == 1 && cells_item_bound(257, 1) == 5 && cells_item_bound(63, 4) == 4 && cells_item_bound((int64_t)1 << 24, (int64_t)1 << 20) == (1 << 18) + (1 << 20), "the bound");
   // the bound holds, and is reached, over distributions of n keys over c cells
   for (int c : {1, 2, 3, 33, 257, 1000})
      for (int n : {1, 63, 64, 65, 257, 4099, 100000}) {
         for (int trial = 0; trial < 6; trial++) {
            std::vector<uint32_t> m((size_t)c, 0);
            if (trial == 0) m[0] = (uint32_t)n;                                   // all keys in one cell
            else if (trial == 1) for (int i = 0; i < n; i++) m[(size_t)(i % c)]++;   // even
            else if (trial == 2) { for (int j = 0; j < c && j < n; j++) m[(size_t)j] = 1; m[(size_t)c - 1] += (uint32_t)(n > c ? n - c : 0); }   // one key per cell, the rest in the last
            else for (int i = 0; i < n; i++) m[(size_t)(rnd() % (uint32_t)c)]++;
            const std::vector<uint32_t> f = item_offsets(m);
            CHECK((int64_t)f.back() <= cells_item_bound(n, c), "c %d n %d trial %d: %u items, bound %lld", c, n, trial, f.back(), (long long)cells_item_bound(n, c));
            // every item finds the cell a linear walk finds, and that cell has keys for it
            uint32_t item = 0;
            for (int j = 0; j < c; j++)
               for (uint32_t q = 0; q < cells_items_of(m[(size_t)j]); q++, item++) {
                  const int got = cells_item_cell(f.data(), c, item);
                  CHECK(got == j && (item - f[(size_t)got]) * HS_CELLS_ITEM_KEYS < m[(size_t)got], "c %d n %d trial %d: item %u -> cell %d, not %d", c, n, trial, item, got, j);
               }
            CHECK(item == f.back(), "items walked");
         }
      }
   // n = 63 + 64 q keys with one key in each of c - 1 cells: floor(n / 64) + c items exactly where the remainders allow
   std::vector<uint32_t> m = {63, 1, 1, 1};
   CHECK(item_offsets(m).back() == 4 && cells_item_bound(66, 4) == 5, "66 keys in 4 cells");
}

static void check_mask()
{
   struct Cell { uint32_t lo, hi; };
   const Cell cells[] = {{0, 32}, {0, 31}, {0, 33}, {31, 32}, {31, 33}, {32, 33}, {32, 64}, {33, 64}, {33, 63}, {63, 65}, {64, 65}, {5, 9}, {100, 3300}, {0, 1}, {(1u << 20) - 1, 1u << 20}};
   for (const Cell &c : cells) {
      const int t0 = cells_first_tile(c.lo), t1 = cells_last_tile(c.hi);
      CHECK(t0 == (int)(c.lo / 32) && t1 == (int)((c.hi - 1) / 32) && t0 <= t1, "[%u, %u): tiles %d .. %d", c.lo, c.hi, t0, t1);
      uint32_t kept = 0;
      for (int t = t0; t <= t1; t++) {
         bool any = false;
         for (uint32_t r = 0; r < 32; r++) {
            const uint32_t row = (uint32_t)t * 32 + r;
            const bool masked = cells_row_masked(row, c.lo, c.hi);
            CHECK(masked == !(row >= c.lo && row < c.hi), "[%u, %u): row %u", c.lo, c.hi, row);
            any |= masked;
            kept += masked ? 0u : 1u;
         }
         CHECK(cells_tile_is_edge(t, c.lo, c.hi) == any, "[%u, %u): tile %d %s rows outside the cell", c.lo, c.hi, t, any ? "holds" : "holds no");
         if (t > t0 && t < t1) CHECK(!cells_tile_is_edge(t, c.lo, c.hi), "[%u, %u): an interior tile", c.lo, c.hi);
      }
      CHECK(kept == c.hi - c.lo && kept >= 1, "[%u, %u): the streamed tiles hold every row of the cell", c.lo, c.hi);
   }
}

static void check_slices()
{
   const int64_t S = HS_CELLS_SLICE_KEYS;
   CHECK(S == ((int64_t)1 << 24), "a slice is what training accepts");
   CHECK(cells_slice_count(0, S) == 0 && cells_slice_count(1, S) == 1 && cells_slice_count(S, S) == 1 && cells_slice_count(S + 1, S) == 2, "slice counts");
   CHECK(cells_slice_count((int64_t)1 << 38, S) == ((int64_t)1 << 14), "the longest source");
   for (int64_t slice : {(int64_t)1, (int64_t)64, (int64_t)100, S})
      for (int64_t n : {(int64_t)1, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)257, (int64_t)1000, 3 * slice, 3 * slice + 1, 3 * slice - 1}) {
         if (n < 1 || cells_slice_count(n, slice) > 5000) continue;
         int64_t next = 0;
         for (int64_t s = 0; s < cells_slice_count(n, slice); s++) {
            CHECK(cells_slice_begin(s, slice) == next, "n %lld slice %lld: slice %lld begins at %lld", (long long)n, (long long)slice, (long long)s, (long long)next);
            const int64_t m = cells_slice_keys(s, n, slice);
            CHECK(m >= 1 && m <= slice, "n %lld slice %lld: %lld keys", (long long)n, (long long)slice, (long long)m);
            next += m;
         }
         CHECK(next == n, "n %lld slice %lld: the slices cover the keys once", (long long)n, (long long)slice);
      }
}

static void check_grouping()
{
   for (int c : {1, 4, 33})
      for (int k : {33, 257}) {
         if (c > k) continue;
         std::vector<int32_t> cell((size_t)k), order((size_t)k), kept((size_t)c);
         std::vector<uint32_t> first((size_t)c + 1);
         for (int r = 0; r < k; r++) cell[(size_t)r] = (int32_t)(rnd() % (uint32_t)c);
         if (c > 2) for (int r = 0; r < k; r++) if (cell[(size_t)r] == 1) cell[(size_t)r] = 2;   // cell 1 receives no row
         const int n = cells_group_rows(cell.data(), k, c, order.data(), kept.data(), first.data());
         // against a stable sort
         std::vector<int32_t> want((size_t)k);
         for (int r = 0; r < k; r++) want[(size_t)r] = r;
         std::stable_sort(want.begin(), want.end(), [&](int32_t a, int32_t b) { return cell[(size_t)a] < cell[(size_t)b]; });
         CHECK(order == want, "c %d k %d: order", c, k);
         CHECK(cells_first_ok(first.data(), n, k), "c %d k %d: first is a layer of %d cells", c, k, n);
         CHECK(c <= 2 || n < c, "c %d k %d: the cell without rows was dropped", c, k);
         for (int j = 0; j < n; j++) {
            CHECK(j == 0 || kept[(size_t)j] > kept[(size_t)j - 1], "kept in order");
            for (uint32_t r = first[(size_t)j]; r < first[(size_t)j + 1]; r++)
               CHECK(cell[(size_t)order[r]] == kept[(size_t)j], "c %d k %d: row %u lies in cell %d", c, k, r, j);
         }
      }
}

struct Extent { const char *name; size_t off, bytes; };

static void check_arrays(int64_t cap, int64_t c)
{
   StagePlan p;
   const CellLayerArrays a = cell_layer_arrays(p, c);
   const CellScratch s = cell_scratch(p, cap, c);
   const std::vector<Extent> e = {{"tiles", a.tiles.off, a.tiles.bytes()}, {"norms", a.norms.off, a.norms.bytes()}, {"first", a.first.off, a.first.bytes()},
                                  {"coarse", s.coarse.off, s.coarse.bytes()}, {"perm", s.perm.off, s.perm.bytes()}, {"sub", s.sub.off, s.sub.bytes()},
                                  {"cursor", s.cursor.off, s.cursor.bytes()}, {"item_first", s.item_first.off, s.item_first.bytes()},
                                  {"block_sums", s.block_sums.off, s.block_sums.bytes()}, {"total", s.total.off, s.total.bytes()}};
   size_t end = 0;
   for (const Extent &x : e) {
      CHECK(x.off % 256 == 0 && x.off >= end && x.bytes > 0, "cap %lld c %lld: %s at %zu, the array before ends at %zu", (long long)cap, (long long)c, x.name, x.off, end);
      end = x.off + x.bytes;
   }
   CHECK(end == p.bytes(), "the end");
   const size_t entries = (size_t)c * (size_t)s.slots;
   CHECK(a.n_tiles == (c + 31) / 32 && a.tiles.count == (size_t)a.n_tiles * 4096 && a.norms.count == (size_t)a.n_tiles * 32 && a.first.count == (size_t)c + 1, "the layer");
   CHECK(s.coarse.count == (size_t)cap * 2 && s.perm.count == (size_t)cap, "12 bytes per key");
   CHECK(s.slots == accumulate_slots(c) && s.sub.count == entries && s.cursor.count == entries && s.item_first.count == (size_t)c + 1, "arrays of size c");
   CHECK(s.block_sums.count >= (entries + 4095) / 4096 + 1 && s.block_sums.count >= ((size_t)c + 4095) / 4096 + 1, "both scans' block sums");
   // 12 bytes per key and arrays of size c: nothing else grows with the keys
   StagePlan q;
   cell_scratch(q, 0, c);
   StagePlan w;
   cell_scratch(w, cap, c);
   CHECK(w.bytes() <= q.bytes() + (size_t)cap * 12 + 512, "cap %lld c %lld: %zu bytes", (long long)cap, (long long)c, w.bytes());
}

int main()
{
   check_first();
   check_items();
   check_mask();
   check_slices();
   check_grouping();
   for (int64_t c : {(int64_t)1, (int64_t)2, (int64_t)33, (int64_t)1024, (int64_t)4097, (int64_t)1 << 20})
      for (int64_t cap : {(int64_t)1, (int64_t)257, (int64_t)4099, (int64_t)1 << 24}) check_arrays(cap, c);
   if (g_failed) {
      fprintf(stderr, "%d checks failed\n", g_failed);
      return 1;
   }
   printf("cells_plan_check ok\n");
   return 0;
}
