// probes_plan_check.cpp -- the host arithmetic of vocabulary probes (hesaff_amd/csrc/cells_plan.h) on the CPU: the accepted probe
// counts and P' = min(P, C), the keys of a slice and that its entries stay within what the grouping is sized for, the work-item bound
// against the items of constructed distributions of n P' entries, the entry -> (key, rank) map, the slices of a source longer than a
// slice, and the layout of the working arrays - at P' = 1 byte for byte cell_scratch's.
// tests/test_vocabulary_probes_host.py builds it with AddressSanitizer + UBSan and runs it.
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

static void check_counts()
{
   CHECK(HS_CELLS_MAX_PROBES == 8, "the bound of the header");
   CHECK(!cells_probes_ok(0) && !cells_probes_ok(-1) && !cells_probes_ok(9) && !cells_probes_ok((int64_t)1 << 32), "outside 1..8");
   for (int p = 1; p <= 8; p++) {
      CHECK(cells_probes_ok(p), "P = %d", p);
      for (int64_t c : {(int64_t)1, (int64_t)2, (int64_t)3, (int64_t)7, (int64_t)8, (int64_t)9, (int64_t)1 << 20})
         CHECK(cells_probes_used(p, c) == (p < c ? p : (int)c) && cells_probes_used(p, c) >= 1, "P = %d, C = %lld", p, (long long)c);
   }
}

static void check_slices()
{
   const int64_t S = (int64_t)1 << 24;
   for (int p = 1; p <= 8; p++) {
      const int64_t keys = cells_probe_slice_keys(p);
      CHECK(keys == S / p && keys >= 1, "P = %d: %lld keys", p, (long long)keys);
      CHECK(cells_probe_entries(keys, p) <= S && cells_probe_entries(keys + 1, p) > S, "P = %d: the entries of a slice fit, one key more does not", p);
      CHECK(cells_probe_entries(keys, p) <= 0x7fffffff, "an int count");
      // a source of more than a slice: the slices cover the keys once, none beyond the bound
      for (int64_t n : {keys - 1, keys, keys + 1, 3 * keys, 3 * keys + 5}) {
         int64_t next = 0;
         for (int64_t s = 0; s < cells_slice_count(n, keys); s++) {
            CHECK(cells_slice_begin(s, keys) == next, "P = %d n %lld: slice %lld", p, (long long)n, (long long)s);
            const int64_t m = cells_slice_keys(s, n, keys);
            CHECK(m >= 1 && m <= keys && cells_probe_entries(m, p) <= S, "P = %d n %lld: %lld keys", p, (long long)n, (long long)m);
            next += m;
         }
         CHECK(next == n, "P = %d n %lld: covered once", p, (long long)n);
      }
   }
   CHECK(cells_probe_slice_keys(1) == HS_CELLS_SLICE_KEYS, "one probe: the slice of the cells path");
}

// the items of n P' entries distributed over c cells, a key at most once in a cell, against the bound floor(n P' / 64) + c
static void check_items()
{
   for (int c : {1, 2, 3, 8, 33, 257, 1000})
      for (int p = 1; p <= 8; p++) {
         const int used = cells_probes_used(p, c);
         for (int n : {1, 7, 8, 9, 63, 64, 65, 257, 4099, 100000}) {
            const int64_t entries = cells_probe_entries(n, used), bound = cells_probe_item_bound(n, used, c);
            CHECK(entries == (int64_t)n * used && bound == entries / 64 + c && bound == cells_item_bound(entries, c), "c %d P %d n %d: the bound", c, p, n);
            for (int trial = 0; trial < 3; trial++) {
               std::vector<uint32_t> m((size_t)c, 0);
               if (trial == 0) m[0] = (uint32_t)entries;                                           // all in one cell (more than probes can put there: the bound holds all the same)
               else if (trial == 1) for (int64_t e = 0; e < entries; e++) m[(size_t)(e % c)]++;    // even: every key probes P' cells in turn
               else {   // one entry per cell, the rest in the last
                  for (int j = 0; j < c && j < entries; j++) m[(size_t)j] = 1;
                  m[(size_t)c - 1] += (uint32_t)(entries > c ? entries - c : 0);
               }
               int64_t items = 0, sum = 0;
               for (int j = 0; j < c; j++) { items += cells_items_of(m[(size_t)j]); sum += m[(size_t)j]; }
               CHECK(sum == entries, "c %d P %d n %d trial %d: %lld entries placed", c, p, n, trial, (long long)sum);
               CHECK(items <= bound, "c %d P %d n %d trial %d: %lld items, bound %lld", c, p, n, trial, (long long)items, (long long)bound);
            }
         }
      }
   // reached: 63 entries in one cell and one in each of three others
   CHECK(cells_probe_item_bound(33, 2, 4) == 5, "66 entries in 4 cells");
}

static void check_entries()
{
   for (uint32_t used = 1; used <= 8; used++) {
      uint32_t e = 0;
      for (uint32_t key = 0; key < 300; key++)
         for (uint32_t rank = 0; rank < used; rank++, e++)
            CHECK(cells_entry_key(e, used) == key && e - cells_entry_key(e, used) * used == rank, "P' = %u: entry %u", used, e);
      const uint32_t last = (uint32_t)cells_probe_entries(cells_probe_slice_keys(used), used) - 1u;
      CHECK(cells_entry_key(last, used) == (uint32_t)cells_probe_slice_keys(used) - 1u, "P' = %u: the last entry of a slice", used);
   }
}

struct Extent { const char *name; size_t off, bytes; };

static void check_scratch(int64_t cap, int64_t c)
{
   // P' = 1: cell_scratch's layout byte for byte, nothing added
   StagePlan p1, p0;
   const ProbeScratch one = probe_scratch(p1, cap, c, 1);
   const CellScratch base = cell_scratch(p0, cap, c);
   CHECK(p1.bytes() == p0.bytes() && one.fine.count == 0 && one.used == 1, "cap %lld c %lld: %zu bytes, not %zu", (long long)cap, (long long)c, p1.bytes(), p0.bytes());
   CHECK(one.s.coarse.off == base.coarse.off && one.s.coarse.count == base.coarse.count && one.s.perm.off == base.perm.off && one.s.perm.count == base.perm.count, "keys' arrays");
   CHECK(one.s.sub.off == base.sub.off && one.s.cursor.off == base.cursor.off && one.s.item_first.off == base.item_first.off && one.s.block_sums.off == base.block_sums.off &&
         one.s.total.off == base.total.off && one.s.slots == base.slots, "arrays of size c");
   for (int used = 2; used <= 8; used++) {
      if (cap > cells_probe_slice_keys(used)) continue;
      StagePlan p;
      const ProbeScratch s = probe_scratch(p, cap, c, used);
      const size_t entries = (size_t)cap * (size_t)used;
      CHECK(s.used == used && s.s.coarse.count == entries * 2 && s.s.perm.count == entries && s.fine.count == entries * 2, "cap %lld P' %d: (8 + 4 + 8) P' bytes per key", (long long)cap, used);
      const std::vector<Extent> e = {{"coarse", s.s.coarse.off, s.s.coarse.bytes()}, {"perm", s.s.perm.off, s.s.perm.bytes()}, {"sub", s.s.sub.off, s.s.sub.bytes()},
                                     {"cursor", s.s.cursor.off, s.s.cursor.bytes()}, {"item_first", s.s.item_first.off, s.s.item_first.bytes()},
                                     {"block_sums", s.s.block_sums.off, s.s.block_sums.bytes()}, {"total", s.s.total.off, s.s.total.bytes()},
                                     {"fine", s.fine.off, s.fine.bytes()}};
      size_t end = 0;
      for (const Extent &x : e) {
         CHECK(x.off % 256 == 0 && x.off >= end && x.bytes > 0, "cap %lld c %lld P' %d: %s at %zu, the array before ends at %zu", (long long)cap, (long long)c, used, x.name, x.off, end);
         end = x.off + x.bytes;
      }
      CHECK(end == p.bytes(), "the end");
      CHECK(s.s.sub.count == base.sub.count && s.s.cursor.count == base.cursor.count && s.s.item_first.count == base.item_first.count, "the arrays of size c do not grow with P'");
      StagePlan q;
      probe_scratch(q, 0, c, used);
      CHECK(p.bytes() <= q.bytes() + (size_t)cap * 20 * (size_t)used + 768, "cap %lld c %lld P' %d: %zu bytes", (long long)cap, (long long)c, used, p.bytes());
   }
}

int main()
{
   check_counts();
   check_slices();
   check_items();
   check_entries();
   for (int64_t c : {(int64_t)1, (int64_t)2, (int64_t)33, (int64_t)1024, (int64_t)4097, (int64_t)1 << 20})
      for (int64_t cap : {(int64_t)1, (int64_t)257, (int64_t)4099, (int64_t)1 << 21, (int64_t)1 << 24}) check_scratch(cap, c);
   if (g_failed) {
      fprintf(stderr, "%d checks failed\n", g_failed);
      return 1;
   }
   printf("probes_plan_check ok\n");
   return 0;
}
