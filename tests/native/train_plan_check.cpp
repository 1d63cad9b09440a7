// train_plan_check.cpp -- the host arithmetic of vocabulary training (hesaff_amd/csrc/train_plan.h) on the CPU: the bounds of a call,
// the sampling index, the update rule against its definition, and the layout of the working arrays.
// tests/test_vocabulary_training_host.py builds it with AddressSanitizer + UBSan and runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../hesaff_amd/csrc/train_plan.h"

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

static void check_bounds()
{
   const int64_t N = (int64_t)1 << 24, K = (int64_t)1 << 20;
   CHECK(train_counts_ok(N, K, 1, false), "the largest call");
   CHECK(train_counts_ok(N, 1, 1, true) && train_counts_ok(1, 1, 1, false), "the smallest");
   CHECK(!train_counts_ok(N + 1, K, 1, false) && !train_counts_ok(N + 1, 1, 1, true), "n = 2^24 + 1");
   CHECK(!train_counts_ok(0, 1, 1, true) && !train_counts_ok(-1, 1, 1, true), "n < 1");
   CHECK(!train_counts_ok(N, K + 1, 1, true) && !train_counts_ok(N, 0, 1, true) && !train_counts_ok(N, -3, 1, true), "k outside 1 .. 2^20");
   CHECK(!train_counts_ok(N, K, 0, true) && !train_counts_ok(N, K, -1, true), "iterations < 1");
   CHECK(train_counts_ok(32, 33, 1, true) && !train_counts_ok(32, 33, 1, false) && train_counts_ok(33, 33, 1, false), "sampling needs n >= k");
   CHECK(!train_counts_ok((int64_t)1 << 40, 1, 1, true), "far beyond");
   CHECK(accumulate_counts_ok(N, K) && !accumulate_counts_ok(N + 1, K) && !accumulate_counts_ok(N, K + 1) && !accumulate_counts_ok(0, 1) && !accumulate_counts_ok(1, 0), "accumulation");
   // the reason for the bound: the largest sum fits uint32, the next size does not
   CHECK((uint64_t)N * 255 <= 0xffffffffull && (uint64_t)(N + (N >> 7)) * 255 > 0xffffffffull, "2^24 * 255 < 2^32");
   CHECK(word_source_ok(164, 36) && word_source_ok(128, 0) && word_source_ok(256, 128), "the sources of hesaff_assign_words_device");
   const int64_t bad[][2] = {{127, 0}, {124, 0}, {164, -4}, {164, 40}, {128, 4}, {166, 36}, {164, 38}, {164, 37}, {0, 0}};
   for (const auto &b : bad) CHECK(!word_source_ok(b[0], b[1]), "stride %lld offset %lld", (long long)b[0], (long long)b[1]);
}

static void check_sampling()
{
   const int64_t N = (int64_t)1 << 24, K = (int64_t)1 << 20;
   for (int64_t n : {(int64_t)1, (int64_t)33, (int64_t)257, K})   // n = k: the identity
      for (int64_t r = 0; r < n; r += (n > 4096 ? 4093 : 1)) CHECK(train_sample_index(r, n, n) == r, "n = k = %lld, row %lld", (long long)n, (long long)r);
   CHECK(train_sample_index(K - 1, K, K) == K - 1, "last row at n = k");
   // n = 2^24, k = 2^20: every 16th key; the product 2^44 needs 64 bits
   CHECK(train_sample_index(0, N, K) == 0 && train_sample_index(1, N, K) == 16 && train_sample_index(K - 1, N, K) == N - 16, "n = 2^24, k = 2^20");
   CHECK(train_sample_index(32, 257, 33) == 249 && train_sample_index(1, 257, 2) == 128 && train_sample_index(64, 257, 65) == 253, "n = 257");
   // strictly increasing and inside the keys whenever n >= k
   for (int64_t k : {(int64_t)1, (int64_t)2, (int64_t)33, (int64_t)65, (int64_t)4099})
      for (int64_t n : {k, k + 1, 2 * k - 1, (int64_t)4099, N}) {
         if (n < k) continue;
         int64_t last = -1;
         for (int64_t r = 0; r < k; r++) {
            const int64_t i = train_sample_index(r, n, k);
            CHECK(i > last && i < n, "n %lld k %lld row %lld -> %lld", (long long)n, (long long)k, (long long)r, (long long)i);
            last = i;
         }
      }
}

static void check_update_rule()
{
   CHECK(train_rounded_mean(0 + 1, 2) == 1, "{0, 1} -> 1: a half rounds up");
   CHECK(train_rounded_mean(0 + 0 + 1, 3) == 0, "{0, 0, 1} -> 0");
   CHECK(train_rounded_mean(255, 1) == 255 && train_rounded_mean(255u * 4099u, 4099) == 255, "all 255 stays 255");
   CHECK(train_rounded_mean(0xff000000u, 1u << 24) == 255 && train_rounded_mean(0, 1u << 24) == 0, "the largest sum: 2 sum + count needs 33 bits");
   CHECK(train_rounded_mean(0xff000000u - (1u << 23), 1u << 24) == 255 && train_rounded_mean(0xff000000u - (1u << 23) - 1, 1u << 24) == 254, "the half at the largest count");
   // against the definition: the integer v that minimises sum (d - v)^2 = count v^2 - 2 v sum + const, the larger one on a tie
   for (uint32_t count : {1u, 2u, 3u, 7u, 64u, 255u, 4099u})
      for (uint32_t sum = 0; sum <= 255u * count; sum += (count > 64 ? 37u : 1u)) {
         long long best = -1, best_cost = 0;
         for (long long v = 0; v <= 255; v++) {
            const long long cost = (long long)count * v * v - 2 * v * (long long)sum;
            if (best < 0 || cost <= best_cost) { best = v; best_cost = cost; }
         }
         CHECK(train_rounded_mean(sum, count) == (uint32_t)best, "sum %u count %u: %u, minimiser %lld", sum, count, train_rounded_mean(sum, count), best);
      }
}

struct Extent { const char *name; size_t off, bytes; };

static void check_arrays(int64_t n, int64_t k)
{
   StagePlan p;
   const TrainArrays t = train_arrays(p, n, k);
   const std::vector<Extent> e = {
      {"sums", t.acc.sums.off, t.acc.sums.bytes()}, {"counts", t.acc.counts.off, t.acc.counts.bytes()}, {"sub", t.acc.sub.off, t.acc.sub.bytes()}, {"cursor", t.acc.cursor.off, t.acc.cursor.bytes()},
      {"perm", t.acc.perm.off, t.acc.perm.bytes()}, {"block_sums", t.acc.block_sums.off, t.acc.block_sums.bytes()},
      {"stats", t.acc.stats.off, t.acc.stats.bytes()}, {"total", t.acc.total.off, t.acc.total.bytes()}, {"rows", t.rows.off, t.rows.bytes()},
      {"tiles", t.tiles.off, t.tiles.bytes()}, {"norms", t.norms.off, t.norms.bytes()}, {"assigned", t.assigned.off, t.assigned.bytes()}};
   size_t end = 0;
   for (const Extent &x : e) {
      CHECK(x.off % 256 == 0 && x.off >= end && x.bytes > 0, "n %lld k %lld: %s at %zu, the array before ends at %zu", (long long)n, (long long)k, x.name, x.off, end);
      end = x.off + x.bytes;
   }
   CHECK(end == p.bytes() && p.bytes() == train_working_set_bytes(n, k), "n %lld k %lld: %zu bytes", (long long)n, (long long)k, p.bytes());
   const size_t entries = (size_t)k * (size_t)t.acc.slots;
   CHECK(t.acc.sums.count == (size_t)k * 128 && t.acc.counts.count == (size_t)k && t.acc.perm.count == (size_t)n, "per word, per key");
   CHECK(t.acc.slots == accumulate_slots(k) && t.acc.sub.count == entries && t.acc.cursor.count == entries, "%d sub-counters per word", t.acc.slots);
   CHECK(t.acc.slots >= 1 && t.acc.slots <= 64 && (t.acc.slots & (t.acc.slots - 1)) == 0 && (t.acc.slots == 1 || entries <= 8192), "a power of two, k * slots <= 8192");
   CHECK(t.acc.chunks == accumulate_chunks(n) && t.acc.chunks >= 1 && t.acc.chunks <= 8, "%d chunks", t.acc.chunks);
   CHECK(t.rows.count == (size_t)k * 128 && t.assigned.count == (size_t)n * 2, "rows and (word, dist2)");
   CHECK(t.n_tiles == (k + 31) / 32 && t.tiles.count == (size_t)t.n_tiles * 4096 && t.norms.count == (size_t)t.n_tiles * 32, "whole tiles of 32 rows");
   CHECK(t.acc.block_sums.count >= (entries + 4095) / 4096 + 1, "a block sum per 4096 entries of the scan, and one");
}

int main()
{
   check_bounds();
   check_sampling();
   check_update_rule();
   CHECK(accumulate_slots(1) == 64 && accumulate_slots(33) == 64 && accumulate_slots(128) == 64 && accumulate_slots(129) == 32 && accumulate_slots(1000) == 8 &&
         accumulate_slots(4096) == 2 && accumulate_slots(4097) == 1 && accumulate_slots((int64_t)1 << 20) == 1, "sub-counters");
   CHECK(accumulate_chunks(1) == 1 && accumulate_chunks(4095) == 1 && accumulate_chunks(4096) == 2 && accumulate_chunks(4099) == 2 && accumulate_chunks(16383) == 7 &&
         accumulate_chunks(16384) == 8 && accumulate_chunks((int64_t)1 << 24) == 8, "walk lengths");
   for (int64_t k : {(int64_t)1, (int64_t)2, (int64_t)32, (int64_t)33, (int64_t)4096, (int64_t)4099, (int64_t)1 << 20})
      for (int64_t n : {(int64_t)1, (int64_t)257, (int64_t)4099, (int64_t)1 << 24}) check_arrays(n, k);
   // the largest call: about 1 GB, of which the sums are half
   const size_t largest = train_working_set_bytes((int64_t)1 << 24, (int64_t)1 << 20);
   CHECK(largest > ((size_t)960 << 20) && largest < ((size_t)1 << 30), "%zu bytes", largest);
   if (g_failed) {
      fprintf(stderr, "%d checks failed\n", g_failed);
      return 1;
   }
   printf("train_plan_check ok\n");
   return 0;
}
