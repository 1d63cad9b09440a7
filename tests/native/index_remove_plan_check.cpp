// index_remove_plan_check.cpp -- the host arithmetic of a removal from the image index (hesaff_amd/csrc/index_remove_plan.h) on the
// CPU: what a removal refuses, on both sides of every bound; the gone-flags of a call's numbers and the number they fail on; the
// remap at the smallest sizes and across the scan's block of 4096; the scratch; the bytes a removal holds at its peak.
// tests/test_index_remove_host.py builds it with AddressSanitizer + UBSan and runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../hesaff_amd/csrc/index_remove_plan.h"

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
   const int64_t N = (int64_t)1 << 20;
   CHECK(index_remove_ok(2, 1) && index_remove_ok(N, 1) && index_remove_ok(N, N - 1) && index_remove_ok(4097, 4096), "1 <= m <= N - 1");
   CHECK(!index_remove_ok(2, 0) && !index_remove_ok(N, 0) && !index_remove_ok(5, -1), "m = 0, m < 0");
   CHECK(!index_remove_ok(2, 2) && !index_remove_ok(N, N) && !index_remove_ok(1, 1) && !index_remove_ok(5, 6) && !index_remove_ok(5, INT64_MAX), "m = N, m > N");
   CHECK(!index_remove_ok(0, 1) && !index_remove_ok(-1, 1) && !index_remove_ok(N + 1, 1) && !index_remove_ok(1, 0), "no index of 0 or of more than 2^20 images; N = 1 keeps its image");
}

static void check_flags()
{
   std::vector<uint32_t> gone;
   int64_t bad = 77;
   const int32_t fine[3] = {4, 0, 2};
   CHECK(index_remove_flags(fine, 3, 5, gone, &bad) == HS_REMOVE_FINE && bad == 77, "numbers in any order");
   CHECK(gone.size() == 5 && gone[0] == 1 && gone[1] == 0 && gone[2] == 1 && gone[3] == 0 && gone[4] == 1, "the flags of 4, 0, 2");
   CHECK(index_remove_flags(fine, 0, 5, gone, &bad) == HS_REMOVE_FINE && gone.size() == 5 && gone[4] == 0, "no number: no flag");
   const int32_t below[2] = {3, -1}, above[2] = {5, 3}, far[1] = {INT32_MAX}, low[1] = {INT32_MIN};
   CHECK(index_remove_flags(below, 2, 5, gone, &bad) == HS_REMOVE_OUTSIDE && bad == -1, "a number of -1");
   CHECK(index_remove_flags(above, 2, 5, gone, &bad) == HS_REMOVE_OUTSIDE && bad == 5, "a number of N");
   CHECK(index_remove_flags(far, 1, 5, gone, &bad) == HS_REMOVE_OUTSIDE && bad == INT32_MAX, "the largest int");
   CHECK(index_remove_flags(low, 1, 5, gone, &bad) == HS_REMOVE_OUTSIDE && bad == INT32_MIN, "the smallest int");
   const int32_t twice[5] = {2, 0, 1, 4, 2}, pair[2] = {3, 3}, mixed[3] = {1, 1, 9};
   CHECK(index_remove_flags(twice, 5, 5, gone, &bad) == HS_REMOVE_TWICE && bad == 2, "a number twice, first against last position");
   CHECK(index_remove_flags(pair, 2, 5, gone, &bad) == HS_REMOVE_TWICE && bad == 3, "a number twice, side by side");
   CHECK(index_remove_flags(mixed, 3, 5, gone, &bad) == HS_REMOVE_TWICE && bad == 1, "the first fault in the order given is the one reported");
   // the largest call: every number of 2^20 but one, descending
   const int64_t N = (int64_t)1 << 20;
   std::vector<int32_t> all;
   for (int64_t i = N - 1; i >= 1; i--) all.push_back((int32_t)i);
   CHECK(index_remove_flags(all.data(), N - 1, N, gone, &bad) == HS_REMOVE_FINE && gone[0] == 0 && gone[1] == 1 && gone[(size_t)N - 1] == 1, "2^20 - 1 numbers");
   all.push_back((int32_t)(N / 2));
   CHECK(index_remove_flags(all.data(), N, N, gone, &bad) == HS_REMOVE_TWICE && bad == N / 2, "and one of them again");
}

static void check_remap()
{
   std::vector<int32_t> remap(1, 99);
   const uint32_t none[1] = {0};
   CHECK(index_remove_remap(none, 1, remap.data()) == 1 && remap[0] == 0, "N = 1: the image stays");
   const uint32_t first[2] = {1, 0}, last[2] = {0, 1};
   remap.assign(2, 99);
   CHECK(index_remove_remap(first, 2, remap.data()) == 1 && remap[0] == -1 && remap[1] == 0, "N = 2, the first goes");
   CHECK(index_remove_remap(last, 2, remap.data()) == 1 && remap[0] == 0 && remap[1] == -1, "N = 2, the last goes");
   // N = 4097: every second image, then all but the last
   const int64_t n = 4097;
   std::vector<uint32_t> gone((size_t)n, 0u);
   for (int64_t i = 0; i < n; i += 2) gone[(size_t)i] = 1u;
   remap.assign((size_t)n, 99);
   CHECK(index_remove_remap(gone.data(), n, remap.data()) == 2048, "every second of 4097: 2048 stay");
   bool ok = true;
   for (int64_t i = 0; i < n; i++) ok = ok && remap[(size_t)i] == (i % 2 ? (int32_t)(i / 2) : -1);
   CHECK(ok && remap[4095] == 2047 && remap[4096] == -1, "old image i becomes i - #{removed below i}");
   gone.assign((size_t)n, 1u);
   gone[4096] = 0u;
   CHECK(index_remove_remap(gone.data(), n, remap.data()) == 1 && remap[4096] == 0 && remap[4095] == -1 && remap[0] == -1, "all but the last of 4097");
}

static void check_working_set()
{
   const int64_t N = (int64_t)1 << 20, K = (int64_t)1 << 20, T = (int64_t)1 << 28;
   const size_t MiB = (size_t)1 << 20, GiB = (size_t)1 << 30;
   StagePlan s;
   const IndexRemoveArrays r = index_remove_arrays(s, N, K, false);
   CHECK(r.gone.count == (size_t)N && r.remap.count == (size_t)N && r.cursor.count == (size_t)K && r.key_count.count == 1 && r.key_offsets.count == 1, "the plain scratch");
   CHECK(r.block_sums.count == 257, "block sums for N = K = 2^20: 256 and one more");
   CHECK(r.removed.count == 1024 && HS_REMOVE_STRIPE_WORDS * sizeof(unsigned long long) == 128, "64 counters of the removed keys, a 128-byte line each");
   std::vector<unsigned long long> stripes(r.removed.count, 1000);
   for (int i = 0; i < HS_REMOVE_STRIPES; i++) stripes[(size_t)i * HS_REMOVE_STRIPE_WORDS] = (unsigned long long)i << 40;
   CHECK(index_remove_sum(stripes.data()) == (unsigned long long)(63 * 64 / 2) << 40, "their sum, and nothing of what lies between them");
   CHECK(s.bytes() >= 12 * MiB && s.bytes() < 13 * MiB, "the plain scratch: three arrays of 2^20 words (%zu)", s.bytes());
   StagePlan t;
   const IndexRemoveArrays q = index_remove_arrays(t, 8193, 33, true);
   CHECK(q.block_sums.count == 4 && q.key_count.count == 33 && q.key_offsets.count == 34 && q.key_cursor.count == 33, "block sums sized for N where N > K");
   // the largest index: N = K = 2^20, every key a posting of its own
   const size_t plain = index_remove_working_set_bytes(N, 1, K, T, T, false), embedded = index_remove_working_set_bytes(N, 1, K, T, T, true);
   printf("index_remove_working_set_bytes at N = K = 2^20, 2^28 postings: plain %zu (%.2f GiB), embedded %zu (%.2f GiB)\n", plain, (double)plain / GiB, embedded,
          (double)embedded / GiB);
   CHECK(plain >= 2 * GiB && plain < 2 * GiB + 64 * MiB, "plain: the lists are 2 GiB, tables and scratch below 64 MiB (%zu)", plain);
   CHECK(embedded >= 5 * GiB && embedded < 5 * GiB + 96 * MiB, "embedded: 3 GiB of key lists more (%zu)", embedded);
   CHECK(plain < index_working_set_bytes(N, K, T) / 3, "no hash table: a third of the build's working set at the most");
   // it grows with what it has to hold and does not depend on m but through the new tables
   CHECK(index_remove_working_set_bytes(N, N - 1, K, T, T, false) < plain, "fewer images left: smaller tables");
   CHECK(index_remove_working_set_bytes(2, 1, 1, 0, 0, false) < 64 * 1024, "the smallest removal");
}

int main()
{
   check_bounds();
   check_flags();
   check_remap();
   check_working_set();
   if (g_failed) {
      fprintf(stderr, "index_remove_plan_check: %d checks failed\n", g_failed);
      return 1;
   }
   printf("index_remove_plan_check ok\n");
   return 0;
}
