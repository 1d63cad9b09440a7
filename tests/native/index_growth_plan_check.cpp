// index_growth_plan_check.cpp -- the host arithmetic of the growing, durable index (hesaff_amd/csrc/index_plan.h) on the CPU: what
// an add refuses, on both sides of every bound; the bytes an add holds at its peak, against the build's; the layout, the head and
// the head's rules of the index file; the rules of the load's device pass in their order.
// tests/test_index_growth_host.py builds it with AddressSanitizer + UBSan and runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../hesaff_amd/csrc/index_plan.h"

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

static void check_add_bounds()
{
   const int64_t N = (int64_t)1 << 20, C = (int64_t)1 << 18, T = (int64_t)1 << 28;
   CHECK(index_add_ok(1, 1, 0, 0), "the smallest add: one image without keys behind one image without keys");
   CHECK(index_add_ok(N - 1, 1, 0, 0) && index_add_ok(1, N - 1, 0, 0) && index_add_ok(N / 2, N / 2, 0, 0), "N + m = 2^20");
   CHECK(!index_add_ok(N, 1, 0, 0) && !index_add_ok(1, N, 0, 0) && !index_add_ok(N / 2, N / 2 + 1, 0, 0), "N + m = 2^20 + 1");
   CHECK(!index_add_ok(1, 0, 0, 0) && !index_add_ok(1, -1, 0, 0), "m < 1");
   CHECK(!index_add_ok(0, 1, 0, 0) && !index_add_ok(-1, 1, 0, 0) && !index_add_ok(N + 1, 1, 0, 0), "no index of 0 or of more than 2^20 images");
   CHECK(!index_add_ok(1, (int64_t)1 << 40, 0, 0) && !index_add_ok(1, INT64_MAX, 0, 0), "an m that would wrap the sum");
   CHECK(index_add_ok(5, 5, T - 1, 1) && index_add_ok(5, 5, 0, T) && index_add_ok(5, 5, T, 0) && index_add_ok(5, 5, T / 2, T / 2), "keys = 2^28");
   CHECK(!index_add_ok(5, 5, T, 1) && !index_add_ok(5, 5, 1, T) && !index_add_ok(5, 5, T / 2 + 1, T / 2), "keys = 2^28 + 1");
   CHECK(!index_add_ok(5, 5, -1, 1) && !index_add_ok(5, 5, 1, -1) && !index_add_ok(5, 5, T + 1, 0) && !index_add_ok(5, 5, INT64_MAX, INT64_MAX), "key counts out of range");
   // the counts of the new images: the rule is the build's, and -1 is what the entry points refuse
   const int32_t ok[3] = {0, (int32_t)C, 7}, over[2] = {1, (int32_t)C + 1}, neg[1] = {-1};
   CHECK(index_total_keys(ok, 3) == C + 7 && index_total_keys(over, 2) == -1 && index_total_keys(neg, 1) == -1, "a count of 2^18 + 1");
}

static void check_working_set()
{
   const int64_t N = (int64_t)1 << 20, K = (int64_t)1 << 20, C = (int64_t)1 << 18, T = (int64_t)1 << 28;
   // one image of 2^18 keys behind the largest index: the lists are all of it, the hash table is sized for the new keys alone
   const size_t add = index_add_working_set_bytes(N - 1, 1, K, T - C, C), build = index_working_set_bytes(N, K, T);
   StagePlan scratch;
   const IndexBuildArrays b = index_build_arrays(scratch, 1, K, C);
   CHECK(b.bits == 19 && b.slots == ((uint64_t)1 << 19), "2^19 slots for 2^18 new keys, not 2^29 for all: %d bits", b.bits);
   CHECK(add > ((size_t)2 << 30) && add < ((size_t)2 << 30) + ((size_t)64 << 20), "the add's peak is the 2 GiB of lists and some MiB: %zu", add);
   CHECK(build > ((size_t)8 << 30) && add * 3 < build, "the build of the same collection holds more than three times as much: %zu against %zu", build, add);
   printf("working set: add of one image to the largest index %zu bytes (scratch %zu), its rebuild %zu bytes\n", add, scratch.bytes(), build);
   // the pieces: the new tables, the scratch, the lists
   StagePlan a;
   index_arrays(a, N, K);
   CHECK(add == a.bytes() + scratch.bytes() + index_lists_bytes(T), "the sum of its parts");
   // growing by images without keys: no lists beyond the old ones, the smallest table
   StagePlan s0;
   const IndexBuildArrays b0 = index_build_arrays(s0, 3, 33, 0);
   CHECK(b0.slots == 1024, "the smallest table");
   StagePlan a0;
   index_arrays(a0, 5, 33);
   CHECK(index_add_working_set_bytes(2, 3, 33, 10, 0) == a0.bytes() + s0.bytes() + index_lists_bytes(10), "m images without keys");
}

static void check_file_layout()
{
   CHECK(HS_INDEX_FILE_HEAD == 40, "the head");
   for (uint32_t k : {1u, 2u, 33u, 300u, 1u << 20})
      for (uint64_t keys : {(uint64_t)0, (uint64_t)1, (uint64_t)7, (uint64_t)64})
         for (uint32_t flags : {0u, 1u}) {
            IndexFileHead h;
            h.flags = flags; h.k = k; h.n_images = 5; h.n_keys = keys; h.n_postings = keys / 2;
            const IndexFileLayout l = index_file_layout(h);
            CHECK(l.df == 40 && l.postings % 8 == 0 && l.key_count % 8 == 0 && l.key_image % 8 == 0 && l.key_sig % 8 == 0 && l.size % 8 == 0, "every array on 8 bytes");
            CHECK(l.postings >= l.df + (size_t)k * 4 && l.postings < l.df + (size_t)k * 4 + 8, "df and at most a pad");
            CHECK(l.key_count == l.postings + h.n_postings * 8, "the postings");
            if (!flags) CHECK(l.key_image == l.key_count && l.key_sig == l.key_count && l.size == l.key_count, "a plain file ends behind the postings");
            else CHECK(l.key_image >= l.key_count + (size_t)k * 4 && l.key_sig >= l.key_image + keys * 4 && l.key_sig < l.key_image + keys * 4 + 8 && l.size == l.key_sig + keys * 8,
                       "an embedded file's three arrays");
            char head[HS_INDEX_FILE_HEAD];
            index_file_head(head, h);
            IndexFileHead g;
            CHECK(index_file_parse_head(head, l.size, &g) && g.flags == h.flags && g.k == h.k && g.n_images == h.n_images && g.n_keys == h.n_keys && g.n_postings == h.n_postings,
                  "the head reads back");
            CHECK(!index_file_parse_head(head, l.size - 1, &g) && !index_file_parse_head(head, l.size + 1, &g) && !index_file_parse_head(head, l.size + 8, &g), "a short and a long file");
         }
   IndexFileHead h;
   h.flags = 1; h.k = 33; h.n_images = 4; h.n_keys = 9; h.n_postings = 6;
   const size_t size = index_file_layout(h).size;
   CHECK(size == 40 + 136 + 48 + 136 + 40 + 72, "K = 33: 132 bytes of df and 4 of pad; 9 key images and 4 of pad: %zu", size);
   char good[HS_INDEX_FILE_HEAD], bad[HS_INDEX_FILE_HEAD];
   index_file_head(good, h);
   CHECK(memcmp(good, "HESAFFI1", 8) == 0 && good[8] == 1 && good[12] == 33 && good[16] == 4 && good[20] == 0 && good[24] == 9 && good[32] == 6, "little-endian fields in order");
   IndexFileHead g;
   struct { int at; char v; const char *what; } cases[] = {{7, '2', "magic"}, {0, 'h', "magic"}, {8, 3, "unknown flags"}, {11, 1, "unknown flags"}, {20, 1, "reserved"},
                                                           {23, (char)0x80, "reserved"}};
   for (const auto &c : cases) {
      memcpy(bad, good, sizeof bad);
      bad[c.at] = c.v;
      CHECK(!index_file_parse_head(bad, size, &g), "%s", c.what);
   }
   // counts out of bounds, each with the size its own fields imply
   const int64_t M = (int64_t)1 << 20, T = (int64_t)1 << 28;
   struct { int64_t k, n, keys, postings; bool ok; } counts[] = {{1, 1, 0, 0, true}, {M, M, 0, 0, true}, {0, 1, 0, 0, false}, {M + 1, 1, 0, 0, false}, {1, 0, 0, 0, false},
                                                                {1, M + 1, 0, 0, false}, {1, 1, T, T, true}, {1, 1, T + 1, 1, false}, {1, 1, 5, 6, false}, {1, 1, 5, 5, true}};
   for (const auto &c : counts) {
      IndexFileHead q;
      q.flags = 0; q.k = (uint32_t)c.k; q.n_images = (uint32_t)c.n; q.n_keys = (uint64_t)c.keys; q.n_postings = (uint64_t)c.postings;
      index_file_head(bad, q);
      CHECK(index_file_parse_head(bad, index_file_layout(q).size, &g) == c.ok, "k %lld, n %lld, keys %lld, postings %lld", (long long)c.k, (long long)c.n, (long long)c.keys,
            (long long)c.postings);
   }
   // fields that would wrap a 32-bit size
   IndexFileHead huge;
   huge.flags = 1; huge.k = 0xffffffffu; huge.n_images = 1; huge.n_keys = ~(uint64_t)0; huge.n_postings = ~(uint64_t)0;
   index_file_head(bad, huge);
   CHECK(!index_file_parse_head(bad, 40, &g) && !index_file_parse_head(bad, index_file_layout(huge).size, &g), "all-ones fields");
}

static void check_load_rules()
{
   const uint32_t bits[6] = {HS_LOAD_IMAGE, HS_LOAD_TF, HS_LOAD_IMAGE_SUM, HS_LOAD_TOTAL, HS_LOAD_KEY_COUNT, HS_LOAD_KEY_IMAGE};
   uint32_t all = 0;
   for (int i = 0; i < 6; i++) {
      CHECK(bits[i] == (1u << i), "one bit each, in the order of the header");
      all |= bits[i];
   }
   CHECK(index_load_rule(0)[0] == 0, "no flag, no rule");
   for (int i = 0; i < 6; i++) {
      const char *alone = index_load_rule(bits[i]);
      CHECK(alone[0] != 0 && strcmp(alone, index_load_rule(all & ~(bits[i] - 1))) == 0, "the lowest bit names the rule");
      for (int j = 0; j < i; j++) CHECK(strcmp(alone, index_load_rule(bits[j])) != 0, "six different rules");
   }
}

int main()
{
   check_add_bounds();
   check_working_set();
   check_file_layout();
   check_load_rules();
   if (g_failed) { fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
   printf("index_growth_plan_check ok\n");
   return 0;
}
