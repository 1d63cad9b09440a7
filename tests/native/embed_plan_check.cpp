// embed_plan_check.cpp -- the host arithmetic of Hamming embedding (hesaff_amd/csrc/embed_plan.h) on the CPU: the refusals, the range
// of a projection value, the generator's first values, the packed projection against a plain dot product computed the way the kernel
// does (signed bytes plus the bias), the median's rank, the file heads on both sides of every rule, and the layouts.
// tests/test_embedding_host.py builds it with AddressSanitizer + UBSan and runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../hesaff_amd/csrc/embed_plan.h"

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
   std::vector<int8_t> P(HS_EMBED_P_BYTES, 127);
   CHECK(embed_projection_ok(P.data()) && !embed_projection_ok(nullptr), "all 127 is a projection, NULL is none");
   P[HS_EMBED_P_BYTES - 1] = -128;
   CHECK(!embed_projection_ok(P.data()), "-128 in the last entry");
   P[HS_EMBED_P_BYTES - 1] = -127; P[0] = -128;
   CHECK(!embed_projection_ok(P.data()), "-128 in the first entry");
   CHECK(embed_threshold_ok(0) && embed_threshold_ok(64) && !embed_threshold_ok(-1) && !embed_threshold_ok(65), "T in 0 .. 64");
   const int64_t N = (int64_t)1 << 24, K = (int64_t)1 << 20;
   CHECK(embed_train_counts_ok(1, 1) && embed_train_counts_ok(N, K) && !embed_train_counts_ok(0, 1) && !embed_train_counts_ok(N + 1, 1) &&
            !embed_train_counts_ok(1, 0) && !embed_train_counts_ok(1, K + 1), "n in 1 .. 2^24, k in 1 .. 2^20");
   CHECK(HS_EMBED_Z_MAX == 4145280 && HS_EMBED_Z_MAX < HS_EMBED_Z_BIAS && HS_EMBED_Z_BIAS == (1 << 22), "|z| < 2^22");
   CHECK(-HS_EMBED_Z_MAX + HS_EMBED_Z_BIAS > 0 && HS_EMBED_Z_MAX + HS_EMBED_Z_BIAS < (1 << HS_EMBED_Z_BITS), "z + 2^22 takes 23 bits");
   CHECK(embed_median_rank(1) == 0 && embed_median_rank(2) == 0 && embed_median_rank(3) == 1 && embed_median_rank(4) == 1 && embed_median_rank(65) == 32 &&
            embed_median_rank(1u << 24) == (1u << 23) - 1, "the lower median's rank");
}

static void check_generator()
{
   std::vector<int8_t> P(HS_EMBED_P_BYTES), Q(HS_EMBED_P_BYTES);
   // splitmix64's first output from 0 is 0xE220A8397B1DCDAF: top byte 0xE2 = 226 -> 98
   embedding_projection(0, P.data());
   CHECK(P[0] == 98, "seed 0, entry 0: %d", (int)P[0]);
   CHECK(embed_projection_ok(P.data()), "no entry of the default projection is -128");
   embedding_projection(~(uint64_t)0, Q.data());
   CHECK(embed_projection_ok(Q.data()) && memcmp(P.data(), Q.data(), P.size()) != 0, "seed 2^64 - 1");
   // seed + golden ratio shifts the stream by one entry
   embedding_projection(0x9E3779B97F4A7C15ull, Q.data());
   CHECK(memcmp(P.data() + 1, Q.data(), P.size() - 1) == 0, "the state advances by the constant");
}

// z as the kernel computes it from the packed projection: signed bytes d ^ 0x80 against the tiles in lane order, plus the bias
static void check_pack(uint64_t seed)
{
   std::vector<int8_t> P(HS_EMBED_P_BYTES);
   embedding_projection(seed, P.data());
   if (seed == 7) for (size_t e = 0; e < P.size(); e++) P[e] = 127;
   if (seed == 8) for (size_t e = 0; e < P.size(); e++) P[e] = -127;
   std::vector<uint8_t> tiles(HS_EMBED_P_BYTES, 0xAA);
   int32_t bias[HS_EMBED_BITS];
   embed_pack_projection(P.data(), tiles.data(), bias);
   uint8_t d[128];
   for (int j = 0; j < 128; j++) d[j] = seed >= 7 ? 255 : (uint8_t)((j * 37 + seed * 11) & 255);
   for (int row = 0; row < HS_EMBED_BITS; row++) {
      long long want = 0;
      for (int j = 0; j < 128; j++) want += (long long)P[(size_t)row * 128 + j] * d[j];
      const int t = row / 32, r = row % 32;
      long long dot = 0;
      for (int s = 0; s < 4; s++)
         for (int h = 0; h < 2; h++)
            for (int b = 0; b < 16; b++) {
               const int8_t p = (int8_t)tiles[((size_t)(t * 4 + s) * 64 + (size_t)(r + 32 * h)) * 16 + (size_t)b];
               dot += (long long)p * (int8_t)(d[32 * s + 16 * h + b] ^ 0x80);
            }
      CHECK(dot + bias[row] == want, "seed %llu row %d: %lld + %d, want %lld", (unsigned long long)seed, row, dot, bias[row], want);
      CHECK(dot < (1 << 21) && dot > -(1 << 21) && bias[row] < (1 << 21) && bias[row] > -(1 << 21), "each term below 2^21");
      CHECK(want <= HS_EMBED_Z_MAX && want >= -HS_EMBED_Z_MAX, "z inside its range");
      if (seed == 7) CHECK(want == HS_EMBED_Z_MAX, "the upper end");
      if (seed == 8) CHECK(want == -HS_EMBED_Z_MAX, "the lower end");
   }
}

static void check_files()
{
   char head[HS_EMBED_FILE_HEAD];
   embed_file_head(head, 33);
   CHECK(embed_file_bytes(33) == 24 + 8192 + 33 * 256 && embed_file_rows(head, embed_file_bytes(33)) == 33, "a whole embedding file");
   CHECK(embed_file_rows(head, embed_file_bytes(33) - 1) == -1 && embed_file_rows(head, embed_file_bytes(33) + 1) == -1 && embed_file_rows(head, 24) == -1, "size against k");
   for (int field = 0; field < 4; field++) {
      char bad[HS_EMBED_FILE_HEAD];
      memcpy(bad, head, sizeof bad);
      bad[8 + 4 * field] ^= 1;
      uint32_t k;
      memcpy(&k, bad + 16, 4);
      CHECK(embed_file_rows(bad, embed_file_bytes(k)) == -1 || field == 2, "field %d changed", field);
   }
   head[0] = 'X';
   CHECK(embed_file_rows(head, embed_file_bytes(33)) == -1, "the magic");
   embed_file_head(head, 0);
   CHECK(embed_file_rows(head, embed_file_bytes(0)) == -1, "k = 0");
   embed_file_head(head, (1u << 20) + 1);
   CHECK(embed_file_rows(head, embed_file_bytes((1u << 20) + 1)) == -1, "k = 2^20 + 1");
   embed_file_head(head, 1u << 20);
   CHECK(embed_file_rows(head, embed_file_bytes(1u << 20)) == (1 << 20), "k = 2^20");
   char sh[HS_SIGS_FILE_HEAD];
   sigs_file_head(sh, 0);
   CHECK(sigs_file_count(sh, 16) == 0 && sigs_file_count(sh, 24) == -1, "an image without keys");
   sigs_file_head(sh, 221);
   CHECK(sigs_file_count(sh, 16 + 8 * 221) == 221 && sigs_file_count(sh, 16 + 8 * 221 - 1) == -1 && sigs_file_count(sh, 16 + 8 * 222) == -1, "count against size");
   sh[8] = 32;
   CHECK(sigs_file_count(sh, 16 + 8 * 221) == -1, "bits other than 64");
   sigs_file_head(sh, 221);
   sh[7] = '2';
   CHECK(sigs_file_count(sh, 16 + 8 * 221) == -1, "the magic");
   sigs_file_head(sh, 0x80000000u);
   CHECK(sigs_file_count(sh, sigs_file_bytes(0x80000000u)) == -1, "a count beyond int");
}

struct Extent { const char *name; size_t off, bytes; };

static void check_layout(const std::vector<Extent> &e, size_t total, const char *what)
{
   size_t end = 0;
   for (const Extent &x : e) {
      CHECK(x.off % 256 == 0 && x.off >= end && x.bytes > 0, "%s: %s at %zu, the array before ends at %zu", what, x.name, x.off, end);
      end = x.off + x.bytes;
   }
   CHECK(end == total, "%s: %zu bytes, the last array ends at %zu", what, total, end);
}

static void check_arrays(int64_t n, int64_t k)
{
   StagePlan p;
   const EmbedArrays a = embed_arrays(p, k);
   check_layout({{"tiles", a.tiles.off, a.tiles.bytes()}, {"bias", a.bias.off, a.bias.bytes()}, {"tau", a.tau.off, a.tau.bytes()}}, p.bytes(), "embedding");
   CHECK(a.tiles.count == 8192 && a.bias.count == 64 && a.tau.count == (size_t)k * 64, "P, bias and a row of thresholds per word");
   StagePlan q;
   const EmbedTrainArrays t = embed_train_arrays(q, n, k);
   check_layout({{"tiles", t.tiles.off, t.tiles.bytes()}, {"bias", t.bias.off, t.bias.bytes()}, {"z", t.z.off, t.z.bytes()}, {"counts", t.counts.off, t.counts.bytes()},
                 {"sub", t.sub.off, t.sub.bytes()}, {"cursor", t.cursor.off, t.cursor.bytes()}, {"perm", t.perm.off, t.perm.bytes()},
                 {"block_sums", t.block_sums.off, t.block_sums.bytes()}, {"total", t.total.off, t.total.bytes()}, {"tau", t.tau.off, t.tau.bytes()}},
                q.bytes(), "training");
   CHECK(t.slots == accumulate_slots(k) && t.sub.count == (size_t)k * t.slots && t.cursor.count == t.sub.count, "the grouping's sub-counters");
   CHECK(t.z.count == (size_t)n * 64 && t.perm.count == (size_t)n && t.tau.count == (size_t)k * 64 && t.counts.count == (size_t)k, "per key and per word");
   CHECK(embed_train_working_set_bytes(n, k) == q.bytes(), "the working set");
   StagePlan r;
   const KeyListArrays l = key_list_arrays(r, k, n);
   check_layout({{"offsets", l.offsets.off, l.offsets.bytes()}, {"sig", l.sig.off, l.sig.bytes()}, {"image", l.image.off, l.image.bytes()}}, r.bytes(), "key lists");
   CHECK(l.offsets.count == (size_t)k + 1 && l.sig.count == (size_t)n && l.image.count == (size_t)n && l.sig.off % 8 == 0, "an aligned signature per key");
   StagePlan s;
   const KeyListArrays l0 = key_list_arrays(s, k, 0);
   CHECK(l0.sig.count == 1 && l0.image.count == 1, "an index without keys still has its arrays");
   StagePlan u;
   const KeyListBuildArrays b = key_list_build_arrays(u, k);
   check_layout({{"counts", b.counts.off, b.counts.bytes()}, {"block_sums", b.block_sums.off, b.block_sums.bytes()}}, u.bytes(), "key list build");
   CHECK(b.counts.count == (size_t)k && b.block_sums.count >= ((size_t)k + 4095) / 4096 + 1, "the cursor and the scan's block sums");
}

int main()
{
   check_bounds();
   check_generator();
   for (uint64_t seed : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)7, (uint64_t)8}) check_pack(seed);
   check_files();
   for (int64_t n : {(int64_t)1, (int64_t)65, (int64_t)4099, (int64_t)1 << 24})
      for (int64_t k : {(int64_t)1, (int64_t)33, (int64_t)4099, (int64_t)1 << 20}) check_arrays(n, k);
   const size_t largest = embed_train_working_set_bytes((int64_t)1 << 24, (int64_t)1 << 20);
   CHECK(largest > ((size_t)4 << 30) && largest < ((size_t)5 << 30), "%zu bytes", largest);
   if (g_failed) {
      fprintf(stderr, "%d checks failed\n", g_failed);
      return 1;
   }
   printf("embed_plan_check ok\n");
   return 0;
}
