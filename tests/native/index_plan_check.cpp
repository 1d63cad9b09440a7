// index_plan_check.cpp -- the host arithmetic of the image index (hesaff_amd/csrc/index_plan.h) on the CPU: the bounds of a build and
// of a query, the integer logarithm behind idf with its intermediate products checked in 128 bits, the worst-case sums, the size rule
// of the hash table, the packing of host words and the key starts of a build, an add and a batch's chunk, and the layouts of the
// persistent arrays and of the build's scratch.
// tests/test_image_index_host.py builds it with AddressSanitizer + UBSan and runs it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
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

typedef unsigned __int128 u128;

static void check_bounds()
{
   const int64_t N = (int64_t)1 << 20, K = (int64_t)1 << 20, C = (int64_t)1 << 18, T = (int64_t)1 << 28;
   CHECK(index_counts_ok(1, 1) && index_counts_ok(N, K), "the smallest and the largest index");
   CHECK(!index_counts_ok(0, 1) && !index_counts_ok(-1, 1) && !index_counts_ok(N + 1, 1), "n_images outside 1 .. 2^20");
   CHECK(!index_counts_ok(1, 0) && !index_counts_ok(1, -1) && !index_counts_ok(1, K + 1), "k outside 1 .. 2^20");
   CHECK(index_image_keys_ok(0) && index_image_keys_ok(C) && !index_image_keys_ok(C + 1) && !index_image_keys_ok(-1), "keys of an image: 0 .. 2^18");
   CHECK(index_total_ok(0) && index_total_ok(T) && !index_total_ok(T + 1) && !index_total_ok(-1), "keys of a build: 0 .. 2^28");
   CHECK(index_word_stride_ok(1) && index_word_stride_ok(2) && !index_word_stride_ok(0) && !index_word_stride_ok(3) && !index_word_stride_ok(-1), "word_stride 1 or 2");
   CHECK(index_query_ok(0, 1) && index_query_ok(C, 1024) && !index_query_ok(C + 1, 1) && !index_query_ok(-1, 1), "a query's keys: 0 .. 2^18");
   CHECK(!index_query_ok(1, 0) && !index_query_ok(1, 1025) && !index_query_ok(1, -1), "top outside 1 .. 1024");
   const int32_t ok[3] = {0, (int32_t)C, 5}, over[2] = {3, (int32_t)C + 1}, neg[2] = {-1, 4};
   CHECK(index_total_keys(ok, 3) == C + 5 && index_total_keys(over, 2) == -1 && index_total_keys(neg, 2) == -1, "the sum of the counts");
   std::vector<int32_t> full(1025, (int32_t)C);   // 1024 x 2^18 = 2^28 keys: the largest build; one image more is refused
   CHECK(index_total_keys(full.data(), 1024) == T && index_total_keys(full.data(), 1025) == -1, "2^28 keys and 2^28 + 2^18");
}

// ilog2_q8 with every intermediate checked in 128 bits
static uint32_t checked_ilog2(uint64_t n, uint64_t df)
{
   const u128 q128 = ((u128)n << 31) / df;
   CHECK(q128 >= ((u128)1 << 31) && q128 < ((u128)1 << 55), "q of %llu / %llu", (unsigned long long)n, (unsigned long long)df);
   uint64_t q = (uint64_t)q128;
   int e = 0;
   while ((q >> e) >= ((uint64_t)1 << 32)) e++;
   uint64_t m = q >> e;
   uint32_t r = (uint32_t)e;
   for (int i = 0; i < 8; i++) {
      CHECK(m >= ((uint64_t)1 << 31) && m < ((uint64_t)1 << 32), "m before squaring %d", i);
      const u128 sq = (u128)m * m;
      CHECK(sq < ((u128)1 << 64), "m * m fits uint64");
      m = (uint64_t)(sq >> 31);
      r *= 2;
      if (m >= ((uint64_t)1 << 32)) { r += 1; m >>= 1; }
   }
   return r;
}

static void check_ilog2()
{
   CHECK(ilog2_q8(5, 5) == 0 && ilog2_q8(1, 1) == 0 && ilog2_q8(1 << 20, 1 << 20) == 0, "df = N: 0");
   CHECK(ilog2_q8(4, 1) == 512 && ilog2_q8(1 << 20, 1 << 18) == 512, "N / df = 4: 512");
   CHECK(ilog2_q8(3, 2) == 149, "3 / 2: 149, got %u", ilog2_q8(3, 2));
   CHECK(ilog2_q8((1 << 24) - 1, 1) == 6143 && HS_INDEX_MAX_IDF == 6143, "N = 2^24 - 1, df = 1: 6143, got %u", ilog2_q8((1 << 24) - 1, 1));
   CHECK(ilog2_q8(1 << 20, 1) == 5120 && ilog2_q8((1 << 20) - 1, 1) == 5119, "N = 2^20, df = 1: 5120");
   CHECK(index_idf(7, 0) == 0 && index_idf(7, 7) == 0 && index_idf(4, 1) == 512, "idf: 0 where df = 0");
   // a sweep: every df at small N, and strides of df at N = 2^20, 2^20 - 1 and 2^24 - 1; the header's function against the checked
   // one, against the logarithm within one unit, and monotone in df
   for (uint64_t n : {(uint64_t)1, (uint64_t)2, (uint64_t)3, (uint64_t)65, (uint64_t)257, (uint64_t)4099})
      for (uint64_t df = 1; df <= n; df++) {
         const uint32_t r = ilog2_q8(n, df);
         CHECK(r == checked_ilog2(n, df), "n %llu df %llu", (unsigned long long)n, (unsigned long long)df);
         const double want = 256.0 * std::log2((double)n / (double)df);
         CHECK(std::fabs((double)r - std::floor(want)) <= 1.0, "n %llu df %llu: %u, 256 log2 = %.6f", (unsigned long long)n, (unsigned long long)df, r, want);
      }
   for (uint64_t n : {(uint64_t)1 << 20, ((uint64_t)1 << 20) - 1, ((uint64_t)1 << 24) - 1}) {
      uint32_t last = 0xffffffffu;
      for (uint64_t df = 1; df <= n; df += (df < 4096 ? 1 : 997)) {
         const uint32_t r = ilog2_q8(n, df);
         CHECK(r == checked_ilog2(n, df) && r <= last && r <= HS_INDEX_MAX_IDF, "n %llu df %llu: %u after %u", (unsigned long long)n, (unsigned long long)df, r, last);
         last = r;
      }
   }
}

static void check_sums()
{
   // the largest terms and sums of the definition, in 128 bits: each below 2^62, so below 2^64
   const u128 idf = HS_INDEX_MAX_IDF, keys = (u128)HS_INDEX_MAX_IMAGE_KEYS;
   CHECK(idf * idf < ((u128)1 << 26), "idf^2 < 2^26");
   const u128 term = (keys * idf) * (keys * idf);          // one word holds every key of an image
   const u128 dot = keys * keys * idf * idf;               // ... and of the query
   CHECK(term < ((u128)1 << 62) && dot < ((u128)1 << 62), "the largest norm2, nq2 and dot");
   CHECK(keys * idf < ((u128)1 << 31), "tf * idf fits 31 bits");
   // spreading the keys over more words only lowers a sum of squares: sum tf^2 <= (sum tf)^2
   const u128 spread = (keys / 2) * (keys / 2) * 2 * idf * idf;
   CHECK(spread < term, "two words of 2^17 keys each");
   CHECK(index_key(HS_INDEX_MAX_IMAGES - 1, HS_INDEX_MAX_WORDS - 1) == (((uint64_t)1 << 40) - 1) && index_key(0, 0) == 0, "the key takes 40 bits");
   CHECK(index_key(HS_INDEX_MAX_IMAGES - 1, HS_INDEX_MAX_WORDS - 1) != HS_INDEX_EMPTY, "no key is the empty mark");
   CHECK(index_key_image(index_key(12345, 54321)) == 12345 && index_key_word(index_key(12345, 54321)) == 54321, "the key's halves");
}

static void check_hash()
{
   CHECK(index_hash_slots(0) == 1024 && index_hash_slots(1) == 1024 && index_hash_slots(511) == 1024 && index_hash_slots(512) == 1024, "at least 1024 slots");
   CHECK(index_hash_slots(513) == 2048 && index_hash_slots(1024) == 2048 && index_hash_slots(1025) == 4096, "the power of two that is at least 2 T");
   CHECK(index_hash_slots((int64_t)1 << 28) == ((uint64_t)1 << 29) && index_hash_bits((int64_t)1 << 28) == 29, "T = 2^28: 2^29 slots");
   for (int64_t t : {(int64_t)0, (int64_t)1, (int64_t)511, (int64_t)512, (int64_t)513, (int64_t)4099, (int64_t)1 << 28}) {
      const uint64_t s = index_hash_slots(t);
      CHECK((s & (s - 1)) == 0 && s >= 1024 && s >= 2 * (uint64_t)t && (s == 1024 || s / 2 < 2 * (uint64_t)t), "T = %lld: %llu slots", (long long)t, (unsigned long long)s);
      const int bits = index_hash_bits(t);
      for (uint64_t key : {(uint64_t)0, (uint64_t)1, ((uint64_t)1 << 40) - 1, (uint64_t)0x123456789ull})
         CHECK(index_hash_slot(key, bits) < s, "the first slot lies inside the table");
   }
}

// index_stage_words: the packing of host words at strides 1, 2 and 3, n = 0, k = 1, and the first and the last word out of range on
// either side.  The source arrays are exactly as long as the walk (1 + (n - 1) stride words), so the sanitizer sees a read past it.
static void check_stage_words()
{
   const int k = 7;
   for (int stride : {1, 2, 3})
      for (int n : {0, 1, 2, 5}) {
         std::vector<int32_t> src(n ? (size_t)(1 + (n - 1) * stride) : 0, -99);   // (the gaps hold a word that would be refused)
         std::vector<int32_t> want((size_t)n), out(3, 42);
         for (int j = 0; j < n; j++) src[(size_t)(j * stride)] = want[(size_t)j] = (j * 3 + n) % k;
         CHECK(index_stage_words(src.data(), stride, n, k, out) && out == want, "stride %d, n %d: the words packed in order", stride, n);
         if (n == 0) continue;
         for (int at : {0, n - 1})
            for (int32_t bad : {-1, k, INT32_MIN, INT32_MAX}) {
               std::vector<int32_t> s2 = src;
               s2[(size_t)(at * stride)] = bad;
               CHECK(!index_stage_words(s2.data(), stride, n, k, out), "stride %d, n %d: word %d = %d is refused", stride, n, at, bad);
            }
         std::vector<int32_t> edge = src;
         edge[0] = 0;
         edge[(size_t)((n - 1) * stride)] = k - 1;
         CHECK(index_stage_words(edge.data(), stride, n, k, out) && out[0] == (n == 1 ? k - 1 : 0) && out[(size_t)n - 1] == k - 1, "stride %d, n %d: 0 and k - 1 pass", stride, n);
      }
   std::vector<int32_t> out;
   const int32_t zeros[3] = {0, 0, 0}, one[3] = {0, 1, 0};
   CHECK(index_stage_words(zeros, 1, 3, 1, out) && out == std::vector<int32_t>(3, 0), "k = 1: the word 0 alone");
   CHECK(!index_stage_words(one, 1, 3, 1, out), "k = 1: the word 1 is refused");
   CHECK(index_stage_words(nullptr, 2, 0, 1, out) && out.empty(), "n = 0 reads nothing");
}

// index_starts: the exclusive prefix sums with the total at the end; zero counts in front, inside and at the end repeat a start;
// n = 0 is the single 0; a total of exactly UINT32_MAX is what it is (the function bounds nothing: index_total_keys does, far below)
static void check_starts()
{
   const int32_t counts[8] = {0, 0, 3, 0, 4, 1, 0, 0};
   std::vector<uint32_t> s(9, 77u);
   index_starts(counts, 8, s.data());
   CHECK(s == std::vector<uint32_t>({0, 0, 0, 3, 3, 7, 8, 8, 8}), "leading, inner and trailing zeros");
   std::vector<uint32_t> one(1, 77u);
   index_starts(nullptr, 0, one.data());
   CHECK(one[0] == 0u, "n = 0: one start");
   std::vector<uint32_t> part(4, 77u);   // (a window of the counts, as a chunk of a batch takes them)
   index_starts(counts + 2, 3, part.data());
   CHECK(part == std::vector<uint32_t>({0, 3, 3, 7}), "a window starts at 0 again");
   const int32_t big[3] = {INT32_MAX, INT32_MAX, 1};   // 2 (2^31 - 1) + 1 = 2^32 - 1
   std::vector<uint32_t> b(4);
   index_starts(big, 3, b.data());
   CHECK(b[1] == (uint32_t)INT32_MAX && b[2] == 0xfffffffeu && b[3] == UINT32_MAX, "a total of 2^32 - 1 is exact");
   std::vector<int32_t> full(1024, (int32_t)1 << 18);   // the largest build: 2^28 keys
   std::vector<uint32_t> f(1025);
   index_starts(full.data(), 1024, f.data());
   CHECK(f[1024] == ((uint32_t)1 << 28) && (int64_t)f[1024] == index_total_keys(full.data(), 1024), "the largest build's total");
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

static void check_arrays(int64_t n, int64_t k, int64_t t)
{
   StagePlan p;
   const IndexArrays a = index_arrays(p, n, k);
   check_layout({{"offsets", a.offsets.off, a.offsets.bytes()}, {"df", a.df.off, a.df.bytes()}, {"idf", a.idf.off, a.idf.bytes()}, {"tfq", a.tfq.off, a.tfq.bytes()},
                 {"norm2", a.norm2.off, a.norm2.bytes()}, {"dot", a.dot.off, a.dot.bytes()}, {"score", a.score.off, a.score.bytes()},
                 {"head", a.head.off, a.head.bytes()}, {"top_scores", a.top_scores.off, a.top_scores.bytes()}, {"top_images", a.top_images.off, a.top_images.bytes()}},
                p.bytes(), "index");
   CHECK(a.offsets.count == (size_t)k + 1 && a.df.count == (size_t)k && a.idf.count == (size_t)k && a.tfq.count == (size_t)k, "per word");
   CHECK(a.norm2.count == (size_t)n && a.dot.count == (size_t)n && a.score.count == (size_t)n, "per image");
   CHECK(a.top_scores.count == 1024 && a.top_images.count == 1024 && a.head.count == 1, "the ranked result");
   StagePlan q;
   const IndexBuildArrays b = index_build_arrays(q, n, k, t);
   check_layout({{"hash_keys", b.hash_keys.off, b.hash_keys.bytes()}, {"hash_tf", b.hash_tf.off, b.hash_tf.bytes()}, {"starts", b.starts.off, b.starts.bytes()},
                 {"cursor", b.cursor.off, b.cursor.bytes()}, {"block_sums", b.block_sums.off, b.block_sums.bytes()}},
                q.bytes(), "build");
   CHECK(b.slots == index_hash_slots(t) && b.hash_keys.count == b.slots && b.hash_tf.count == b.slots && ((uint64_t)1 << b.bits) == b.slots, "one key and one count per slot");
   CHECK(b.starts.count == (size_t)n + 1 && b.cursor.count == (size_t)k && b.block_sums.count >= ((size_t)k + 4095) / 4096 + 1, "starts, cursor, the scan's block sums");
   CHECK(index_working_set_bytes(n, k, t) == p.bytes() + q.bytes() + index_lists_bytes(t), "the working set");
   CHECK(index_lists_bytes(t) == (size_t)(t > 0 ? t : 1) * 8, "8 bytes per posting");
}

int main()
{
   check_bounds();
   check_ilog2();
   check_sums();
   check_hash();
   check_stage_words();
   check_starts();
   for (int64_t n : {(int64_t)1, (int64_t)3, (int64_t)257, (int64_t)1 << 20})
      for (int64_t k : {(int64_t)1, (int64_t)33, (int64_t)4099, (int64_t)1 << 20})
         for (int64_t t : {(int64_t)0, (int64_t)1, (int64_t)513, (int64_t)1 << 28}) check_arrays(n, k, t);
   // the largest case: 6 GB of hash table, 2 GB of lists, some tens of MB of tables
   const size_t largest = index_working_set_bytes((int64_t)1 << 20, (int64_t)1 << 20, (int64_t)1 << 28);
   CHECK(largest > ((size_t)8 << 30) && largest < ((size_t)9 << 30), "%zu bytes", largest);
   if (g_failed) {
      fprintf(stderr, "%d checks failed\n", g_failed);
      return 1;
   }
   printf("index_plan_check ok\n");
   return 0;
}
