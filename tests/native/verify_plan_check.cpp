// verify_plan_check.cpp -- the host arithmetic of spatial verification (hesaff_amd/csrc/verify_plan.h) on the CPU: every bound on both
// sides, the liveness rule at its edges, the key of the best hypothesis, the layouts of the result and of the scratch, and the
// working set of the largest call.  tests/test_verify_host.py builds it with AddressSanitizer + UBSan and runs it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../hesaff_amd/csrc/verify_plan.h"

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
   const int64_t K = (int64_t)1 << 20, C = (int64_t)1 << 18, T = (int64_t)1 << 28;
   CHECK(verify_counts_ok(1, 1) && verify_counts_ok(1024, K), "the smallest and the largest call");
   CHECK(!verify_counts_ok(0, 1) && !verify_counts_ok(-1, 1) && !verify_counts_ok(1025, 1), "candidates outside 1 .. 1024");
   CHECK(!verify_counts_ok(1, 0) && !verify_counts_ok(1, -1) && !verify_counts_ok(1, K + 1), "k outside 1 .. 2^20");
   CHECK(verify_image_keys_ok(0) && verify_image_keys_ok(C) && !verify_image_keys_ok(C + 1) && !verify_image_keys_ok(-1), "keys of an image: 0 .. 2^18");
   CHECK(verify_total_ok(0) && verify_total_ok(T) && !verify_total_ok(T + 1) && !verify_total_ok(-1), "keys of all candidates: 0 .. 2^28");
   CHECK(verify_pairs_ok(1) && verify_pairs_ok(16) && !verify_pairs_ok(0) && !verify_pairs_ok(17) && !verify_pairs_ok(-1), "P in 1 .. 16");
   CHECK(verify_used_ok(0) && verify_used_ok(4096) && !verify_used_ok(4097) && !verify_used_ok(-1), "m in 0 .. 4096");
   const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
   CHECK(verify_tolerance_ok(1048576.0f) && verify_tolerance_ok(std::numeric_limits<float>::denorm_min()) && verify_tolerance_ok(0.5f), "0 < tol <= 2^20");
   CHECK(!verify_tolerance_ok(0.0f) && !verify_tolerance_ok(-1.0f) && !verify_tolerance_ok(std::nextafterf(1048576.0f, inf)) && !verify_tolerance_ok(inf) &&
            !verify_tolerance_ok(-inf) && !verify_tolerance_ok(nan),
         "tol outside, infinite or NaN");
   const int32_t ok[3] = {0, (int32_t)C, 5}, over[2] = {3, (int32_t)C + 1}, neg[2] = {-1, 4};
   CHECK(verify_total_keys(ok, 3) == C + 5 && verify_total_keys(over, 2) == -1 && verify_total_keys(neg, 2) == -1, "the sum of the counts");
   std::vector<int32_t> full(1024, (int32_t)C);   // 1024 x 2^18 = 2^28 keys: the largest call
   CHECK(verify_total_keys(full.data(), 1024) == T, "2^28 keys");
   CHECK(HS_VERIFY_MAX_WORDS == HS_INDEX_MAX_WORDS && HS_VERIFY_MAX_CANDIDATES <= HS_INDEX_MAX_IMAGES && HS_VERIFY_MAX_CANDIDATES == HS_INDEX_MAX_TOP,
         "the hash key of the index build holds (candidate, word)");
   CHECK(HS_VERIFY_MIN_AXIS == std::ldexp(1.0f, -20) && HS_VERIFY_MAX_AXIS == std::ldexp(1.0f, 20) && HS_VERIFY_MAX_A == std::ldexp(1.0f, 40) &&
            HS_VERIFY_MAX_COORD == std::ldexp(1.0f, 20) && HS_VERIFY_MAX_TOL == std::ldexp(1.0f, 20),
         "the powers of two of the definition");
}

static float ulps(float v, int n)
{
   for (int i = 0; i < std::abs(n); i++) v = std::nextafterf(v, n > 0 ? std::numeric_limits<float>::infinity() : -std::numeric_limits<float>::infinity());
   return v;
}

static bool live(float x, float y, float a, float b, float c) { return verify_frame(x, y, a, b, c).live; }

static void check_liveness()
{
   const float lo2 = std::ldexp(1.0f, -40), hi2 = std::ldexp(1.0f, 40), hi = std::ldexp(1.0f, 20), lo = std::ldexp(1.0f, -20);
   const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
   const VerifyFrame f = verify_frame(3.0f, -4.0f, 5.0f, 2.0f, 4.0f);   // r = 2, q = 1, t = 4, p = 2
   CHECK(f.live && f.x == 3.0f && f.y == -4.0f && f.p == 2.0f && f.q == 1.0f && f.r == 2.0f, "a plain frame: p %g q %g r %g", f.p, f.q, f.r);
   // p at exactly 2^-20 and 2^20; two ulps of a beyond, p has moved by one (one ulp of a is a tie that rounds back to the power of two)
   CHECK(verify_frame(0, 0, lo2, 0, 1).p == lo && live(0, 0, lo2, 0, 1), "p = 2^-20 is live");
   CHECK(verify_frame(0, 0, ulps(lo2, -2), 0, 1).p < lo && !live(0, 0, ulps(lo2, -2), 0, 1), "p below 2^-20");
   CHECK(verify_frame(0, 0, hi2, 0, 1).p == hi && live(0, 0, hi2, 0, 1), "p = 2^20 with a = 2^40 is live");
   CHECK(!live(0, 0, ulps(hi2, 1), 0, 1) && !live(0, 0, ulps(hi2, 2), 0, 1), "a above 2^40");
   // r likewise
   CHECK(verify_frame(0, 0, 1, 0, lo2).r == lo && live(0, 0, 1, 0, lo2), "r = 2^-20 is live");
   CHECK(verify_frame(0, 0, 1, 0, ulps(lo2, -2)).r < lo && !live(0, 0, 1, 0, ulps(lo2, -2)), "r below 2^-20");
   CHECK(verify_frame(0, 0, 1, 0, hi2).r == hi && live(0, 0, 1, 0, hi2), "r = 2^20 is live");
   CHECK(verify_frame(0, 0, 1, 0, ulps(hi2, 2)).r > hi && !live(0, 0, 1, 0, ulps(hi2, 2)), "r above 2^20");
   // t: the smallest positive float is positive but its root is far below 2^-20; zero and negative t; c zero, negative, infinite
   const float tiny = std::numeric_limits<float>::denorm_min();
   CHECK(verify_frame(0, 0, tiny, 0, 1).p > 0.0f && !live(0, 0, tiny, 0, 1), "t = the smallest positive float");
   CHECK(!live(0, 0, 0, 0, 1) && !live(0, 0, 1, 1, 1) && !live(0, 0, 1, 2, 1) && !live(0, 0, -1, 0, 1), "t zero or negative");
   CHECK(!live(0, 0, 1, 0, 0) && !live(0, 0, 1, 0, -1) && !live(0, 0, 1, 0, inf) && !live(0, 0, inf, 0, 1), "c zero, negative or infinite; a infinite");
   // the coordinates
   CHECK(live(hi, -hi, 1, 0, 1) && live(-hi, hi, 1, 0, 1), "|x|, |y| = 2^20 are live");
   CHECK(!live(ulps(hi, 1), 0, 1, 0, 1) && !live(-ulps(hi, 1), 0, 1, 0, 1) && !live(0, ulps(hi, 1), 1, 0, 1) && !live(0, -ulps(hi, 1), 1, 0, 1) && !live(inf, 0, 1, 0, 1),
         "coordinates beyond 2^20");
   // a NaN in each field
   CHECK(!live(nan, 0, 1, 0, 1) && !live(0, nan, 1, 0, 1) && !live(0, 0, nan, 0, 1) && !live(0, 0, 1, nan, 1) && !live(0, 0, 1, 0, nan), "a NaN in any field");
   // the range argument at its corner: the largest L11, L22 and L21 are finite
   const VerifyMap m = verify_map(hi, ulps(hi, -1), hi, lo, -ulps(hi, -1), lo);
   CHECK(m.L11 == hi2 && m.L22 == hi2 && std::isfinite(m.L21) && m.L21 > std::ldexp(1.0f, 79) && m.L21 < std::ldexp(1.0f, 81), "L21 = %g", m.L21);
   const VerifyMap id = verify_map(0.3f, 0.1f, 0.7f, 0.3f, 0.1f, 0.7f);
   CHECK(id.L11 == 1.0f && id.L21 == 0.0f && id.L22 == 1.0f, "a key against itself is the identity");
}

static void check_best_key()
{
   CHECK(verify_best_h(0) == -1 && verify_best_inliers(0) == 0, "no hypothesis");
   CHECK(verify_best_key(1, 0) > 0 && verify_best_h(verify_best_key(1, 0)) == 0 && verify_best_inliers(verify_best_key(1, 0)) == 1, "the smallest key");
   CHECK(verify_best_h(verify_best_key(4096, 4095)) == 4095 && verify_best_inliers(verify_best_key(4096, 4095)) == 4096, "the largest");
   CHECK(verify_best_key(7, 3) > verify_best_key(7, 4) && verify_best_key(8, 4095) > verify_best_key(7, 0), "more inliers first, then the lower h");
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

static void check_arrays(int64_t R, int64_t k, int64_t nq, int64_t t)
{
   StagePlan p;
   const VerifyResultArrays a = verify_result_arrays(p, R);
   check_layout({{"pairs", a.pairs.off, a.pairs.bytes()}, {"out", a.out.off, a.out.bytes()}, {"hyp", a.hyp.off, a.hyp.bytes()}, {"order", a.order.off, a.order.bytes()},
                 {"qinert", a.qinert.off, a.qinert.bytes()}},
                p.bytes(), "result");
   CHECK(a.pairs.count == (size_t)R * 8192 && a.out.count == (size_t)R * 6 && a.hyp.count == (size_t)R * 3 && a.order.count == (size_t)R && a.qinert.count == 1, "per candidate");
   StagePlan q;
   const VerifyScratchArrays s = verify_scratch_arrays(q, R, k, nq, t);
   check_layout({{"hash_keys", s.hash_keys.off, s.hash_keys.bytes()}, {"hash_tf", s.hash_tf.off, s.hash_tf.bytes()}, {"starts", s.starts.off, s.starts.bytes()},
                 {"tfq", s.tfq.off, s.tfq.bytes()}, {"offsets", s.offsets.off, s.offsets.bytes()}, {"cursor", s.cursor.off, s.cursor.bytes()},
                 {"members", s.members.off, s.members.bytes()}, {"block_sums", s.block_sums.off, s.block_sums.bytes()}, {"inert", s.inert.off, s.inert.bytes()},
                 {"found", s.found.off, s.found.bytes()}, {"used", s.used.off, s.used.bytes()}, {"best", s.best.off, s.best.bytes()}, {"corr", s.corr.off, s.corr.bytes()}},
                q.bytes(), "scratch");
   CHECK(s.slots == index_hash_slots(t) && s.slots >= 2 * (uint64_t)t && s.hash_keys.count == s.slots && s.hash_tf.count == s.slots && ((uint64_t)1 << s.bits) == s.slots,
         "one key and one count per slot, at least two slots per key");
   CHECK(s.starts.count == (size_t)R + 1 && s.tfq.count == (size_t)k && s.offsets.count == (size_t)k + 1 && s.cursor.count == (size_t)k, "per word");
   CHECK(s.members.count >= (size_t)nq && s.members.count >= 1 && s.block_sums.count >= ((size_t)k + 4095) / 4096 + 1, "the query's groups, the scan's block sums");
   CHECK(s.inert.count == (size_t)R && s.found.count == (size_t)R && s.used.count == (size_t)R && s.best.count == (size_t)R, "per candidate");
   CHECK(s.corr.count == (size_t)R * HS_VERIFY_MAX_USED * HS_VERIFY_PAIR_FLOATS && HS_VERIFY_PAIR_FLOATS == 10, "ten floats per used correspondence");
   CHECK(verify_working_set_bytes(R, k, nq, t) == p.bytes() + q.bytes(), "the working set");
}

int main()
{
   check_bounds();
   check_liveness();
   check_best_key();
   for (int64_t R : {(int64_t)1, (int64_t)3, (int64_t)1024})
      for (int64_t k : {(int64_t)1, (int64_t)33, (int64_t)4099, (int64_t)1 << 20})
         for (int64_t nq : {(int64_t)0, (int64_t)1, (int64_t)1 << 18})
            for (int64_t t : {(int64_t)0, (int64_t)1, (int64_t)513, (int64_t)1 << 28}) check_arrays(R, k, nq, t);
   // the largest call: 6 GiB of hash table, 160 MiB of correspondences, 32 MiB of pairs, some MB of tables
   const size_t largest = verify_working_set_bytes(1024, (int64_t)1 << 20, (int64_t)1 << 18, (int64_t)1 << 28);
   CHECK(largest > ((size_t)6 << 30) + ((size_t)192 << 20) && largest < ((size_t)6 << 30) + ((size_t)256 << 20), "%zu bytes", largest);
   if (g_failed) {
      fprintf(stderr, "%d checks failed\n", g_failed);
      return 1;
   }
   printf("verify_plan_check ok\n");
   return 0;
}
