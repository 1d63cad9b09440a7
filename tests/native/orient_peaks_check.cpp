// CPU check of the orientation count's peak rule (hesaff_amd/csrc/orient_peaks.h: hs_ori_peaks and hs_ori_theta, the text the device's
// k_orientation_peaks runs; built and run by tests/test_orientation_count_host.py with g++ -fsanitize=address,undefined
// -ffp-contract=off).  Constructed histograms, each with the answer written out by hand from the rule in include/hesaff_amd.h.
// Prints "orient_peaks_check ok"; a failed check prints a message and ends the program with exit code 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../hesaff_amd/csrc/orient_peaks.h"

#define CHECK(cond, ...)                                                                        \
   do {                                                                                         \
      if (!(cond)) {                                                                            \
         fprintf(stderr, "orient_peaks_check: %s:%d: %s failed: ", __FILE__, __LINE__, #cond);  \
         fprintf(stderr, __VA_ARGS__);                                                          \
         fprintf(stderr, "\n");                                                                 \
         exit(1);                                                                               \
      }                                                                                         \
   } while (0)

struct Hist {
   float h[HS_ORI_BINS];
   Hist() { for (float &v : h) v = 0.0f; }
   Hist &set(int b, float v) { h[b] = v; return *this; }
};

// hs_ori_peaks(h, K) must return exactly `want`; the entries of bins[] beyond the count are not looked at
static void expect(const char *what, const Hist &H, int K, std::vector<int> want)
{
   int bins[HS_ORI_MAX_COUNT] = {-7, -7, -7, -7};
   const int n = hs_ori_peaks(H.h, K, bins);
   CHECK(n == (int)want.size(), "%s, K = %d: n_ori %d, expected %zu", what, K, n, want.size());
   for (int j = 0; j < n; j++) CHECK(bins[j] == want[(size_t)j], "%s, K = %d: rank %d is bin %d, expected %d", what, K, j, bins[j], want[(size_t)j]);
}

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main()
{
   // all zero: flat, one orientation, bin 0, whatever K
   for (int K = 1; K <= 4; K++) expect("all zero", Hist(), K, {0});
   // one non-zero bin: its neighbours are no local maxima, everything else is below 80 %
   for (int K = 1; K <= 4; K++) expect("one bin", Hist().set(17, 3.0f), K, {17});
   // a plateau of two equal maxima: m is the lower one, and its neighbour is not strictly above m, so it is no candidate
   for (int K = 1; K <= 4; K++) expect("plateau", Hist().set(10, 5.0f).set(11, 5.0f), K, {10});
   // two candidates of equal height: the lower bin first; the maximum need not be the lowest bin
   {
      const Hist H = Hist().set(20, 10.0f).set(5, 9.0f).set(30, 9.0f);
      expect("equal candidates", H, 4, {20, 5, 30});
      expect("equal candidates", H, 3, {20, 5, 30});
      expect("equal candidates", H, 2, {20, 5});
      expect("equal candidates", H, 1, {20});
      // ... and with the equal pair on the other side of an intermediate height
      expect("equal candidates + one between", Hist().set(20, 10.0f).set(5, 9.0f).set(30, 9.0f).set(12, 9.5f), 4, {20, 12, 5, 30});
      expect("equal candidates + one between", Hist().set(20, 10.0f).set(5, 9.0f).set(30, 9.0f).set(12, 9.5f), 3, {20, 12, 5});
   }
   // the 80 % line: exactly 0.8f * h[m] (one binary32 product) is a candidate, the float below it is not, the float above it is
   {
      const float top = 7.3f, line = 0.8f * top;
      const float below = nextafterf(line, 0.0f), above = nextafterf(line, 100.0f);
      CHECK(below < line && line < above, "nextafterf");
      expect("at the line", Hist().set(3, top).set(9, line), 2, {3, 9});
      expect("below the line", Hist().set(3, top).set(9, below), 2, {3});
      expect("above the line", Hist().set(3, top).set(9, above), 2, {3, 9});
      expect("at, below and above", Hist().set(3, top).set(9, line).set(15, below).set(21, above), 4, {3, 21, 9});
   }
   // the wrap: bin 0's left neighbour is bin 35 and the other way round
   {
      expect("peaks at 0 and 35 are one slope", Hist().set(0, 6.0f).set(35, 5.5f), 4, {0});            // 35 is not above its right neighbour 0
      expect("peak at 35, candidate at 0", Hist().set(35, 6.0f).set(34, 1.0f).set(1, 5.0f).set(0, 5.5f).set(35, 6.0f), 4, {35});   // 0 is below its left neighbour 35
      expect("peak at 0 over the wrap", Hist().set(35, 2.0f).set(0, 6.0f).set(1, 2.0f).set(18, 5.0f), 4, {0, 18});
      expect("candidate at 35 over the wrap", Hist().set(34, 2.0f).set(35, 5.0f).set(0, 2.0f).set(18, 6.0f), 4, {18, 35});
      expect("candidate at 0 over the wrap", Hist().set(35, 4.9f).set(0, 5.0f).set(1, 2.0f).set(18, 6.0f), 4, {18, 0});
      expect("maximum at 35, candidate at 0's far side", Hist().set(35, 6.0f).set(2, 5.0f), 2, {35, 2});
   }
   // six peaks, all within 80 %: the four highest for K = 4, in height order; K = 1, 2, 3 take the front of that list
   {
      const Hist H = Hist().set(2, 9.0f).set(8, 9.8f).set(14, 10.0f).set(20, 8.5f).set(26, 9.5f).set(32, 8.1f);
      expect("six peaks", H, 4, {14, 8, 26, 2});
      expect("six peaks", H, 3, {14, 8, 26});
      expect("six peaks", H, 2, {14, 8});
      expect("six peaks", H, 1, {14});
      // descending and ascending runs of candidates exercise both ends of the insertion
      expect("six peaks, ascending", Hist().set(2, 8.1f).set(8, 8.5f).set(14, 9.0f).set(20, 9.5f).set(26, 9.8f).set(32, 10.0f), 4, {32, 26, 20, 14});
      expect("six peaks, descending", Hist().set(2, 10.0f).set(8, 9.8f).set(14, 9.5f).set(20, 9.0f).set(26, 8.5f).set(32, 8.1f), 4, {2, 8, 14, 20});
   }
   // a comparison with a NaN is false: a NaN bin is neither the maximum nor a candidate, and its neighbours' strict comparisons fail
   {
      const float nan = nanf("");
      expect("NaN bin", Hist().set(4, 5.0f).set(10, nan).set(20, 4.5f), 4, {4, 20});
      expect("NaN beside a candidate", Hist().set(4, 5.0f).set(19, nan).set(20, 4.5f), 4, {4});
   }
   // the angle: step 5's formula around any bin, `den == 0 -> off = 0` included
   {
      const float PI = (float)M_PI, width = (2.0f * PI) / 36.0f;
      Hist H = Hist().set(9, 4.0f).set(10, 6.0f).set(11, 2.0f).set(0, 5.0f).set(35, 1.0f).set(1, 3.0f);
      const float off10 = (0.5f * (4.0f - 2.0f)) / ((4.0f + 2.0f) - (6.0f + 6.0f));
      CHECK(bits(hs_ori_theta(H.h, 10)) == bits(((10.0f + 0.5f) + off10) * width - PI), "theta around bin 10");
      const float off0 = (0.5f * (1.0f - 3.0f)) / ((1.0f + 3.0f) - (5.0f + 5.0f));
      CHECK(bits(hs_ori_theta(H.h, 0)) == bits(((0.0f + 0.5f) + off0) * width - PI), "theta around bin 0 (left neighbour 35)");
      Hist F;
      for (float &v : F.h) v = 2.0f;   // l + r == q + q: the denominator is 0
      CHECK(bits(hs_ori_theta(F.h, 35)) == bits((35.0f + 0.5f) * width - PI), "den == 0");
   }
   printf("orient_peaks_check ok\n");
   return 0;
}
