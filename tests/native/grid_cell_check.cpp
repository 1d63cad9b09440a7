// grid_cell_check.cpp -- the grid selection's cell arithmetic (hesaff_amd/csrc/select_grid.h, the lines the device runs) on the host,
// under AddressSanitizer + UBSan (tests/test_keypoint_grid.py builds and runs it): for every axis length W in 1..300 and W = 65535,
// every cell count C in 1..64 and every pixel col of the axis, the cell c = hs_grid_cell_1d(col, C, W) satisfies
//    c * W / C <= col < (c + 1) * W / C      (integer division: the cell ranges of OpenCV's GridAdaptedFeatureDetector),
// c never decreases along the axis and ends at C - 1 (with more cells than pixels the first cells are empty), and the function's largest intermediate, (col + 1) * C, computed
// here in 64 bits, stays inside int32 (UBSan would also stop at a signed overflow inside the function).  Also hs_sel_pixel on a few
// values, and the row-major cell index.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../hesaff_amd/csrc/select_grid.h"

static long long g_checked = 0;

static bool check_axis(int W)
{
   for (int C = 1; C <= HS_GRID_MAX_CELLS; C++) {
      int prev = 0;
      for (int col = 0; col < W; col++) {
         const long long widest = ((long long)col + 1) * C;
         if (widest > INT32_MAX) { fprintf(stderr, "W=%d C=%d col=%d: (col + 1) * C leaves int32\n", W, C, col); return false; }
         const int c = hs_grid_cell_1d(col, C, W);
         const long long lo = (long long)c * W / C, hi = ((long long)c + 1) * W / C;
         if (c < 0 || c >= C || !(lo <= col && col < hi)) { fprintf(stderr, "W=%d C=%d col=%d: cell %d, range [%lld, %lld)\n", W, C, col, c, lo, hi); return false; }
         if (c < prev) { fprintf(stderr, "W=%d C=%d col=%d: cell %d after %d\n", W, C, col, c, prev); return false; }
         prev = c;
         g_checked++;
      }
      if (prev != C - 1) { fprintf(stderr, "W=%d C=%d: the last pixel lies in cell %d\n", W, C, prev); return false; }
   }
   return true;
}

int main()
{
   for (int W = 1; W <= 300; W++)
      if (!check_axis(W)) return 1;
   if (!check_axis(65535)) return 1;
   // the closed form is not col * C / W: 77 rows in 4 cells
   int differ = 0;
   for (int row = 0; row < 77; row++) differ += hs_grid_cell_1d(row, 4, 77) != row * 4 / 77;
   if (differ == 0) { fprintf(stderr, "77 / 4: the range rule equals row * R / H everywhere\n"); return 1; }
   // pixels: round half up in binary32, truncate, clamp
   const float half_below = 9.49999905f;   // the float below 9.5
   if (hs_sel_pixel(9.5f, 12) != 10 || hs_sel_pixel(half_below, 12) != 9 || hs_sel_pixel(11.6f, 12) != 11 || hs_sel_pixel(112.0f, 12) != 11 ||
       hs_sel_pixel(-3.0f, 12) != 0 || hs_sel_pixel(-0.6f, 12) != 0 || hs_sel_pixel(0.49f, 12) != 0) { fprintf(stderr, "hs_sel_pixel\n"); return 1; }
   // rows of cells outermost: a 2 x 3 grid over 12 x 10 (W x H)
   std::vector<int> cells;
   for (int row : {0, 4, 5, 9}) for (int col : {0, 3, 4, 7, 8, 11}) cells.push_back(hs_grid_cell(row, col, 2, 3, 12, 10));
   const std::vector<int> want = {0, 0, 1, 1, 2, 2, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 3, 3, 4, 4, 5, 5};
   if (cells != want) { fprintf(stderr, "hs_grid_cell: rows and columns\n"); return 1; }
   printf("checked=%lld differ_77_4=%d ok\n", g_checked, differ);
   return 0;
}
