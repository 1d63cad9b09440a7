// jpeg_plan_check.cpp -- the host arithmetic of the device JPEG stage (hesaff_amd/csrc/jpeg_plan.h) on the CPU: every bound of
// make_jpeg_geom on both sides, jdsample.c's method for every ratio at cw = 1, 2, 3, the offsets and sizes of the layouts
// tests/test_jpeg_constructed.py runs, and - over an exhaustive sweep of small layouts - that every block k_jpeg_idct writes and
// every sample index hs_jpeg_sample can form stays inside the component's plane (the index formulas of kernels_jpeg.h are restated
// below; the kernels themselves need a device).  tests/test_jpeg_constructed_host.py builds it with AddressSanitizer + UBSan and runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../hesaff_amd/csrc/jpeg_plan.h"

using hesaff_plan::make_jpeg_geom;

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

static int ceil_div(int a, int b) { return (a + b - 1) / b; }

// what hesaff_read_jpeg_coefficients reports for a W x H file with these sampling factors (tests/jpeg_build.py: layout_for)
static hesaff_jpeg_layout layout_for(int W, int H, int nc, const int *h, const int *v)
{
   hesaff_jpeg_layout L;
   memset(&L, 0, sizeof L);
   int hmax = 1, vmax = 1;
   for (int i = 0; i < nc; i++) { hmax = h[i] > hmax ? h[i] : hmax; vmax = v[i] > vmax ? v[i] : vmax; }
   L.width = W; L.height = H; L.channels = nc;
   for (int i = 0; i < nc; i++) {
      L.h[i] = h[i]; L.v[i] = v[i]; L.hx[i] = hmax / h[i]; L.vx[i] = vmax / v[i];
      L.bw[i] = ceil_div(W, 8 * hmax) * h[i]; L.bh[i] = ceil_div(H, 8 * vmax) * v[i];
      L.cw[i] = ceil_div(W * h[i], hmax); L.chgt[i] = ceil_div(H * v[i], vmax);
   }
   return L;
}

static hesaff_jpeg_layout colour_420(int W, int H)
{
   const int h[3] = {2, 1, 1}, v[3] = {2, 1, 1};
   return layout_for(W, H, 3, h, v);
}
static hesaff_jpeg_layout grey(int W, int H)
{
   const int one[1] = {1};
   return layout_for(W, H, 1, one, one);
}
static bool ok(const hesaff_jpeg_layout &L)
{
   JpegGeom g;
   return make_jpeg_geom(L, g);
}

static void check_bounds()
{
   // image size 0 / 1 / 65535 / 65536
   for (int side = 0; side < 2; side++) {
      for (int size : {0, 1, 65535, 65536}) {
         hesaff_jpeg_layout L = grey(side ? 8 : (size ? size : 1), side ? (size ? size : 1) : 8);
         (side ? L.height : L.width) = size;
         if (size == 65536) { (side ? L.bh[0] : L.bw[0]) = 8192; (side ? L.chgt[0] : L.cw[0]) = 65536; }
         CHECK(ok(L) == (size == 1 || size == 65535), "%s %d", side ? "height" : "width", size);
      }
      hesaff_jpeg_layout L = grey(8, 8);
      (side ? L.height : L.width) = -1;
      CHECK(!ok(L), "a negative size");
   }
   // channels
   for (int nc : {0, 1, 2, 3, 4}) {
      hesaff_jpeg_layout L = colour_420(16, 16);
      if (nc == 1) L = grey(16, 16);
      L.channels = nc;
      CHECK(ok(L) == (nc == 1 || nc == 3), "channels %d", nc);
   }
   // hx and vx 0 / 1 / 4 / 5, on every component: the chroma of a 4x-sub-sampled file is the accepted end
   for (int c = 0; c < 3; c++)
      for (int side = 0; side < 2; side++)
         for (int r : {0, 1, 4, 5}) {
            hesaff_jpeg_layout L = colour_420(16, 16);
            for (int i = 0; i < 3; i++) { L.hx[i] = L.vx[i] = 1; L.cw[i] = L.chgt[i] = 16; L.bw[i] = L.bh[i] = 2; }   // 4:4:4 16 x 16 ...
            (side ? L.vx[c] : L.hx[c]) = r;                                                                          // ... with one ratio set
            CHECK(ok(L) == (r == 1 || r == 4), "component %d %s %d", c, side ? "vx" : "hx", r);
         }
   // bw and bh 0 / 1 / 8192 / 8193
   for (int side = 0; side < 2; side++)
      for (int b : {0, 1, 8192, 8193}) {
         hesaff_jpeg_layout L = grey(8, 8);
         (side ? L.bh[0] : L.bw[0]) = b;
         CHECK(ok(L) == (b == 1 || b == 8192), "%s %d", side ? "bh" : "bw", b);
      }
   // cw == bw * 8 against + 1, cw 0; the same for chgt
   for (int side = 0; side < 2; side++) {
      hesaff_jpeg_layout L = grey(16, 16);
      (side ? L.chgt[0] : L.cw[0]) = 16;
      CHECK(ok(L), "cw == bw * 8");
      (side ? L.chgt[0] : L.cw[0]) = 17;
      CHECK(!ok(L), "cw == bw * 8 + 1");
      (side ? L.chgt[0] : L.cw[0]) = 0;
      (side ? L.height : L.width) = 1;
      CHECK(!ok(L), "cw == 0");
   }
   // cw * hx == W against W + 1 (a component that does not cover the image), per component and direction
   for (int c = 0; c < 3; c++)
      for (int side = 0; side < 2; side++) {
         hesaff_jpeg_layout L = colour_420(16, 16);   // cw = 16, 8, 8 with hx = 1, 2, 2
         CHECK(ok(L), "cw * hx == W");
         (side ? L.height : L.width) = 17;
         for (int i = 0; i < 3; i++)
            if (i != c) { (side ? L.chgt[i] : L.cw[i]) = 17; (side ? L.bh[i] : L.bw[i]) = 3; (side ? L.vx[i] : L.hx[i]) = 1; }
         CHECK(!ok(L), "component %d: cw * hx == W - 1", c);
      }
   // a grey layout has no ratio
   for (int side = 0; side < 2; side++) {
      hesaff_jpeg_layout L = grey(8, 8);
      (side ? L.vx[0] : L.hx[0]) = 2;
      CHECK(!ok(L), "grey with a ratio of 2");
   }
   // the largest layout: sums stay inside their types
   {
      const int h[3] = {1, 1, 1};
      hesaff_jpeg_layout L = layout_for(65535, 65535, 3, h, h);
      JpegGeom g;
      CHECK(make_jpeg_geom(L, g), "65535 x 65535 4:4:4");
      CHECK(g.blocks_per_image == 3u * 8192u * 8192u && g.plane_bytes == 3ull * 65536 * 65536 && g.blob_bytes == 1024 + 6ull * 65536 * 65536, "its sizes");
   }
}

static void check_methods()
{
   for (int hx = 1; hx <= 4; hx++)
      for (int vx = 1; vx <= 4; vx++)
         for (int cw = 1; cw <= 3; cw++) {
            const int W = cw * hx, H = 3 * vx;
            const int h[3] = {hx, 1, 1}, v[3] = {vx, 1, 1};
            hesaff_jpeg_layout L = layout_for(W, H, 3, h, v);
            JpegGeom g;
            CHECK(make_jpeg_geom(L, g) && L.cw[1] == cw && L.hx[1] == hx && L.vx[1] == vx, "%d x %d at cw %d", hx, vx, cw);
            // jdsample.c, jinit_upsampler with fancy up-sampling: the triangle filters of h2v1 and h2v2 need more than two columns; h1v2
            // has no such condition; every other integral ratio is replicated
            int want = JPEG_UP_REPLICATE;
            if (hx == 1 && vx == 1) want = JPEG_UP_NONE;
            else if (hx == 2 && vx == 1 && cw >= 3) want = JPEG_UP_H2V1;
            else if (hx == 2 && vx == 2 && cw >= 3) want = JPEG_UP_H2V2;
            else if (hx == 1 && vx == 2) want = JPEG_UP_H1V2;
            CHECK(g.mode[0] == JPEG_UP_NONE && g.mode[1] == want && g.mode[2] == want, "%d x %d at cw %d: mode %d, not %d", hx, vx, cw, g.mode[1], want);
         }
}

// the layouts of the block-addressing table of tests/test_jpeg_constructed.py (tests/test_jpeg_constructed_host.py reads this list)
struct TableLayout { int W, H, nc; int h[3], v[3]; unsigned blocks; };
static const TableLayout kTable[] = {
   {8, 8, 1, {1}, {1}, 1},
   {1, 1, 1, {1}, {1}, 1},
   {5, 3, 1, {1}, {1}, 1},
   {8, 8, 3, {1, 1, 1}, {1, 1, 1}, 3},
   {16, 16, 3, {2, 1, 1}, {2, 1, 1}, 6},
   {40, 40, 3, {2, 1, 1}, {2, 1, 1}, 54},
   {56, 72, 1, {1}, {1}, 63},
   {64, 64, 1, {1}, {1}, 64},
   {40, 104, 1, {1}, {1}, 65},
};

static void check_offsets()
{
   for (const TableLayout &t : kTable) {
      const hesaff_jpeg_layout L = layout_for(t.W, t.H, t.nc, t.h, t.v);
      JpegGeom g;
      CHECK(make_jpeg_geom(L, g), "%d x %d", t.W, t.H);
      CHECK(g.blocks_per_image == t.blocks, "%d x %d: %u blocks, not %u", t.W, t.H, g.blocks_per_image, t.blocks);
      unsigned long long coef = HESAFF_JPEG_BLOB_HEADER, plane = 0;
      unsigned blocks = 0;
      for (int c = 0; c < t.nc; c++) {
         CHECK(g.coef_off[c] == coef && g.plane_off[c] == plane && g.blocks[c] == (unsigned)(L.bw[c] * L.bh[c]), "%d x %d component %d", t.W, t.H, c);
         coef += 128ull * g.blocks[c]; plane += 64ull * g.blocks[c]; blocks += g.blocks[c];
      }
      CHECK(g.blob_bytes == coef && g.plane_bytes == plane && blocks == t.blocks && g.blob_bytes == 1024 + 128ull * t.blocks, "%d x %d sizes", t.W, t.H);
      CHECK(g.W == t.W && g.H == t.H && g.nc == t.nc, "%d x %d", t.W, t.H);
   }
   // 4:2:0 40 x 40: 3 x 3 MCUs, the luma's 36 blocks in front of 9 + 9
   const hesaff_jpeg_layout L = layout_for(40, 40, 3, kTable[5].h, kTable[5].v);
   JpegGeom g;
   CHECK(make_jpeg_geom(L, g) && g.blocks[0] == 36 && g.blocks[1] == 9 && g.coef_off[1] == 1024 + 36 * 128 && g.plane_off[2] == 45 * 64 && g.cw[1] == 20 && g.bw[1] == 3,
         "4:2:0 40 x 40");
}

// ---- every index the kernels form from an accepted layout ----
// A component's plane: bw * 8 columns (the row stride) x bh * 8 rows.  `touch` notes a read of sample (x, y) and checks it.
struct Plane {
   int stride, rows, w, h;
   long long reads = 0;
   bool bad = false;
   void touch(long long y, long long x)
   {
      reads++;
      // inside the plane for memory safety, and inside the w x h samples the component has: a read of block padding would be a wrong pixel
      if (x < 0 || y < 0 || x >= w || y >= h || x >= stride || y >= rows) bad = true;
   }
};

// hs_jpeg_sample's indices (kernels_jpeg.h), restated
static void sample_reads(Plane &p, int mode, int hx, int vx, int ox, int oy)
{
   const int w = p.w, h = p.h;
   if (mode == JPEG_UP_NONE) { p.touch(oy, ox); return; }
   if (mode == JPEG_UP_H2V1) {
      const int x = ox >> 1;
      if (ox == 0) { p.touch(oy, 0); return; }
      if (ox == 2 * w - 1) { p.touch(oy, w - 1); return; }
      p.touch(oy, x);
      p.touch(oy, (ox & 1) ? x + 1 : x - 1);
      return;
   }
   if (mode == JPEG_UP_H2V2) {
      const int y = oy >> 1;
      int yf = (oy & 1) ? y + 1 : y - 1;
      yf = yf < 0 ? 0 : (yf > h - 1 ? h - 1 : yf);
      const int y0 = y > h - 1 ? h - 1 : y;
      const int x = ox >> 1;
      p.touch(y0, x); p.touch(yf, x);
      if (ox == 0 || ox == 2 * w - 1) return;
      const int xn = (ox & 1) ? x + 1 : x - 1;
      p.touch(y0, xn); p.touch(yf, xn);
      return;
   }
   if (mode == JPEG_UP_H1V2) {
      const int y = (oy >> 1) > h - 1 ? h - 1 : (oy >> 1);
      int yf = (oy & 1) ? y + 1 : y - 1;
      yf = yf < 0 ? 0 : (yf > h - 1 ? h - 1 : yf);
      p.touch(y, ox); p.touch(yf, ox);
      return;
   }
   const int y = (oy / vx) > h - 1 ? h - 1 : (oy / vx), x = (ox / hx) > w - 1 ? w - 1 : (ox / hx);
   p.touch(y, x);
}

static void check_indices()
{
   long long layouts = 0, reads = 0;
   for (int W = 1; W <= 20; W++)
      for (int H = 1; H <= 20; H++)
         for (int code = 0; code < 4096; code++) {   // all factor triples (h, v) in 1 .. 4 whose ratios to the largest are integral
            int h[3], v[3], hmax = 1, vmax = 1;
            for (int i = 0, c = code; i < 3; i++, c >>= 4) { h[i] = 1 + (c & 3); v[i] = 1 + ((c >> 2) & 3); hmax = h[i] > hmax ? h[i] : hmax; vmax = v[i] > vmax ? v[i] : vmax; }
            bool integral = true;
            for (int i = 0; i < 3; i++) integral = integral && hmax % h[i] == 0 && vmax % v[i] == 0;
            if (!integral) continue;
            const hesaff_jpeg_layout L = layout_for(W, H, 3, h, v);
            JpegGeom g;
            if (!make_jpeg_geom(L, g)) { CHECK(false, "%d x %d code %d: a layout the reader reports is refused", W, H, code); continue; }
            layouts++;
            for (int c = 0; c < 3; c++) {
               // k_jpeg_idct: block k of the component goes to rows by * 8 .. + 7, columns bx * 8 .. + 7 of a plane of blocks[c] * 64 bytes
               const unsigned last = g.blocks[c] - 1;
               const unsigned long long end = (unsigned long long)(last / g.bw[c]) * 8 * (g.bw[c] * 8) + (last % g.bw[c]) * 8 + 7ull * (g.bw[c] * 8) + 8;
               CHECK(end == 64ull * g.blocks[c] && g.plane_off[c] + end <= g.plane_bytes, "%d x %d code %d component %d: the last block ends at %llu", W, H, code, c, end);
               Plane p{g.bw[c] * 8, g.bh[c] * 8, g.cw[c], g.chgt[c]};
               for (int oy = 0; oy < g.H; oy++)
                  for (int ox = 0; ox < g.W; ox++) sample_reads(p, g.mode[c], g.hx[c], g.vx[c], ox, oy);
               CHECK(!p.bad, "%d x %d code %d component %d (mode %d, %d x %d samples): a read outside the component", W, H, code, c, g.mode[c], g.cw[c], g.chgt[c]);
               reads += p.reads;
            }
         }
   // grey: the copy reads (x, y) of a plane bw * 8 wide
   for (int W = 1; W <= 20; W++)
      for (int H = 1; H <= 20; H++) {
         JpegGeom g;
         CHECK(make_jpeg_geom(grey(W, H), g) && g.bw[0] * 8 >= W && g.bh[0] * 8 >= H && g.plane_bytes == 64ull * g.bw[0] * g.bh[0], "grey %d x %d", W, H);
      }
   CHECK(layouts > 100000, "%lld layouts", layouts);
   printf("index sweep: %lld layouts, %lld sample reads inside their components\n", layouts, reads);
}

int main()
{
   check_bounds();
   check_methods();
   check_offsets();
   check_indices();
   if (g_failed) { fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
   puts("jpeg_plan_check ok");
   return 0;
}
