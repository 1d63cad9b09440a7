// The out-of-line part of the OpenCV stand-in (cv.h): SVD, GaussianBlur, imread.
#include "cv.h"

#include <cstdio>

namespace cv {

// cv::SVD of a 2x2 float matrix, as the closed-form symmetric eigen-decomposition of A A^T in
// double; u and w are then stored as float, which is what the members of cv::SVD hold.  The
// reference uses only u * diag(f(w)) * u^T, which does not depend on the signs of u's columns.
SVD::SVD(const Mat &A, int)
{
   assert(A.rows == 2 && A.cols == 2 && A.type() == CV_32FC1);
   const double a11 = A.at<float>(0, 0), a12 = A.at<float>(0, 1), a21 = A.at<float>(1, 0), a22 = A.at<float>(1, 1);
   const double m00 = a11 * a11 + a12 * a12, m01 = a11 * a21 + a12 * a22, m11 = a21 * a21 + a22 * a22;
   const double tr = m00 + m11, df = m00 - m11;
   const double disc = std::sqrt(df * df + 4.0 * m01 * m01);
   const double l1 = (tr + disc) / 2.0, l2 = (tr - disc) / 2.0;
   // the eigenvector of l1 is (l1 - m11, m01) and also (m01, l1 - m00): take the longer one
   double vx = l1 - m11, vy = m01;
   const double wx = m01, wy = l1 - m00;
   if (wx * wx + wy * wy > vx * vx + vy * vy) { vx = wx; vy = wy; }
   const double n = std::sqrt(vx * vx + vy * vy);
   float c = 1.0f, s = 0.0f;
   if (n > 0) { c = (float)(vx / n); s = (float)(vy / n); }
   u = Mat(2, 2, CV_32FC1);
   u.at<float>(0, 0) = c; u.at<float>(0, 1) = -s;
   u.at<float>(1, 0) = s; u.at<float>(1, 1) = c;
   w = Mat(2, 1, CV_32FC1);
   w.at<float>(0, 0) = (float)std::sqrt(l1);
   w.at<float>(1, 0) = (float)std::sqrt(l2);
}

static inline int clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// the separable float filter of OpenCV 2.4's scalar path.
void GaussianBlur(const Mat &src, Mat &dst, Size ksize, double sigmaX, double, int borderType)
{
   assert(src.type() == CV_32FC1 && ksize.width == ksize.height && (ksize.width & 1) && borderType == BORDER_REPLICATE);
   (void)borderType;
   const int K = ksize.width, r = K / 2, rows = src.rows, cols = src.cols;

   // getGaussianKernel(K, sigma, CV_32F)
   std::vector<float> k(K);
   const double scale2X = -0.5 / (sigmaX * sigmaX);
   double sum = 0;
   for (int i = 0; i < K; i++) {
      const double x = i - (K - 1) * 0.5;
      k[i] = (float)std::exp(scale2X * x * x);
      sum += k[i];
   }
   sum = 1. / sum;
   for (int i = 0; i < K; i++) k[i] = (float)(k[i] * sum);

   // row pass into a buffer of its own, so an in-place call reads nothing it has written
   Mat tmp(rows, cols, CV_32FC1);
   for (int y = 0; y < rows; y++) {
      const float *S = src.ptr<float>(y);
      float *T = tmp.ptr<float>(y);
      for (int x = 0; x < cols; x++) {
         float t;
         if (K <= 5) {   // SymmRowSmallFilter
            t = S[x] * k[r];
            for (int j = 1; j <= r; j++) t += (S[clampi(x - j, cols - 1)] + S[clampi(x + j, cols - 1)]) * k[r + j];
         } else {        // RowFilter: ascending, sequential
            t = k[0] * S[clampi(x - r, cols - 1)];
            for (int j = 1; j < K; j++) t += k[j] * S[clampi(x - r + j, cols - 1)];
         }
         T[x] = t;
      }
   }

   if (!dst.data || dst.rows != rows || dst.cols != cols || dst.type() != CV_32FC1) dst = Mat(rows, cols, CV_32FC1);
   // SymmColumnFilter; reads tmp only, so dst may be src
   for (int y = 0; y < rows; y++) {
      float *D = dst.ptr<float>(y);
      for (int x = 0; x < cols; x++) {
         float d = k[r] * tmp.at<float>(y, x);
         for (int j = 1; j <= r; j++) d += k[r + j] * (tmp.at<float>(clampi(y + j, rows - 1), x) + tmp.at<float>(clampi(y - j, rows - 1), x));
         D[x] = d;
      }
   }
}

Mat imread(const std::string &path)
{
   FILE *f = std::fopen(path.c_str(), "rb");
   if (!f) return Mat();
   char magic[3] = {0, 0, 0};
   int hdr[3], got = 0;
   if (std::fscanf(f, "%2s", magic) == 1 && magic[0] == 'P' && (magic[1] == '5' || magic[1] == '6')) {
      while (got < 3) {
         int ch = std::fgetc(f);
         if (ch == '#') { while (ch != '\n' && ch != EOF) ch = std::fgetc(f); continue; }
         if (ch == EOF) break;
         if (ch == ' ' || ch == '\t' || ch == '\n' || ch == '\r') continue;
         std::ungetc(ch, f);
         if (std::fscanf(f, "%d", &hdr[got]) != 1) break;
         got++;
      }
   }
   if (got != 3 || hdr[0] <= 0 || hdr[1] <= 0 || hdr[2] != 255) { std::fclose(f); return Mat(); }
   std::fgetc(f);   // the single whitespace byte after maxval
   const int w = hdr[0], h = hdr[1], ch = magic[1] == '6' ? 3 : 1;
   std::vector<uchar> raw((size_t)w * h * ch);
   const bool ok = std::fread(raw.data(), 1, raw.size(), f) == raw.size();
   std::fclose(f);
   if (!ok) return Mat();
   Mat m(h, w, CV_8UC3);
   for (size_t i = 0; i < (size_t)w * h; i++)
      for (int c = 0; c < 3; c++) m.data[i * 3 + c] = ch == 3 ? raw[i * 3 + 2 - c] : raw[i];
   return m;
}

} // namespace cv
