// Stand-in for the part of OpenCV 2.4's <cv.h> that the reference sources use (SURVEY.md
// Appendix B).  Test infrastructure: it lets `make -C oracle ref` compile the reference
// unmodified into oracle/_ref/.  Nothing under hesaff_amd/ includes it.
//
// -DSHIM_POISON fills every freshly allocated Mat buffer with 0xFF bytes (a NaN as float),
// so that a read of memory the reference never wrote changes the output.
#ifndef HESAFF_CVSHIM_CV_H
#define HESAFF_CVSHIM_CV_H

#include <cassert>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

// affine.h and siftdesc.h name these outside namespace cv, so they are macros as in OpenCV
#define CV_8UC1 0
#define CV_32FC1 5
#define CV_8UC3 16

namespace cv {

typedef unsigned char uchar;

enum { BORDER_REPLICATE = 1 };

struct Scalar {
   double val[4];
   Scalar(double v0 = 0, double v1 = 0, double v2 = 0, double v3 = 0) { val[0] = v0; val[1] = v1; val[2] = v2; val[3] = v3; }
};

struct Size {
   int width, height;
   Size(int w = 0, int h = 0) : width(w), height(h) {}
};

class Mat {
 public:
   int rows, cols;
   uchar *data;
   size_t step;   // bytes per row

   Mat() : rows(0), cols(0), data(0), step(0), type_(CV_8UC1) {}
   Mat(int r, int c, int type) { create(r, c, type); }
   Mat(int r, int c, int type, const Scalar &s) { create(r, c, type); *this = s; }
   // a view of memory the caller owns
   Mat(int r, int c, int type, void *p) : rows(r), cols(c), data((uchar *)p), step((size_t)c * elemSize(type)), type_(type) {}
   // copies are shallow and share the ref-counted buffer (the compiler-generated ones do that)

   static size_t elemSize(int type) { return type == CV_32FC1 ? 4 : type == CV_8UC3 ? 3 : 1; }
   int type() const { return type_; }

   void create(int r, int c, int type)
   {
      rows = r; cols = c; type_ = type;
      step = (size_t)c * elemSize(type);
      const size_t bytes = step * (size_t)r;
      buf_.reset((uchar *)std::malloc(bytes ? bytes : 1), std::free);
      data = buf_.get();
#ifdef SHIM_POISON
      std::memset(data, 0xFF, bytes);
#endif
   }

   Mat &operator=(const Scalar &s)
   {
      for (int r = 0; r < rows; r++) {
         if (type_ == CV_32FC1) {
            float *p = ptr<float>(r);
            for (int c = 0; c < cols; c++) p[c] = (float)s.val[0];
         } else {
            uchar *p = ptr<uchar>(r);
            const int ch = (int)elemSize(type_);
            for (int c = 0; c < cols * ch; c++) p[c] = (uchar)s.val[c % ch];
         }
      }
      return *this;
   }

   template <class T> T *ptr(int r = 0) { return (T *)(data + step * (size_t)r); }
   template <class T> const T *ptr(int r = 0) const { return (const T *)(data + step * (size_t)r); }
   template <class T> T &at(int r, int c) { return ptr<T>(r)[c]; }
   template <class T> const T &at(int r, int c) const { return ptr<T>(r)[c]; }

   Mat clone() const
   {
      Mat m(rows, cols, type_);
      for (int r = 0; r < rows; r++) std::memcpy(m.ptr<uchar>(r), ptr<uchar>(r), m.step);
      return m;
   }

   static Mat zeros(int r, int c, int type)
   {
      Mat m(r, c, type);
      std::memset(m.data, 0, m.step * (size_t)r);
      return m;
   }

   // float only from here on, which is all the reference asks for
   static Mat diag(const Mat &w)
   {
      const int n = w.rows * w.cols;
      Mat m = zeros(n, n, CV_32FC1);
      for (int i = 0; i < n; i++) m.at<float>(i, i) = ((const float *)w.data)[i];
      return m;
   }

   Mat t() const
   {
      Mat m(cols, rows, CV_32FC1);
      for (int r = 0; r < rows; r++)
         for (int c = 0; c < cols; c++) m.at<float>(c, r) = at<float>(r, c);
      return m;
   }

 private:
   int type_;
   std::shared_ptr<uchar> buf_;
};

// cv::gemm accumulates CV_32F products in double and stores float
inline Mat operator*(const Mat &a, const Mat &b)
{
   assert(a.cols == b.rows);
   Mat m(a.rows, b.cols, CV_32FC1);
   for (int i = 0; i < a.rows; i++)
      for (int j = 0; j < b.cols; j++) {
         double acc = 0;
         for (int k = 0; k < a.cols; k++) acc += (double)a.at<float>(i, k) * (double)b.at<float>(k, j);
         m.at<float>(i, j) = (float)acc;
      }
   return m;
}

// Mat_<float>(2,2) << a, b, c, d
template <class T> class Mat_ : public Mat {
 public:
   Mat_(int r, int c) : Mat(r, c, CV_32FC1) {}
};

template <class T> class MatCommaInitializer_ {
 public:
   MatCommaInitializer_(const Mat &m, T first) : m_(m), n_(0) { put(first); }
   MatCommaInitializer_ &operator,(T v) { put(v); return *this; }
   operator Mat() const { return m_; }

 private:
   void put(T v) { assert(n_ < m_.rows * m_.cols); ((T *)m_.data)[n_++] = v; }
   Mat m_;
   int n_;
};

template <class T> MatCommaInitializer_<T> operator<<(const Mat_<T> &m, T first) { return MatCommaInitializer_<T>(m, first); }

// 2x2 float only; u (2x2) and w (2x1) as cv::SVD names them
class SVD {
 public:
   enum { FULL_UV = 4 };
   Mat u, w;
   SVD(const Mat &A, int flags = 0);
};

void GaussianBlur(const Mat &src, Mat &dst, Size ksize, double sigmaX, double sigmaY, int borderType);

// binary PGM (P5) and PPM (P6), 8 bit; returns CV_8UC3 in B,G,R order like cv::imread
Mat imread(const std::string &path);

} // namespace cv

#endif
