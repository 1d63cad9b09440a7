// ref_driver: the reference's own classes behind a command line that the tests can steer.
// Test infrastructure; `make -C oracle ref` links it with the unmodified reference sources
// and the OpenCV stand-in (cvshim/) into oracle/_ref/.  It holds no reference code: it calls
// the public members of HessianDetector, AffineShape and SIFTDescriptor and writes down what
// they return.
//
//   ref_driver IMAGE.f32 ROWS COLS OUT.rec [planes=FILE] [points=FILE | shapes=FILE] [key=value ...]
//
// IMAGE.f32 is a raw little-endian float32 grey plane (the CV_32FC1 detector input).
// Parameters: threshold edgeEigenValueRatio initialSigma maxIterations convergenceThreshold
// mrSize maxBinValue.  initialSigma sets PyramidParams::initialSigma only;
// affineInitialSigma sets AffineShapeParams::initialSigma (the library never changes it, the
// key exists so that a test can show the two readings differ).
//
// OUT.rec: one Record per Hessian keypoint, in callback order.
// planes=FILE: every distinct blur plane handed to onHessianKeypointDetected, once, in order
//    of first appearance: int32 rows, int32 cols, float pixelDistance, rows*cols floats.
// points=FILE: records {int32 plane, float x, y, s}.  The detector runs first (keypoints only)
//    to capture the planes; then findAffineShape -> rectify -> normalizeAffine -> SIFT run on
//    each point with the plane of that index.  OUT.rec holds one Record per point.
// shapes=FILE: records {float x, y, s, u11, u12, u21, u22}: rectify -> normalizeAffine -> SIFT
//    on the image.  OUT.rec holds one Record per shape.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pyramid.h"
#include "helpers.h"
#include "affine.h"
#include "siftdesc.h"

enum { NOT_CONVERGED = 0, REJECTED = 1, DESCRIBED = 2 };

struct Record {
   float x, y, s, pixelDistance, response;
   int32_t type, fate, iters, plane;
   float U[4];   // findAffineShape's matrix, before rectification (fate >= 1)
   float A[4];   // rectified (fate == 2)
   unsigned char desc[128];
};
static_assert(sizeof(Record) == 196, "Record is read back with a fixed numpy dtype");

struct Driver : HessianDetector, AffineShape, HessianKeypointCallback, AffineShapeCallback {
   const Mat image;
   SIFTDescriptor sift;
   std::vector<Record> records;
   std::vector<Mat> planes;            // shallow copies: they keep every buffer alive, so a data pointer names one plane
   std::vector<float> planeDistance;
   bool keypointsOnly;

   Driver(const Mat &img, const PyramidParams &pp, const AffineShapeParams &ap, const SIFTDescriptorParams &sp)
      : HessianDetector(pp), AffineShape(ap), image(img), sift(sp), keypointsOnly(false)
   {
      setHessianKeypointCallback(this);
      setAffineShapeCallback(this);
   }

   int planeIndex(const Mat &blur, float pixelDistance)
   {
      for (size_t i = planes.size(); i-- > 0;)
         if (planes[i].data == blur.data) return (int)i;
      planes.push_back(blur);
      planeDistance.push_back(pixelDistance);
      return (int)planes.size() - 1;
   }

   Record &open(float x, float y, float s, float pixelDistance, int type, float response, int plane)
   {
      Record r;
      memset(&r, 0, sizeof r);
      r.x = x; r.y = y; r.s = s; r.pixelDistance = pixelDistance; r.response = response;
      r.type = type; r.fate = NOT_CONVERGED; r.plane = plane;   // iters, U, A, desc stay 0 until a stage fills them
      records.push_back(r);
      return records.back();
   }

   void onHessianKeypointDetected(const Mat &blur, float x, float y, float s, float pixelDistance, int type, float response)
   {
      open(x, y, s, pixelDistance, type, response, planeIndex(blur, pixelDistance));
      if (!keypointsOnly) findAffineShape(blur, x, y, s, pixelDistance, type, response);
   }

   // findAffineShape calls this only when it converged; the record is the one opened last
   void onAffineShapeFound(const Mat &, float x, float y, float s, float, float a11, float a12, float a21, float a22, int, float, int iters)
   {
      Record &r = records.back();
      r.iters = iters;
      describe(r, x, y, s, a11, a12, a21, a22);
   }

   void describe(Record &r, float x, float y, float s, float a11, float a12, float a21, float a22)
   {
      r.U[0] = a11; r.U[1] = a12; r.U[2] = a21; r.U[3] = a22;
      r.fate = REJECTED;
      rectifyAffineTransformationUpIsUp(a11, a12, a21, a22);
      if (normalizeAffine(image, x, y, s, a11, a12, a21, a22)) return;
      sift.computeSiftDescriptor(patch);
      r.A[0] = a11; r.A[1] = a12; r.A[2] = a21; r.A[3] = a22;
      for (int i = 0; i < 128; i++) r.desc[i] = (unsigned char)sift.vec[i];
      r.fate = DESCRIBED;
   }
};

template <class T> static bool readAll(const std::string &path, std::vector<T> &out)
{
   FILE *f = fopen(path.c_str(), "rb");
   if (!f) return false;
   fseek(f, 0, SEEK_END);
   const long bytes = ftell(f);
   fseek(f, 0, SEEK_SET);
   out.resize(bytes / sizeof(T));
   const bool ok = bytes % (long)sizeof(T) == 0 && fread(out.data(), sizeof(T), out.size(), f) == out.size();
   fclose(f);
   return ok;
}

static int fail(const std::string &msg)
{
   fprintf(stderr, "ref_driver: %s\n", msg.c_str());
   return 2;
}

struct PointIn { int32_t plane; float x, y, s; };
struct ShapeIn { float x, y, s, u[4]; };

int main(int argc, char **argv)
{
   if (argc < 5) return fail("usage: ref_driver IMAGE.f32 ROWS COLS OUT.rec [planes=FILE] [points=FILE | shapes=FILE] [key=value ...]");
   const int rows = atoi(argv[2]), cols = atoi(argv[3]);
   if (rows <= 0 || cols <= 0) return fail("bad image size");

   PyramidParams pp;
   AffineShapeParams ap;
   SIFTDescriptorParams sp;
   std::string planesPath, pointsPath, shapesPath;
   for (int i = 5; i < argc; i++) {
      const char *eq = strchr(argv[i], '=');
      if (!eq) return fail(std::string("not key=value: ") + argv[i]);
      const std::string key(argv[i], eq - argv[i]), value(eq + 1);
      const float v = strtof(value.c_str(), 0);
      if (key == "threshold") pp.threshold = v;
      else if (key == "edgeEigenValueRatio") pp.edgeEigenValueRatio = v;
      else if (key == "initialSigma") pp.initialSigma = v;
      else if (key == "affineInitialSigma") ap.initialSigma = v;
      else if (key == "maxIterations") ap.maxIterations = atoi(value.c_str());
      else if (key == "convergenceThreshold") ap.convergenceThreshold = v;
      else if (key == "mrSize") ap.mrSize = v;
      else if (key == "maxBinValue") sp.maxBinValue = v;
      else if (key == "planes") planesPath = value;
      else if (key == "points") pointsPath = value;
      else if (key == "shapes") shapesPath = value;
      else if (key == "upscaleInputImage")
         return fail("upscaleInputImage is refused: the reference's doubleImage indexes float rows with the byte step and reads "
                     "outside its input buffer, so its output there is not defined");
      else return fail("unknown parameter: " + key);
   }
   if (!pointsPath.empty() && !shapesPath.empty()) return fail("points= and shapes= exclude each other");

   Mat image(rows, cols, CV_32FC1);
   {
      std::vector<float> pix;
      if (!readAll(argv[1], pix) || pix.size() != (size_t)rows * cols) return fail(std::string("cannot read ") + argv[1]);
      memcpy(image.data, pix.data(), pix.size() * sizeof(float));
   }

   Driver d(image, pp, ap, sp);
   if (!shapesPath.empty()) {
      std::vector<ShapeIn> in;
      if (!readAll(shapesPath, in)) return fail("cannot read " + shapesPath);
      for (const ShapeIn &q : in) {
         Record &r = d.open(q.x, q.y, q.s, 0.0f, 0, 0.0f, -1);
         d.describe(r, q.x, q.y, q.s, q.u[0], q.u[1], q.u[2], q.u[3]);
      }
   } else {
      d.keypointsOnly = !pointsPath.empty();
      d.detectPyramidKeypoints(image);
      if (!pointsPath.empty()) {
         std::vector<PointIn> in;
         if (!readAll(pointsPath, in)) return fail("cannot read " + pointsPath);
         d.keypointsOnly = false;
         d.records.clear();
         for (const PointIn &q : in) {
            if (q.plane < 0 || q.plane >= (int)d.planes.size()) return fail("point names a plane that was not captured");
            const float pd = d.planeDistance[q.plane];
            d.open(q.x, q.y, q.s, pd, 0, 0.0f, q.plane);
            d.findAffineShape(d.planes[q.plane], q.x, q.y, q.s, pd, 0, 0.0f);
         }
      }
   }

   FILE *f = fopen(argv[4], "wb");
   if (!f) return fail(std::string("cannot write ") + argv[4]);
   if (!d.records.empty()) fwrite(d.records.data(), sizeof(Record), d.records.size(), f);
   fclose(f);
   if (!planesPath.empty()) {
      f = fopen(planesPath.c_str(), "wb");
      if (!f) return fail("cannot write " + planesPath);
      for (size_t i = 0; i < d.planes.size(); i++) {
         const Mat &m = d.planes[i];
         const int32_t dims[2] = {m.rows, m.cols};
         fwrite(dims, sizeof dims, 1, f);
         fwrite(&d.planeDistance[i], sizeof(float), 1, f);
         for (int r = 0; r < m.rows; r++) fwrite(m.ptr<float>(r), sizeof(float), m.cols, f);
      }
      fclose(f);
   }
   size_t described = 0;
   for (const Record &r : d.records) described += r.fate == DESCRIBED;
   printf("%zu records, %zu described, %zu planes\n", d.records.size(), described, d.planes.size());
   return 0;
}
