// hesaff.hpp -- C++ host mirror of the reference's operator interface for the detect +
// describe path, implemented over the C ABI (include/hesaff_amd.h).  Names, argument
// meaning and outputs follow hesaff.cpp:21-131: HessianAffineParams (defaults :28-35),
// Keypoint (:41-48), AffineHessianDetector::{detectPyramidKeypoints, keys,
// exportKeypoints}, and the reference's two per-keypoint virtual callbacks
// HessianKeypointCallback (pyramid.h:43-47) and AffineShapeCallback (affine.h:48-58) with
// their setters.  The GPU runs the stages breadth-first and hands back the same `keys`
// vector, in the same order.  With a callback set, detectPyramidKeypoints replays the
// records of hesaff_detect_regions depth-first, in the reference's call order
// (hesaff.cpp:66-105): onHessianKeypointDetected for every Hessian keypoint, followed at
// once by onAffineShapeFound when findAffineShape converged.  The one difference: the
// callbacks observe a chain that has already run - a callback cannot suppress or alter
// the later stages of THAT run, and its `keys` is the same whatever the callbacks do.  What
// the reference lets a caller do by overriding or calling the two public callback members
// of AffineHessianDetector (hesaff.cpp:66-105) - keep the strongest N keypoints and only
// then find their shapes, describe the keypoints of another detector - is done here in two
// steps: collect the records in the callbacks (or bring your own), choose, and hand what
// was kept to onHessianKeypointsDetected (findAffineShape + the rest, hesaff.cpp:66-105) or
// onAffineShapesFound (rectify, normalizeAffine, SIFT, hesaff.cpp:73-105), the batch forms
// of those two members: they run the rest of the chain on the device for exactly the
// records given and fill `keys` and the counters from them.  The `blur` plane is
// a light handle (BlurPlane) instead of the cv::Mat; its pixels are those of
// hesaff_stage_pyramid's plane of that octave and level (hesaff_stage_pyramid_f32's for float input).
// detectPyramidKeypoints takes the reference's own input, a CV_32FC1 plane (pyramid.h:73), or
// the 8-bit image main() converts to one (hesaff.cpp:138-148).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <ostream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/hesaff_amd.h"

namespace hesaff_amd {

struct HessianAffineParams {   // hesaff.cpp:21-36
   float threshold;
   int max_iter;
   float desc_factor;
   int patch_size;
   bool verbose;
   HessianAffineParams()
   {
      threshold = 16.0f / 3.0f;
      max_iter = 16;
      desc_factor = 3.0f * std::sqrt(3.0f);
      patch_size = 41;
      verbose = false;
   }
};

typedef hesaff_keypoint Keypoint;   // hesaff.cpp:41-48, identical layout

// the `const cv::Mat &blur` argument of both callbacks: which plane of the scale space the keypoint was found / shaped on
// (pixels: the blur plane `level` of octave `octave` of hesaff_stage_pyramid - of hesaff_stage_pyramid_f32 when the input was a
// float plane), and that octave's pixelDistance (pyramid.cpp:288)
struct BlurPlane {
   int octave, level;
   float pixelDistance;
};

class HessianKeypointCallback {   // pyramid.h:43-47
 public:
   virtual void onHessianKeypointDetected(const BlurPlane &blur, float x, float y, float s, float pixelDistance, int type, float response) = 0;
   virtual ~HessianKeypointCallback() {}
};

struct AffineShapeCallback {   // affine.h:48-58; a11..a22 are U as found (not rectified), iters = l at affine.cpp:95
   virtual void onAffineShapeFound(const BlurPlane &blur, float x, float y, float s, float pixelDistance, float a11, float a12, float a21,
                                   float a22, int type, float response, int iters) = 0;
   virtual ~AffineShapeCallback() {}
};

struct AffineHessianDetector {
   std::vector<Keypoint> keys;      // hesaff.cpp:54
   int g_numberOfPoints = 0;        // hesaff.cpp:38
   int g_numberOfAffinePoints = 0;  // hesaff.cpp:39

   explicit AffineHessianDetector(const HessianAffineParams &par = HessianAffineParams(), int device = 0)
   {
      if (par.patch_size != 41) throw std::invalid_argument("patch_size is fixed at 41 in this build");
      // the structs carry no size field: refuse a library built from another header before passing one across
      if (hesaff_abi_version() != HESAFF_ABI_VERSION || hesaff_sizeof_params() != sizeof(hesaff_params) || hesaff_sizeof_timings() != sizeof(hesaff_timings) ||
          hesaff_sizeof_region() != sizeof(hesaff_region))
         throw std::runtime_error("libhesaff_amd.so was built from a different include/hesaff_amd.h (ABI version mismatch)");
      hesaff_default_params(&p_);
      p_.threshold = par.threshold;          // hesaff.cpp:155
      p_.maxIterations = par.max_iter;       // hesaff.cpp:158
      p_.mrSize = par.desc_factor;           // hesaff.cpp:160
      p_.max_batch = 1;
      if (hesaff_create(&ctx_, &p_, device) != HESAFF_OK) throw std::runtime_error(hesaff_last_error(nullptr));
   }
   ~AffineHessianDetector() { hesaff_destroy(ctx_); }
   AffineHessianDetector(const AffineHessianDetector &) = delete;
   AffineHessianDetector &operator=(const AffineHessianDetector &) = delete;

   // pyramid.h:69, affine.h:87 (nullptr: none).  The callbacks are the caller's; they are called from detectPyramidKeypoints.
   void setHessianKeypointCallback(HessianKeypointCallback *callback) { hessianKeypointCallback_ = callback; }
   void setAffineShapeCallback(AffineShapeCallback *callback) { affineShapeCallback_ = callback; }

   // No counterpart in the reference (hesaff_set_keypoint_limit, include/hesaff_amd.h): detectPyramidKeypoints keeps the n Hessian
   // keypoints of greatest |response| (ties at the cut to the earlier one) and drops the rest on the device before findAffineShape;
   // `keys`, the counters and the replayed callbacks then see only the kept keypoints, in the reference's order, each as the
   // unlimited run produces it.  n bounds Hessian keypoints, not descriptors; 0 (default): no limit.  The batch forms below
   // (onHessianKeypointsDetected, onAffineShapesFound) are not limited: their records are the caller's.
   void setKeypointLimit(int n)
   {
      if (hesaff_set_keypoint_limit(ctx_, n) != HESAFF_OK)
         throw std::invalid_argument("keypoint limit must be 0 (off) or positive, and not below the cells of a set keypoint grid");
   }

   // No counterpart in the reference (hesaff_set_keypoint_grid, include/hesaff_amd.h; OpenCV's GridAdaptedFeatureDetector): with a
   // keypoint limit n, detectPyramidKeypoints keeps the n / (rows * cols) strongest Hessian keypoints of every cell of a rows x cols
   // grid over the image - a budget spread over the image - in the reference's order; 1 x 1 (default): no grid.  rows * cols <= 64,
   // and no more cells than a set limit.
   void setKeypointGrid(int rows, int cols)
   {
      if (hesaff_set_keypoint_grid(ctx_, rows, cols) != HESAFF_OK)
         throw std::invalid_argument("keypoint grid needs rows, cols >= 1, rows * cols <= 64 and at most as many cells as a set keypoint limit");
   }

   // No counterpart in the reference (hesaff_set_orientation, include/hesaff_amd.h), whose descriptors live in the "up is up" frame of
   // rectifyAffineTransformationUpIsUp (hesaff.cpp:79).  HESAFF_ORI_DOMINANT: every region's frame is turned by the dominant gradient
   // angle of its own patch before normalizeAffine runs a second time and SIFT describes it; `keys` then holds A' = A R(theta) (theta =
   // atan2(-a12, a11)), descriptors follow an in-plane rotation of the image, and a region normalizeAffine rejects in either run has
   // no key.  The callbacks replay what they replay in mode 0: U stays un-rectified and un-turned.  One orientation per region
   // unless setOrientationCount says otherwise.
   // HESAFF_ORI_UP (default): the reference's behaviour, bit for bit.  Applies to detectPyramidKeypoints and to the batch forms below.
   void setOrientation(int mode)
   {
      if (hesaff_set_orientation(ctx_, mode) != HESAFF_OK) throw std::invalid_argument("orientation is HESAFF_ORI_UP or HESAFF_ORI_DOMINANT");
   }

   // Secondary orientation peaks (hesaff_set_orientation_count, include/hesaff_amd.h): with HESAFF_ORI_DOMINANT a region gets up to k
   // keys, k in 1..4, one per peak of its orientation histogram within 80 % of the highest, adjacent in `keys` in ascending rank - `keys`
   // may then be longer than the number of regions.  The callbacks still replay once per region.  1 (default): one key per region.
   void setOrientationCount(int k)
   {
      if (hesaff_set_orientation_count(ctx_, k) != HESAFF_OK) throw std::invalid_argument("orientation count is 1..4");
   }

   // No counterpart in the reference (hesaff_set_descriptor, include/hesaff_amd.h), whose descriptors are SIFT bytes.
   // HESAFF_DESC_ROOTSIFT: the vector is L1-normalised and square-rooted on the device before it is quantised (RootSIFT); only
   // `desc` of the keys changes.  HESAFF_DESC_SIFT (default): the reference's bytes, bit for bit.
   void setDescriptor(int mode)
   {
      if (hesaff_set_descriptor(ctx_, mode) != HESAFF_OK) throw std::invalid_argument("descriptor is HESAFF_DESC_SIFT or HESAFF_DESC_ROOTSIFT");
   }

   // No counterpart in the reference (hesaff_set_vocabulary, include/hesaff_amd.h): a vocabulary of k rows of 128 bytes (copied; k = 0:
   // none, the default).  With one set, every call that fills `keys` also assigns each key its visual word on the device - the LOWEST
   // row of least squared distance to the key's descriptor bytes - and words() holds them; `keys` does not change by a bit.
   void setVocabulary(const uint8_t *words, int k)
   {
      const int rc = hesaff_set_vocabulary(ctx_, k, words);
      if (rc == HESAFF_ERR_ARG) throw std::invalid_argument("a vocabulary is k rows of 128 bytes, 0 <= k <= 2^20 (k = 0: none)");
      if (rc != HESAFF_OK) throw std::runtime_error(hesaff_last_error(ctx_));
      words_.clear();
      sigs_.clear();
   }
   // No counterpart in the reference (hesaff_set_embedding, include/hesaff_amd.h): a Hamming embedding over the vocabulary that is set -
   // P is 64 x 128 signed bytes in -127 .. 127, tau 64 int32 thresholds per row of the vocabulary (both copied; nullptr, nullptr:
   // none).  With one set every detection also gives each key a 64-bit signature: bit i is P[i] . desc > tau[word][i].
   // setVocabulary removes the embedding.
   void setEmbedding(const int8_t *P, const int32_t *tau)
   {
      const int rc = hesaff_set_embedding(ctx_, P, tau);
      if (rc == HESAFF_ERR_ARG) throw std::invalid_argument("an embedding needs a vocabulary, a projection with entries in -127 .. 127 and its thresholds (or neither)");
      if (rc != HESAFF_OK) throw std::runtime_error(hesaff_last_error(ctx_));
      sigs_.clear();
   }
   // a signature per key, parallel to `keys` and to words(): nullptr without an embedding or without keys
   const uint64_t *signatures() const { return sigs_.empty() ? nullptr : sigs_.data(); }
   // <image>.hesaff.sigs of the current keys (hesaff_write_signatures), row for row with exportWords' file
   // With a neighbour count R > 1 a row per key and present rank, like exportWords' file: rank 0 is signatures(), the ranks above are
   // made here under that rank's word (hesaff_stage_embed on the keys' descriptors with the neighbours as a words array of stride 2 R)
   void exportSignatures(const std::string &path) const
   {
      const size_t R = (size_t)neighboursR_, n = keys.size();
      if (R <= 1 || neighbours_.empty() || sigs_.empty()) {
         if (hesaff_write_signatures(path.c_str(), sigs_.data(), (int)sigs_.size()) != HESAFF_OK) throw std::runtime_error("cannot write " + path);
         return;
      }
      std::vector<uint8_t> desc(n * 128);
      for (size_t i = 0; i < n; i++) std::memcpy(&desc[i * 128], keys[i].desc, 128);
      std::vector<uint64_t> plane(n), rows;
      std::vector<std::vector<uint64_t>> by_rank(R);
      by_rank[0] = sigs_;
      for (size_t r = 1; r < R && neighbours_[2 * r] >= 0; r++) {   // (a rank is present for every key or for none: it is r < K)
         if (hesaff_stage_embed(ctx_, (int)n, desc.data(), neighbours_.data() + 2 * r, (int)(2 * R), plane.data()) != HESAFF_OK) throw std::runtime_error(hesaff_last_error(ctx_));
         by_rank[r] = plane;
      }
      for (size_t i = 0; i < n; i++)
         for (size_t r = 0; r < R; r++)
            if (neighbours_[(i * R + r) * 2] >= 0) rows.push_back(by_rank[r][i]);
      if (hesaff_write_signatures(path.c_str(), rows.data(), (int)rows.size()) != HESAFF_OK) throw std::runtime_error("cannot write " + path);
   }
   // the default projection of a seed (hesaff_embedding_projection): 64 x 128 bytes
   static std::vector<int8_t> embeddingProjection(uint64_t seed)
   {
      std::vector<int8_t> P((size_t)HESAFF_EMBED_BITS * 128);
      hesaff_embedding_projection(seed, P.data());
      return P;
   }
   // the thresholds of k words (hesaff_train_embedding): per word and bit the lower median of P . desc over the word's keys among n
   // descriptors of 128 bytes with words[i * wordStride] in 0 .. k - 1 -> k x 64 int32.  The detector's own embedding does not
   // change: install the result with setEmbedding.
   std::vector<int32_t> trainEmbedding(const uint8_t *desc, const int32_t *words, int wordStride, int n, int k, const int8_t *P)
   {
      std::vector<int32_t> tau((size_t)(k > 0 ? k : 0) * HESAFF_EMBED_BITS);
      const int rc = hesaff_train_embedding(ctx_, n, desc, words, wordStride, k, P, tau.data(), nullptr);
      if (rc == HESAFF_ERR_ARG) throw std::invalid_argument("training an embedding needs 1 <= n <= 2^24 descriptors, their words in 0 .. k - 1, k <= 2^20, and a projection in -127 .. 127");
      if (rc != HESAFF_OK) throw std::runtime_error(hesaff_last_error(ctx_));
      return tau;
   }
   // (word, dist2) per key, two int32 each, parallel to `keys`: nullptr without a vocabulary or without keys
   const int32_t *words() const { return words_.empty() ? nullptr : words_.data(); }
   // <image>.hesaff.words of the current keys (hesaff_write_words): x, y, a, b, c as exportKeypoints prints them, and the word
   // With a neighbour count R > 1: for every key in key order a row per present rank in ascending rank, the key's five floats with
   // that rank's word - an ordinary words file with up to R rows per key.
   void exportWords(const std::string &path) const
   {
      int k = 0;
      if (hesaff_get_vocabulary_size(ctx_, &k) != HESAFF_OK || k == 0) throw std::runtime_error("exportWords: no vocabulary is set");
      if (neighboursR_ > 1 && !neighbours_.empty()) {
         const size_t R = (size_t)neighboursR_;
         std::vector<hesaff_keypoint> rows;
         std::vector<int32_t> row_words;
         for (size_t i = 0; i < keys.size(); i++)
            for (size_t r = 0; r < R; r++) {
               const int32_t *nb = &neighbours_[(i * R + r) * 2];
               if (nb[0] < 0) continue;
               rows.push_back(keys[i]);
               row_words.push_back(nb[0]); row_words.push_back(nb[1]);
            }
         if (hesaff_write_words(path.c_str(), rows.data(), row_words.data(), (int)rows.size(), p_.mrSize, k) != HESAFF_OK)
            throw std::runtime_error("cannot write '" + path + "'");
         return;
      }
      if (hesaff_write_words(path.c_str(), keys.data(), words(), (int)keys.size(), p_.mrSize, k) != HESAFF_OK)
         throw std::runtime_error("cannot write '" + path + "'");
   }
   // No counterpart in the reference (hesaff_set_vocabulary_neighbours, include/hesaff_amd.h): every key's R nearest rows of the
   // vocabulary, 1..8 (default 1: the word alone).  A setting of the detector: setVocabulary keeps it.  With R > 1 every call also
   // fills neighbours(); words() stays rank 0.  Does not combine with a cell layer: either setter then throws and changes nothing.
   void setVocabularyNeighbours(int neighbours)
   {
      if (hesaff_set_vocabulary_neighbours(ctx_, neighbours) != HESAFF_OK)
         throw std::invalid_argument(neighbours < 1 || neighbours > 8 ? "vocabulary neighbours must be 1..8" : hesaff_last_error(ctx_));
      neighbours_.clear();
      neighboursR_ = 1;
   }
   int vocabularyNeighbours() const
   {
      int r = 1;
      hesaff_get_vocabulary_neighbours(ctx_, &r);
      return r;
   }
   // (word, dist2) per key and rank of the last call, neighboursRanks() x two int32 per key, parallel to `keys`: nullptr with R = 1,
   // without a vocabulary or without keys
   const int32_t *neighbours() const { return neighbours_.empty() ? nullptr : neighbours_.data(); }
   int neighboursRanks() const { return neighboursR_; }

   // No counterpart in the reference (hesaff_train_vocabulary, include/hesaff_amd.h): exact integer k-means on the device over n
   // descriptors of 128 bytes - the initial rows are desc[floor(r n / k)], at most `iterations` Lloyd iterations with the mean rounded
   // half up, fewer when a fixed point is reached.  -> the k rows; distortion() and emptyWords() then hold one entry per iteration
   // that ran.  The detector's own vocabulary does not change: install the result with setVocabulary.
   std::vector<uint8_t> trainVocabulary(const uint8_t *desc, int n, int k, int iterations)
   {
      std::vector<uint8_t> rows((size_t)(k > 0 ? k : 0) * 128);
      distortion_.assign((size_t)(iterations > 0 ? iterations : 0), 0);
      empty_.assign(distortion_.size(), 0);
      int done = 0;
      const int rc = hesaff_train_vocabulary(ctx_, n, desc, k, nullptr, iterations, rows.data(), distortion_.data(), empty_.data(), &done);
      if (rc != HESAFF_OK) { distortion_.clear(); empty_.clear(); }
      if (rc == HESAFF_ERR_ARG) throw std::invalid_argument("training needs 1 <= k <= 2^20 rows, k <= n <= 2^24 descriptors and iterations >= 1");
      if (rc != HESAFF_OK) throw std::runtime_error(hesaff_last_error(ctx_));
      distortion_.resize((size_t)done);
      empty_.resize((size_t)done);
      return rows;
   }
   const std::vector<int64_t> &distortion() const { return distortion_; }   // of the last trainVocabulary: distortion()[t] belongs to V_t
   const std::vector<int32_t> &emptyWords() const { return empty_; }

   // No counterpart in the reference (hesaff_set_vocabulary_cells, include/hesaff_amd.h): a cell layer over the vocabulary that is set -
   // c coarse rows of 128 bytes and first[c + 1], cell j owning rows first[j] .. first[j + 1] - 1 (copied; c = 0: none).  With one set
   // a key's word is the lowest nearest row of the cell of its lowest nearest coarse row.  setVocabulary removes the layer.
   void setVocabularyCells(const uint8_t *coarse, const uint32_t *first, int c)
   {
      const int rc = hesaff_set_vocabulary_cells(ctx_, c, coarse, first);
      if (rc == HESAFF_ERR_ARG && c > 0 && vocabularyNeighbours() > 1) throw std::invalid_argument(hesaff_last_error(ctx_));   // (the two do not combine)
      if (rc == HESAFF_ERR_ARG)
         throw std::invalid_argument("a cell layer needs a vocabulary of K rows, 0 <= c <= K coarse rows and first[0] = 0 < ... < first[c] = K");
      if (rc != HESAFF_OK) throw std::runtime_error(hesaff_last_error(ctx_));
      words_.clear();
   }
   // No counterpart in the reference (hesaff_set_vocabulary_probes, include/hesaff_amd.h): with a cell layer set, a key is searched in
   // its `probes` nearest cells, 1..8 (default 1: its one cell; at least the layer's cell count: the flat assignment).  A setting of the
   // detector: setVocabulary and setVocabularyCells keep it, and without a layer it has no effect.
   void setVocabularyProbes(int probes)
   {
      if (hesaff_set_vocabulary_probes(ctx_, probes) != HESAFF_OK) throw std::invalid_argument("vocabulary probes must be 1..8");
      words_.clear();
   }
   int vocabularyProbes() const
   {
      int p = 1;
      hesaff_get_vocabulary_probes(ctx_, &p);
      return p;
   }

   // A layer for k rows given c coarse rows (hesaff_build_vocabulary_cells): `rows` is put into cell order, order[new] = old row, the
   // coarse rows that attract a row and their `first` are returned.  The detector's own vocabulary does not change.
   struct VocabularyCells {
      std::vector<uint8_t> coarse;
      std::vector<uint32_t> first;
      std::vector<int32_t> order;
      int cells() const { return (int)first.size() - 1; }
   };
   VocabularyCells buildVocabularyCells(std::vector<uint8_t> &rows, const uint8_t *coarse, int c)
   {
      const int k = (int)(rows.size() / 128);
      VocabularyCells v;
      std::vector<uint8_t> sorted(rows.size());
      v.coarse.resize((size_t)(c > 0 ? c : 0) * 128);
      v.first.resize((size_t)(c > 0 ? c : 0) + 1);
      v.order.resize((size_t)k);
      int kept = 0;
      const int rc = hesaff_build_vocabulary_cells(ctx_, k, rows.data(), c, coarse, sorted.data(), v.order.data(), v.coarse.data(), v.first.data(), &kept);
      if (rc == HESAFF_ERR_ARG) throw std::invalid_argument("a cell layer is built for 1 <= k <= 2^20 rows from 1 <= c <= k coarse rows");
      if (rc != HESAFF_OK) throw std::runtime_error(hesaff_last_error(ctx_));
      v.coarse.resize((size_t)kept * 128);
      v.first.resize((size_t)kept + 1);
      rows.swap(sorted);
      return v;
   }
   // trainVocabulary on the rows of a layer, which stays fixed (hesaff_train_vocabulary_cells): `rows` are the initial k rows in the
   // layer's order -> the k rows; distortion() and emptyWords() as for trainVocabulary.
   std::vector<uint8_t> trainVocabularyCells(const uint8_t *desc, int n, const std::vector<uint8_t> &rows, const VocabularyCells &cells, int iterations)
   {
      const int k = (int)(rows.size() / 128);
      std::vector<uint8_t> out(rows.size());
      distortion_.assign((size_t)(iterations > 0 ? iterations : 0), 0);
      empty_.assign(distortion_.size(), 0);
      int done = 0;
      const int rc = hesaff_train_vocabulary_cells(ctx_, n, desc, k, rows.data(), cells.cells(), cells.coarse.data(), cells.first.data(), iterations, out.data(),
                                                   distortion_.data(), empty_.data(), &done);
      if (rc != HESAFF_OK) { distortion_.clear(); empty_.clear(); }
      if (rc == HESAFF_ERR_ARG) throw std::invalid_argument("cell training needs 1 <= n <= 2^24 descriptors, the k rows of the layer and iterations >= 1");
      if (rc != HESAFF_OK) throw std::runtime_error(hesaff_last_error(ctx_));
      distortion_.resize((size_t)done);
      empty_.resize((size_t)done);
      return out;
   }

   // No counterpart in the reference (hesaff_index_build, include/hesaff_amd.h): an inverted file with integer tf-idf scoring over the
   // words of a collection, built on the device.  words: the words of all images one after the other, counts[i] of them for image i,
   // key j's word at words[j * wordStride] (1: packed; 2: the (word, dist2) rows words() holds); vocabularySize: K, every word in
   // 0 .. K - 1.  A successful build replaces the detector's index; the detector's vocabulary plays no part.
   void buildIndex(const std::vector<int32_t> &counts, const int32_t *words, int wordStride, int vocabularySize)
   {
      const int rc = hesaff_index_build(ctx_, (int)counts.size(), counts.data(), words, wordStride, vocabularySize);
      if (rc == HESAFF_ERR_ARG)
         throw std::invalid_argument("an index takes 1..2^20 images of at most 2^18 words each in 0 .. vocabularySize - 1, 2^28 in all, vocabularySize <= 2^20");
      if (rc != HESAFF_OK) throw std::runtime_error(hesaff_last_error(ctx_));
   }
   // the first min(top, images) images in the order (score descending, image ascending) for a query of n words; 1 <= top <= 1024
   std::vector<std::pair<int32_t, double>> queryIndex(const int32_t *words, int n, int wordStride, int top)
   {
      std::vector<int32_t> images((size_t)(top > 0 && top <= 1024 ? top : 1));
      std::vector<double> scores(images.size());
      int count = 0;
      const int rc = hesaff_index_query(ctx_, n, words, wordStride, top, images.data(), scores.data(), &count);
      if (rc == HESAFF_ERR_ARG) throw std::invalid_argument("a query needs an index, at most 2^18 words inside its vocabulary and 1 <= top <= 1024");
      if (rc != HESAFF_OK) throw std::runtime_error(hesaff_last_error(ctx_));
      std::vector<std::pair<int32_t, double>> out((size_t)count);
      for (int i = 0; i < count; i++) out[(size_t)i] = {images[(size_t)i], scores[(size_t)i]};
      return out;
   }
   // The same index with a signature per key (hesaff_index_build_embedded), for the queryIndex overload below
   void buildIndex(const std::vector<int32_t> &counts, const int32_t *words, int wordStride, const uint64_t *signatures, int vocabularySize)
   {
      const int rc = hesaff_index_build_embedded(ctx_, (int)counts.size(), counts.data(), words, wordStride, signatures, vocabularySize);
      if (rc == HESAFF_ERR_ARG)
         throw std::invalid_argument("an embedded index takes 1..2^20 images of at most 2^18 words each in 0 .. vocabularySize - 1 with a signature per word, 2^28 in all");
      if (rc != HESAFF_OK) throw std::runtime_error(hesaff_last_error(ctx_));
   }
   // ... where a word match counts only if the two signatures differ in at most `hamming` bits, 0..64 (hesaff_index_query_embedded)
   std::vector<std::pair<int32_t, double>> queryIndex(const int32_t *words, int n, int wordStride, const uint64_t *signatures, int hamming, int top)
   {
      std::vector<int32_t> images((size_t)(top > 0 && top <= 1024 ? top : 1));
      std::vector<double> scores(images.size());
      int count = 0;
      const int rc = hesaff_index_query_embedded(ctx_, n, words, wordStride, signatures, hamming, top, images.data(), scores.data(), &count);
      if (rc == HESAFF_ERR_ARG) throw std::invalid_argument("an embedded query needs an index built with signatures, words inside its vocabulary, 0 <= hamming <= 64 and 1 <= top <= 1024");
      if (rc != HESAFF_OK) throw std::runtime_error(hesaff_last_error(ctx_));
      std::vector<std::pair<int32_t, double>> out((size_t)count);
      for (int i = 0; i < count; i++) out[(size_t)i] = {images[(size_t)i], scores[(size_t)i]};
      return out;
   }
   // Many queries in one call (hesaff_index_query_batch): counts[q] words of query q, the words of all queries one after the other
   // as buildIndex takes those of its images.  One ranked vector per query: what queryIndex returns for that query's words.
   std::vector<std::vector<std::pair<int32_t, double>>> queryIndexBatch(const std::vector<int32_t> &counts, const int32_t *words, int wordStride, int top)
   {
      return queryBatch_(counts, top, [&](int32_t *images, double *scores, int *count) {
         return hesaff_index_query_batch(ctx_, (int)counts.size(), counts.data(), words, wordStride, top, images, scores, count);
      });
   }
   // ... with a signature per word and a Hamming threshold, 0..64 (hesaff_index_query_batch_embedded): per query the embedded queryIndex
   std::vector<std::vector<std::pair<int32_t, double>>> queryIndexBatch(const std::vector<int32_t> &counts, const int32_t *words, int wordStride,
                                                                        const uint64_t *signatures, int hamming, int top)
   {
      return queryBatch_(counts, top, [&](int32_t *images, double *scores, int *count) {
         return hesaff_index_query_batch_embedded(ctx_, (int)counts.size(), counts.data(), words, wordStride, signatures, hamming, top, images, scores, count);
      });
   }
   // The device scratch a chunk of a batch may hold, in bytes; 0: the default.  Results do not depend on it.
   void setIndexBatchBudget(size_t bytes)
   {
      if (hesaff_index_set_batch_budget(ctx_, bytes) != HESAFF_OK) throw std::runtime_error(hesaff_last_error(ctx_));
   }
   size_t indexBatchBudget() const
   {
      size_t bytes = 0;
      hesaff_index_get_batch_budget(ctx_, &bytes);
      return bytes;
   }
   // Appends images to the detector's index (hesaff_index_add): counts[j] words of new image j, laid out as buildIndex's; the new
   // images take the numbers behind the index's.  The index that results is the one buildIndex would make of all images together.
   void addToIndex(const std::vector<int32_t> &counts, const int32_t *words, int wordStride)
   {
      const int rc = hesaff_index_add(ctx_, (int)counts.size(), counts.data(), words, wordStride);
      if (rc == HESAFF_ERR_ARG)
         throw std::invalid_argument("an add needs a plain index, at least one image, at most 2^20 images and 2^28 words with those of the index, every word inside its vocabulary");
      if (rc != HESAFF_OK) throw std::runtime_error(hesaff_last_error(ctx_));
   }
   // ... to an index built with signatures (hesaff_index_add_embedded)
   void addToIndex(const std::vector<int32_t> &counts, const int32_t *words, int wordStride, const uint64_t *signatures)
   {
      const int rc = hesaff_index_add_embedded(ctx_, (int)counts.size(), counts.data(), words, wordStride, signatures);
      if (rc == HESAFF_ERR_ARG)
         throw std::invalid_argument("an embedded add needs an index built with signatures, at least one image, at most 2^20 images and 2^28 words with those of the index");
      if (rc != HESAFF_OK) throw std::runtime_error(hesaff_last_error(ctx_));
   }
   // Removes the images with the given numbers from the detector's index (hesaff_index_remove): distinct, in any order, at least one
   // and not all.  The images that stay keep their order and are renumbered densely; the index that results is the one buildIndex
   // would make of them.  Returns the new number of every old image, -1 for a removed one.
   std::vector<int32_t> removeFromIndex(const std::vector<int> &images)
   {
      int n = 0;
      std::vector<int32_t> gone(images.begin(), images.end());
      if (hesaff_index_get_info(ctx_, &n, nullptr, nullptr, nullptr) != HESAFF_OK) throw std::invalid_argument("a removal needs an index");
      std::vector<int32_t> remap((size_t)n);
      const int rc = hesaff_index_remove(ctx_, (int)gone.size(), gone.data(), remap.data());
      if (rc == HESAFF_ERR_ARG)
         throw std::invalid_argument("a removal needs an index, at least one image and fewer than the index holds, every number inside the index and given once");
      if (rc != HESAFF_OK) throw std::runtime_error(hesaff_last_error(ctx_));
      return remap;
   }
   // The index to and from an index file (hesaff_index_save, hesaff_index_load: "HESAFFI1"); a file that is refused leaves the index as it was
   void saveIndex(const char *path)
   {
      const int rc = hesaff_index_save(ctx_, path);
      if (rc == HESAFF_ERR_ARG) throw std::invalid_argument("saveIndex needs an index and a path");
      if (rc != HESAFF_OK) throw std::runtime_error(hesaff_last_error(ctx_));
   }
   void loadIndex(const char *path)
   {
      const int rc = hesaff_index_load(ctx_, path);
      if (rc == HESAFF_ERR_ARG) throw std::invalid_argument(path ? hesaff_last_error(ctx_) : "loadIndex needs a path");
      if (rc != HESAFF_OK) throw std::runtime_error(hesaff_last_error(ctx_));
   }
   void clearIndex()
   {
      if (hesaff_index_clear(ctx_) != HESAFF_OK) throw std::runtime_error(hesaff_last_error(ctx_));
   }

   // No counterpart in the reference (hesaff_verify_matches, include/hesaff_amd.h): spatial verification of a shortlist.  queryRows
   // and candidateRows are rows of words files (24 bytes: x, y, a, b, c, word), the candidates' one image after the other, counts[r]
   // of them for candidate r; tolerance in pixels of the candidate image; maxPairs in 1..16.  Returns the candidates in the order
   // (inliers descending, position ascending); `results`, where given, receives one record per candidate, in the candidates' order.
   // Neither the detector's vocabulary nor its index plays a part.
   struct Verified { int32_t inliers, used, found, queryKey, candidateKey, inertKeys; float L11, L21, L22; };
   std::vector<int32_t> verifyMatches(const void *queryRows, int nq, const std::vector<int32_t> &counts, const void *candidateRows, int vocabularySize,
                                      float tolerance, int maxPairs = 1, std::vector<Verified> *results = nullptr)
   {
      const size_t R = counts.size();
      std::vector<int32_t> out(R * 6 + 1), order(R + 1);
      std::vector<float> hyp(R * 3 + 1);
      const int rc = hesaff_verify_matches(ctx_, nq, queryRows, (int)R, counts.data(), candidateRows, vocabularySize, maxPairs, tolerance, out.data(), hyp.data(),
                                           order.data());
      if (rc == HESAFF_ERR_ARG)
         throw std::invalid_argument("verification takes 1..1024 candidates of at most 2^18 rows each with words in 0 .. vocabularySize - 1, 1 <= maxPairs <= 16 and 0 < tolerance <= 2^20");
      if (rc != HESAFF_OK) throw std::runtime_error(hesaff_last_error(ctx_));
      order.resize(R);
      if (results) {
         results->resize(R);
         for (size_t r = 0; r < R; r++)
            (*results)[r] = {out[r * 6], out[r * 6 + 1], out[r * 6 + 2], out[r * 6 + 3], out[r * 6 + 4], out[r * 6 + 5], hyp[r * 3], hyp[r * 3 + 1], hyp[r * 3 + 2]};
      }
      return order;
   }

   // No counterpart in the reference (hesaff_expand_query, include/hesaff_amd.h): query expansion.  The rows of the query followed by
   // the keys of the verified candidates - results[r].inliers >= minInliers, the best maxImages of them - back-projected into the
   // query's frame by their maps and kept where they fall into roi = (x0, y0, x1, y1); `results` is what verifyMatches filled for the
   // same query and candidates.  Returns the expanded rows (24 bytes each; at most maxRows of them), which queryIndex - by their
   // words, `words`, where given - and verifyMatches take as they are; `info`, where given, receives one record per candidate.
   // With signatures (both arrays, and sigsOut) they travel with the rows.
   struct Expanded { int32_t rank, liveKeys, keptKeys, writtenKeys; };
   std::vector<char> expandQuery(const void *queryRows, int nq, const std::vector<int32_t> &counts, const void *candidateRows, const std::vector<Verified> &results,
                                 int vocabularySize, int minInliers, const float roi[4], int maxImages = 1024, int maxRows = 1 << 18,
                                 std::vector<int32_t> *words = nullptr, std::vector<Expanded> *info = nullptr, const uint64_t *querySigs = nullptr,
                                 const uint64_t *candidateSigs = nullptr, std::vector<uint64_t> *sigsOut = nullptr)
   {
      const size_t R = counts.size();
      if (results.size() != R) throw std::invalid_argument("expansion takes one verified record per candidate");
      std::vector<int32_t> out(R * 6 + 1), inf(R * 4 + 1);
      std::vector<float> hyp(R * 3 + 1);
      size_t cap = (size_t)std::max(nq, 0);
      for (size_t r = 0; r < R; r++) {
         const Verified &v = results[r];
         const int32_t o[6] = {v.inliers, v.used, v.found, v.queryKey, v.candidateKey, v.inertKeys};
         std::copy(o, o + 6, out.begin() + (std::ptrdiff_t)(r * 6));
         hyp[r * 3] = v.L11; hyp[r * 3 + 1] = v.L21; hyp[r * 3 + 2] = v.L22;
         cap += (size_t)std::max(counts[r], 0);
      }
      cap = std::max<size_t>(std::min<size_t>(cap, (size_t)std::max(maxRows, 0)), 1);
      std::vector<char> rows(cap * 24);
      std::vector<int32_t> w(cap);
      if (sigsOut) sigsOut->assign(cap, 0);
      int n = 0;
      const int rc = hesaff_expand_query(ctx_, nq, queryRows, querySigs, (int)R, counts.data(), candidateRows, candidateSigs, out.data(), hyp.data(), minInliers, maxImages,
                                         roi, vocabularySize, maxRows, rows.data(), w.data(), sigsOut ? sigsOut->data() : nullptr, &n, inf.data());
      if (rc == HESAFF_ERR_ARG)
         throw std::invalid_argument("expansion takes the arguments and the results of verifyMatches, minInliers >= 1, 1 <= maxImages <= 1024, a finite region within 2^20, "
                                     "nq <= maxRows <= 2^18, and signatures for both sides or for neither");
      if (rc != HESAFF_OK) throw std::runtime_error(hesaff_last_error(ctx_));
      rows.resize((size_t)n * 24);
      w.resize((size_t)n);
      if (sigsOut) sigsOut->resize((size_t)n);
      if (words) *words = w;
      if (info) {
         info->resize(R);
         for (size_t r = 0; r < R; r++) (*info)[r] = {inf[r * 4], inf[r * 4 + 1], inf[r * 4 + 2], inf[r * 4 + 3]};
      }
      return rows;
   }
   // the bounding box of the LIVE rows (step 1 of hesaff_verify_matches) of a words file's rows: the region of an expansion that is given
   // none.  false, and zeros, where no row is live.
   static bool liveBounds(const void *rows, int n, float roi[4])
   {
      bool any = false;
      roi[0] = roi[1] = roi[2] = roi[3] = 0.0f;
      for (int i = 0; i < n; i++) {
         float k[5];
         std::memcpy(k, (const char *)rows + (size_t)i * 24, 20);
         const float r = std::sqrt(k[4]);
         const float q = k[3] / r;
         const float qq = q * q;
         const float t = k[2] - qq;
         const float p = std::sqrt(t);
         const float lo = 9.5367431640625e-07f, hi = 1048576.0f;
         if (!(k[4] > 0.0f && t > 0.0f && p >= lo && p <= hi && r >= lo && r <= hi && k[2] <= 1099511627776.0f && std::fabs(k[0]) <= hi && std::fabs(k[1]) <= hi)) continue;
         if (!any) { roi[0] = roi[2] = k[0]; roi[1] = roi[3] = k[1]; any = true; }
         roi[0] = std::min(roi[0], k[0]); roi[1] = std::min(roi[1], k[1]); roi[2] = std::max(roi[2], k[0]); roi[3] = std::max(roi[3], k[1]);
      }
      return any;
   }

   // No counterpart in the reference (hesaff_set_next_masks, include/hesaff_amd.h; OpenCV's detect(image, keypoints, mask)): the NEXT
   // detectPyramidKeypoints keeps only the Hessian keypoints on a non-zero pixel of `mask` - height x width 8-bit pixels at the size of
   // the image as passed, rows strideBytes apart (0: tightly packed), pixel (row, col) = (clamp((int)(y + 0.5f)), clamp((int)(x +
   // 0.5f))) - and drops the rest on the device before findAffineShape; `keys`, the counters and the replayed callbacks see only the
   // kept keypoints, each as the unmasked run produces it.  One-shot: that call consumes the mask whatever it returns (nullptr:
   // disarm).  The pixels are not copied: they stay valid until that call has returned.  With a keypoint limit, the mask acts first.
   // The batch forms below take no mask: their records are the caller's.
   void setMask(const uint8_t *mask, size_t strideBytes = 0)
   {
      if (strideBytes > (size_t)0x7fffffff) throw std::invalid_argument("row stride too large");
      mask_ = mask;
      maskStride_ = (int)strideBytes;
   }

   // == grey conversion hesaff.cpp:138-148 + detectPyramidKeypoints hesaff.cpp:167 with the
   // whole callback chain; image is what cv::imread would deliver (8-bit, 1 or 3 channels).
   void detectPyramidKeypoints(const uint8_t *image, int width, int height, int channels)
   {
      const int stride = width * channels;
      armMask(width);
      if (!hessianKeypointCallback_ && !affineShapeCallback_) {
         hesaff_result r;
         if (hesaff_detect_batch(ctx_, 1, &image, &width, &height, &stride, &channels, &r) != HESAFF_OK)
            throw std::runtime_error(hesaff_last_error(ctx_));
         take(r.count_hessian, r.count_desc, r.keys);
         return;
      }
      hesaff_region_result r;
      if (hesaff_detect_regions(ctx_, 1, &image, &width, &height, &stride, &channels, &r) != HESAFF_OK)
         throw std::runtime_error(hesaff_last_error(ctx_));
      replay(r);
   }

   // == detectPyramidKeypoints(const Mat &image) pyramid.h:73 with a CV_32FC1 image, the reference's own detector input:
   // image.ptr<float>(0), image.cols, image.rows, image.step.  strideBytes = 0: tightly packed rows.  Every pixel must be finite
   // with |v| <= 2^20 (include/hesaff_amd.h); otherwise std::runtime_error naming the first offending pixel.
   void detectPyramidKeypoints(const float *image, int width, int height, size_t strideBytes = 0)
   {
      if (strideBytes > (size_t)0x7fffffff) throw std::invalid_argument("row stride too large");
      const int stride = strideBytes ? (int)strideBytes : width * 4;
      armMask(width);
      if (!hessianKeypointCallback_ && !affineShapeCallback_) {
         hesaff_result r;
         if (hesaff_detect_batch_f32(ctx_, 1, &image, &width, &height, &stride, &r) != HESAFF_OK) throw std::runtime_error(hesaff_last_error(ctx_));
         take(r.count_hessian, r.count_desc, r.keys);
         return;
      }
      hesaff_region_result r;
      if (hesaff_detect_regions_f32(ctx_, 1, &image, &width, &height, &stride, &r) != HESAFF_OK) throw std::runtime_error(hesaff_last_error(ctx_));
      replay(r);
   }

   // The batch forms of the reference's two public callback members (hesaff.cpp:66-71 and :73-105) for one image: the rest of the
   // chain for the caller's records (hesaff_describe_regions).  image: the image the keypoints belong to, as detectPyramidKeypoints
   // takes it.  records: hesaff_region, e.g. region() of what a callback received, or rows of hesaff_detect_regions; which fields are
   // read, and which values are refused (std::runtime_error naming the record), is in include/hesaff_amd.h.  keys is replaced by the
   // descriptors of these records, in their order; g_numberOfPoints = records.size(), g_numberOfAffinePoints grows by keys.size() -
   // as detectPyramidKeypoints leaves them.  described (optional) receives the records with a11..a22, iters, outcome and key
   // filled in.  The callbacks set on this detector are not called: the caller made these calls itself.
   // == onHessianKeypointDetected(blur, x, y, s, pixelDistance, type, response) per record, blur = the plane (octave, level)
   void onHessianKeypointsDetected(const uint8_t *image, int width, int height, int channels, const std::vector<hesaff_region> &records,
                                   std::vector<hesaff_region> *described = nullptr)
   {
      describe(image, width, height, channels, records, HESAFF_FROM_POINTS, described);
   }
   void onHessianKeypointsDetected(const float *image, int width, int height, size_t strideBytes, const std::vector<hesaff_region> &records,
                                   std::vector<hesaff_region> *described = nullptr)
   {
      describe_f32(image, width, height, strideBytes, records, HESAFF_FROM_POINTS, described);
   }
   // == onAffineShapeFound(blur, x, y, s, pixelDistance, a11, a12, a21, a22, type, response, iters) per record (U not rectified)
   void onAffineShapesFound(const uint8_t *image, int width, int height, int channels, const std::vector<hesaff_region> &records,
                            std::vector<hesaff_region> *described = nullptr)
   {
      describe(image, width, height, channels, records, HESAFF_FROM_SHAPES, described);
   }
   void onAffineShapesFound(const float *image, int width, int height, size_t strideBytes, const std::vector<hesaff_region> &records,
                            std::vector<hesaff_region> *described = nullptr)
   {
      describe_f32(image, width, height, strideBytes, records, HESAFF_FROM_SHAPES, described);
   }
   // the record of a keypoint as the callbacks received it (a11..a22 / iters: leave at 0 for onHessianKeypointsDetected)
   static hesaff_region region(const BlurPlane &blur, float x, float y, float s, int type, float response, float a11 = 0.0f, float a12 = 0.0f,
                               float a21 = 0.0f, float a22 = 0.0f, int iters = 0)
   {
      hesaff_region g = {};
      g.x = x; g.y = y; g.s = s; g.pixelDistance = blur.pixelDistance; g.response = response;
      g.type = type; g.octave = blur.octave; g.level = blur.level;
      g.a11 = a11; g.a12 = a12; g.a21 = a21; g.a22 = a22; g.iters = iters;
      g.key = -1;
      return g;
   }

   // hesaff.cpp:107-130
   void exportKeypoints(std::ostream &out)
   {
      char *buf = nullptr;
      size_t len = 0;
      if (hesaff_format_sift_mt(keys.data(), (int)keys.size(), p_.mrSize, 0, &buf, &len) != HESAFF_OK)   // rows on all host cores
         throw std::runtime_error("hesaff_format_sift_mt failed");
      out.write(buf, (std::streamsize)len);
      out.flush();
      hesaff_free(buf);
   }

 private:
   // setMask's mask goes to the context for the call that follows, and leaves this object
   void armMask(int width)
   {
      const uint8_t *mask = mask_;
      const int stride = maskStride_ ? maskStride_ : width;
      mask_ = nullptr;
      maskStride_ = 0;
      if (mask && hesaff_set_next_masks(ctx_, 1, &mask, &stride) != HESAFF_OK) throw std::runtime_error("hesaff_set_next_masks failed");
   }
   void take(int count_hessian, int count_desc, const hesaff_keypoint *k)
   {
      g_numberOfPoints = count_hessian;
      g_numberOfAffinePoints += count_desc;   // the reference never resets this counter (hesaff.cpp:166)
      keys.assign(k, k + count_desc);
      // the words of these keys, when a vocabulary is set (every call here has one image: index 0)
      words_.clear();
      int vk = 0, n = 0;
      const int32_t *w = nullptr;
      if (hesaff_get_vocabulary_size(ctx_, &vk) == HESAFF_OK && vk > 0) {
         if (hesaff_get_words(ctx_, 0, &w, &n) != HESAFF_OK) throw std::runtime_error("hesaff_get_words failed");
         if (n > 0) words_.assign(w, w + 2 * (size_t)n);
      }
      // ... their neighbours, when a neighbour count above 1 is set
      neighbours_.clear();
      neighboursR_ = 1;
      if (vk > 0 && vocabularyNeighbours() > 1) {
         int m = 0, r = 1;
         const int32_t *nb = nullptr;
         if (hesaff_get_neighbours(ctx_, 0, &nb, &m, &r) != HESAFF_OK) throw std::runtime_error("hesaff_get_neighbours failed");
         neighboursR_ = r;
         if (m > 0) neighbours_.assign(nb, nb + 2 * (size_t)m * (size_t)r);
      }
      // ... and their signatures, when an embedding is set as well
      sigs_.clear();
      int ek = 0, m = 0;
      const uint64_t *g = nullptr;
      if (vk > 0 && hesaff_get_embedding(ctx_, &ek, nullptr, nullptr) == HESAFF_OK && ek > 0) {
         if (hesaff_get_signatures(ctx_, 0, &g, &m) != HESAFF_OK) throw std::runtime_error("hesaff_get_signatures failed");
         if (m > 0) sigs_.assign(g, g + (size_t)m);
      }
   }
   void taken(const hesaff_region_result &r, std::vector<hesaff_region> *described)
   {
      take(r.count_hessian, r.count_desc, r.keys);
      if (described) described->assign(r.regions, r.regions + r.count_hessian);   // (count 0: regions is null, the range empty)
   }
   void describe(const uint8_t *image, int width, int height, int channels, const std::vector<hesaff_region> &records, int from,
                 std::vector<hesaff_region> *described)
   {
      const int stride = width * channels, count = (int)records.size();
      const hesaff_region *recs = records.data();
      hesaff_region_result r;
      if (hesaff_describe_regions(ctx_, 1, &image, &width, &height, &stride, &channels, &recs, &count, from, &r) != HESAFF_OK)
         throw std::runtime_error(hesaff_last_error(ctx_));
      taken(r, described);
   }
   void describe_f32(const float *image, int width, int height, size_t strideBytes, const std::vector<hesaff_region> &records, int from,
                     std::vector<hesaff_region> *described)
   {
      if (strideBytes > (size_t)0x7fffffff) throw std::invalid_argument("row stride too large");
      const int stride = strideBytes ? (int)strideBytes : width * 4, count = (int)records.size();
      const hesaff_region *recs = records.data();
      hesaff_region_result r;
      if (hesaff_describe_regions_f32(ctx_, 1, &image, &width, &height, &stride, &recs, &count, from, &r) != HESAFF_OK)
         throw std::runtime_error(hesaff_last_error(ctx_));
      taken(r, described);
   }
   void replay(const hesaff_region_result &r)
   {
      take(r.count_hessian, r.count_desc, r.keys);
      // hesaff.cpp:66-105 depth-first: each Hessian keypoint, then its affine shape when findAffineShape converged
      for (int i = 0; i < r.count_hessian; i++) {
         const hesaff_region &g = r.regions[i];
         const BlurPlane blur = {g.octave, g.level, g.pixelDistance};
         if (hessianKeypointCallback_) hessianKeypointCallback_->onHessianKeypointDetected(blur, g.x, g.y, g.s, g.pixelDistance, g.type, g.response);
         if (affineShapeCallback_ && g.outcome >= 1)
            affineShapeCallback_->onAffineShapeFound(blur, g.x, g.y, g.s, g.pixelDistance, g.a11, g.a12, g.a21, g.a22, g.type, g.response, g.iters);
      }
   }
   // queryIndexBatch: the flat rows of a batch call as one ranked vector per query
   template <class Call> std::vector<std::vector<std::pair<int32_t, double>>> queryBatch_(const std::vector<int32_t> &counts, int top, Call call)
   {
      const size_t row = (size_t)(top > 0 && top <= 1024 ? top : 1), nq = counts.empty() ? 1 : counts.size();
      std::vector<int32_t> images(nq * row);
      std::vector<double> scores(nq * row);
      int count = 0;
      const int rc = call(images.data(), scores.data(), &count);
      if (rc == HESAFF_ERR_ARG)
         throw std::invalid_argument("a batch needs an index (built with signatures for the embedded form), 1..2^16 queries of at most 2^18 words each inside its vocabulary, "
                                     "2^28 in all, 0 <= hamming <= 64 and 1 <= top <= 1024");
      if (rc != HESAFF_OK) throw std::runtime_error(hesaff_last_error(ctx_));
      std::vector<std::vector<std::pair<int32_t, double>>> out(counts.size());
      for (size_t q = 0; q < counts.size(); q++) {
         out[q].resize((size_t)count);
         for (int i = 0; i < count; i++) out[q][(size_t)i] = {images[q * row + (size_t)i], scores[q * row + (size_t)i]};
      }
      return out;
   }

   hesaff_params p_;
   hesaff_ctx *ctx_ = nullptr;
   HessianKeypointCallback *hessianKeypointCallback_ = nullptr;
   AffineShapeCallback *affineShapeCallback_ = nullptr;
   std::vector<int32_t> words_;      // setVocabulary: (word, dist2) per key
   std::vector<int32_t> neighbours_; // setVocabularyNeighbours above 1: (word, dist2) per key and rank
   int neighboursR_ = 1;             // ... and the ranks per key they hold
   std::vector<uint64_t> sigs_;      // setEmbedding: a signature per key
   std::vector<int64_t> distortion_; // trainVocabulary: per iteration that ran
   std::vector<int32_t> empty_;
   const uint8_t *mask_ = nullptr;   // setMask
   int maskStride_ = 0;
};

} // namespace hesaff_amd
