// index_plan.h -- the host arithmetic of the image index (hesaff_index_build / hesaff_index_query, include/hesaff_amd.h): which calls
// are refused, the packing of host words and the key starts of a call's images or queries, the integer logarithm behind idf, the key
// and the size of the build's hash table, and where the arrays of an index and of a build lie in their buffers.  Pure functions and plain structs, no HIP: capi_index.h and kernels_index.h obtain their numbers
// here, and tests/native/index_plan_check.cpp checks them on the CPU (tests/test_image_index_host.py).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "buffer_layouts.h"   // StagePlan, Span

#if defined(__HIPCC__)
#define HS_INDEX_HD __host__ __device__ __forceinline__
#else
#define HS_INDEX_HD inline
#endif

namespace hesaff_plan {

// The bounds, and why every sum of the definition stays inside uint64: idf <= 6143 < 2^13, so idf^2 < 2^26; a query and an image hold
// at most 2^18 keys each, so sum_w tfq(w) tf(i, w) <= 2^18 * 2^18 = 2^36 and sum_w tf(i, w)^2 <= 2^36; hence dot, nq2 and norm2 are
// each below 2^36 * 2^26 = 2^62.  A single term (tf * idf)^2 < (2^18 * 2^13)^2 = 2^62 as well.
constexpr int64_t HS_INDEX_MAX_IMAGES = (int64_t)1 << 20;       // the image index takes 20 bits of the hash key
constexpr int64_t HS_INDEX_MAX_WORDS = (int64_t)1 << 20;        // hesaff_set_vocabulary's bound; the word takes the key's other 20 bits
constexpr int64_t HS_INDEX_MAX_IMAGE_KEYS = (int64_t)1 << 18;   // of an image, and of a query
constexpr int64_t HS_INDEX_MAX_KEYS = (int64_t)1 << 28;         // of a build: the posting offsets are uint32
constexpr int HS_INDEX_MAX_TOP = 1024;                          // the survivors of a query are sorted by one block
constexpr uint32_t HS_INDEX_MAX_IDF = 6143;                     // ilog2_q8 at N / df < 2^24

inline bool index_counts_ok(int64_t n_images, int64_t k) { return n_images >= 1 && n_images <= HS_INDEX_MAX_IMAGES && k >= 1 && k <= HS_INDEX_MAX_WORDS; }
inline bool index_image_keys_ok(int64_t count) { return count >= 0 && count <= HS_INDEX_MAX_IMAGE_KEYS; }
inline bool index_total_ok(int64_t total) { return total >= 0 && total <= HS_INDEX_MAX_KEYS; }
inline bool index_word_stride_ok(int64_t stride) { return stride == 1 || stride == 2; }
inline bool index_query_ok(int64_t n, int64_t top) { return index_image_keys_ok(n) && top >= 1 && top <= HS_INDEX_MAX_TOP; }
// counts[n_images] -> the number of keys, or -1 where an image or the sum is out of bounds
inline int64_t index_total_keys(const int32_t *counts, int64_t n_images)
{
   int64_t total = 0;
   for (int64_t i = 0; i < n_images; i++) {
      if (!index_image_keys_ok(counts[i])) return -1;
      total += counts[i];
   }
   return index_total_ok(total) ? total : -1;
}
// starts[n + 1]: image (or query) i's keys are words[starts[i] .. starts[i + 1]), an item without keys repeats a start.  The sums
// are the caller's to bound (index_total_keys); they are made modulo 2^32
inline void index_starts(const int32_t *counts, int64_t n, uint32_t *starts)
{
   starts[0] = 0;
   for (int64_t i = 0; i < n; i++) starts[i + 1] = starts[i] + (uint32_t)counts[i];
}
// words in host memory, key j's at words[j * word_stride] -> packed, checked against 0 .. k - 1 on the way (false: one lies outside)
inline bool index_stage_words(const int32_t *words, int64_t word_stride, int64_t n, int64_t k, std::vector<int32_t> &out)
{
   out.resize((size_t)n);
   for (int64_t j = 0; j < n; j++) {
      const int32_t w = words[j * word_stride];
      if (w < 0 || w >= k) return false;
      out[(size_t)j] = w;
   }
   return true;
}

// idf of a word in df of n images, 1 <= df <= n < 2^33: floor(256 log2(n / df)) but for the truncations below, which ARE the
// definition.  q = floor(n 2^31 / df) lies in [2^31, 2^64); m is q's leading 32 bits, in [2^31, 2^32), so m * m < 2^64; eight
// squarings yield eight fraction bits.
HS_INDEX_HD uint32_t ilog2_q8(uint64_t n, uint64_t df)
{
   const uint64_t q = (n << 31) / df;
   const int e = 63 - __builtin_clzll(q) - 31;
   uint64_t m = q >> e;
   uint32_t r = (uint32_t)e;
   for (int i = 0; i < 8; i++) {
      m = (m * m) >> 31;
      r *= 2;
      if (m >= ((uint64_t)1 << 32)) { r += 1; m >>= 1; }
   }
   return r;
}
HS_INDEX_HD uint32_t index_idf(uint64_t n_images, uint32_t df) { return df == 0 ? 0u : ilog2_q8(n_images, df); }

// ---- the build's hash table: one slot per distinct (image, word) ----
constexpr uint64_t HS_INDEX_EMPTY = ~(uint64_t)0;   // no key has bits above 40
HS_INDEX_HD uint64_t index_key(uint32_t image, uint32_t word) { return ((uint64_t)image << 20) | (uint64_t)word; }
HS_INDEX_HD uint32_t index_key_image(uint64_t key) { return (uint32_t)(key >> 20); }
HS_INDEX_HD uint32_t index_key_word(uint64_t key) { return (uint32_t)(key & 0xfffffu); }
// slots: the power of two that is at least 2 T and at least 1024, so that a probe always meets an empty slot
inline int index_hash_bits(int64_t total_keys)
{
   int bits = 10;
   while (((int64_t)1 << bits) < 2 * total_keys) bits++;
   return bits;
}
inline uint64_t index_hash_slots(int64_t total_keys) { return (uint64_t)1 << index_hash_bits(total_keys); }
// a key's first slot: the top `bits` bits of the key times 2^64 / phi; the probe goes on to slot + 1, + 2 .. modulo the table
HS_INDEX_HD uint64_t index_hash_slot(uint64_t key, int bits) { return (key * 0x9E3779B97F4A7C15ull) >> (64 - bits); }

// ---- the persistent arrays of an index, one buffer, each 256-byte aligned; the posting lists are a buffer of their own, sized once
// the number of distinct (image, word) pairs is known ----
struct IndexPosting { uint32_t image, tf; };
static_assert(sizeof(IndexPosting) == 8, "8 bytes per posting");
struct IndexResultHead { unsigned long long nq2; uint32_t count, pad; };   // of the last query: its squared norm and its result count
static_assert(sizeof(IndexResultHead) == 16, "one 16-byte copy");
struct IndexArrays {
   Span<uint32_t> offsets;            // [k + 1]: word w's postings are lists[offsets[w] .. offsets[w + 1])
   Span<uint32_t> df, idf;            // [k]
   Span<uint32_t> tfq;                // [k]: zero between queries
   Span<unsigned long long> norm2;    // [n]
   Span<unsigned long long> dot;      // [n]: of the last query
   Span<double> score;                // [n]: of the last query
   Span<IndexResultHead> head;
   Span<double> top_scores;           // [HS_INDEX_MAX_TOP]: the last query's ranked scores ...
   Span<int32_t> top_images;          // ... and images
};
inline IndexArrays index_arrays(StagePlan &p, int64_t n_images, int64_t k)
{
   IndexArrays a;
   a.offsets = p.add<uint32_t>((size_t)k + 1);
   a.df = p.add<uint32_t>((size_t)k);
   a.idf = p.add<uint32_t>((size_t)k);
   a.tfq = p.add<uint32_t>((size_t)k);
   a.norm2 = p.add<unsigned long long>((size_t)n_images);
   a.dot = p.add<unsigned long long>((size_t)n_images);
   a.score = p.add<double>((size_t)n_images);
   a.head = p.add<IndexResultHead>(1);
   a.top_scores = p.add<double>((size_t)HS_INDEX_MAX_TOP);
   a.top_images = p.add<int32_t>((size_t)HS_INDEX_MAX_TOP);
   return a;
}
inline size_t index_lists_bytes(int64_t n_postings) { return (size_t)(n_postings > 0 ? n_postings : 1) * sizeof(IndexPosting); }

// ---- the scratch of a build, released before the call returns ----
struct IndexBuildArrays {
   Span<unsigned long long> hash_keys;   // [slots]: HS_INDEX_EMPTY or index_key(image, word)
   Span<uint32_t> hash_tf;               // [slots]
   Span<uint32_t> starts;                // [n + 1]: image i's keys are words[starts[i] .. starts[i + 1])
   Span<uint32_t> cursor;                // [k]: each list's next free position
   Span<uint32_t> block_sums;            // the scan's, one per 4096 words and one more
   uint64_t slots;
   int bits;
};
inline IndexBuildArrays index_build_arrays(StagePlan &p, int64_t n_images, int64_t k, int64_t total_keys)
{
   IndexBuildArrays b;
   b.bits = index_hash_bits(total_keys);
   b.slots = (uint64_t)1 << b.bits;
   b.hash_keys = p.add<unsigned long long>((size_t)b.slots);
   b.hash_tf = p.add<uint32_t>((size_t)b.slots);
   b.starts = p.add<uint32_t>((size_t)n_images + 1);
   b.cursor = p.add<uint32_t>((size_t)k);
   b.block_sums = p.add<uint32_t>(((size_t)k + 4095) / 4096 + 1);
   return b;
}
// the bytes a build holds at its peak beside the caller's words: index, lists (at most one posting per key) and scratch
// (n = k = 2^20, T = 2^28: 8.04 GiB, of which the hash table is 6)
inline size_t index_working_set_bytes(int64_t n_images, int64_t k, int64_t total_keys)
{
   StagePlan a, b;
   index_arrays(a, n_images, k);
   index_build_arrays(b, n_images, k, total_keys);
   return a.bytes() + b.bytes() + index_lists_bytes(total_keys);
}

// ---- growing an index (hesaff_index_add): n_old images of keys_old keys take m more of keys_new keys (each count already inside
// index_image_keys_ok); the sums are the build's bounds ----
inline bool index_add_ok(int64_t n_old, int64_t m, int64_t keys_old, int64_t keys_new)
{
   if (n_old < 1 || n_old > HS_INDEX_MAX_IMAGES || m < 1 || m > HS_INDEX_MAX_IMAGES || n_old + m > HS_INDEX_MAX_IMAGES) return false;
   return index_total_ok(keys_old) && index_total_ok(keys_new) && keys_old + keys_new <= HS_INDEX_MAX_KEYS;
}
// the bytes an add holds at its peak beside the caller's words and the old index: the new tables, the new lists (at most one
// posting per key of either) and a scratch whose hash table is sized for the NEW keys alone (n_old = 2^20 - 1, m = 1, k = 2^20,
// keys_old = 2^28 - 2^18, keys_new = 2^18: 2.05 GiB, of which the lists are 2 and the hash table 6 MiB)
inline size_t index_add_working_set_bytes(int64_t n_old, int64_t m, int64_t k, int64_t keys_old, int64_t keys_new)
{
   StagePlan a, b;
   index_arrays(a, n_old + m, k);
   index_build_arrays(b, m, k, keys_new);
   return a.bytes() + b.bytes() + index_lists_bytes(keys_old + keys_new);
}

// ---- the index file (hesaff_index_save / hesaff_index_load).  Little-endian, every array on a multiple of 8 bytes:
//   char magic[8] = "HESAFFI1"; uint32 flags (bit 0: embedded), k, n_images, reserved = 0; uint64 n_keys, n_postings;
//   uint32 df[k] (+ 4 bytes of zero where k is odd); { uint32 image, tf } postings[n_postings], word-major;
//   embedded only: uint32 key_count[k] (+ pad); uint32 key_image[n_keys] (+ pad); uint64 key_sig[n_keys]
// idf, both offset tables and norm2 are derived on load. ----
constexpr size_t HS_INDEX_FILE_HEAD = 40;
constexpr uint32_t HS_INDEX_FILE_EMBEDDED = 1u;
struct IndexFileHead { uint32_t flags, k, n_images; uint64_t n_keys, n_postings; };
inline size_t index_file_pad8(size_t bytes) { return (bytes + 7) & ~(size_t)7; }
struct IndexFileLayout { size_t df, postings, key_count, key_image, key_sig, size; };   // byte offsets; the last three == size for a plain file
inline IndexFileLayout index_file_layout(const IndexFileHead &h)
{
   IndexFileLayout l;
   l.df = HS_INDEX_FILE_HEAD;
   l.postings = l.df + index_file_pad8((size_t)h.k * 4);
   size_t at = l.postings + (size_t)h.n_postings * 8;
   l.key_count = l.key_image = l.key_sig = at;
   if (h.flags & HS_INDEX_FILE_EMBEDDED) {
      l.key_image = l.key_count + index_file_pad8((size_t)h.k * 4);
      l.key_sig = l.key_image + index_file_pad8((size_t)h.n_keys * 4);
      at = l.key_sig + (size_t)h.n_keys * 8;
   }
   l.size = at;
   return l;
}
inline void index_file_put32(char *p, uint32_t v) { for (int i = 0; i < 4; i++) p[i] = (char)(v >> (8 * i)); }
inline void index_file_put64(char *p, uint64_t v) { for (int i = 0; i < 8; i++) p[i] = (char)(v >> (8 * i)); }
inline uint32_t index_file_get32(const char *p) { uint32_t v = 0; for (int i = 0; i < 4; i++) v |= (uint32_t)(unsigned char)p[i] << (8 * i); return v; }
inline uint64_t index_file_get64(const char *p) { uint64_t v = 0; for (int i = 0; i < 8; i++) v |= (uint64_t)(unsigned char)p[i] << (8 * i); return v; }
inline void index_file_head(char *out, const IndexFileHead &h)
{
   const char magic[8] = {'H', 'E', 'S', 'A', 'F', 'F', 'I', '1'};
   for (int i = 0; i < 8; i++) out[i] = magic[i];
   index_file_put32(out + 8, h.flags); index_file_put32(out + 12, h.k); index_file_put32(out + 16, h.n_images); index_file_put32(out + 20, 0u);
   index_file_put64(out + 24, h.n_keys); index_file_put64(out + 32, h.n_postings);
}
// the head of a file of `size` bytes -> true and *h where it is the head of a whole index file: magic, known flags, reserved 0,
// 1 <= k, n_images <= 2^20, n_postings <= n_keys <= 2^28, and the size the fields imply
inline bool index_file_parse_head(const char *in, uint64_t size, IndexFileHead *h)
{
   const char magic[8] = {'H', 'E', 'S', 'A', 'F', 'F', 'I', '1'};
   for (int i = 0; i < 8; i++) if (in[i] != magic[i]) return false;
   h->flags = index_file_get32(in + 8); h->k = index_file_get32(in + 12); h->n_images = index_file_get32(in + 16);
   h->n_keys = index_file_get64(in + 24); h->n_postings = index_file_get64(in + 32);
   if ((h->flags & ~HS_INDEX_FILE_EMBEDDED) != 0u || index_file_get32(in + 20) != 0u) return false;
   if (!index_counts_ok((int64_t)h->n_images, (int64_t)h->k)) return false;
   if (h->n_keys > (uint64_t)HS_INDEX_MAX_KEYS || h->n_postings > h->n_keys) return false;
   return index_file_layout(*h).size == size;
}

// ---- the rules the device pass of a load checks, one bit each in its flag word; the lowest set bit is the rule reported ----
constexpr uint32_t HS_LOAD_IMAGE = 1u;        // a posting's image >= n_images
constexpr uint32_t HS_LOAD_TF = 2u;           // a posting's tf outside 1 .. 2^18
constexpr uint32_t HS_LOAD_IMAGE_SUM = 4u;    // an image's tf sum above 2^18
constexpr uint32_t HS_LOAD_TOTAL = 8u;        // the tf of all postings != n_keys
constexpr uint32_t HS_LOAD_KEY_COUNT = 16u;   // embedded: a word's key count != the tf of its postings
constexpr uint32_t HS_LOAD_KEY_IMAGE = 32u;   // embedded: a key's image >= n_images
inline const char *index_load_rule(uint32_t flags)
{
   if (flags & HS_LOAD_IMAGE) return "a posting's image is not below n_images";
   if (flags & HS_LOAD_TF) return "a posting's tf is outside 1 .. 2^18";
   if (flags & HS_LOAD_IMAGE_SUM) return "an image's tf sum is above 2^18";
   if (flags & HS_LOAD_TOTAL) return "the tf of all postings is not n_keys";
   if (flags & HS_LOAD_KEY_COUNT) return "a word's key count is not the tf of its postings";
   if (flags & HS_LOAD_KEY_IMAGE) return "a key's image is not below n_images";
   return "";
}

} // namespace hesaff_plan
