// embed_plan.h -- the host arithmetic of Hamming embedding (hesaff_set_embedding, hesaff_train_embedding, hesaff_index_build_embedded of
// include/hesaff_amd.h): which calls are refused, the default projection's generator, the projection as k_embed_keys reads it, the
// range of a projection value, the rank of the lower median, the file headers, and where the arrays of a training call and of an
// embedded index's key lists lie in their buffers.  Pure functions and plain structs, no HIP: capi_embed.h, kernels_embed.h and
// hostio.cpp obtain their numbers here, and tests/native/embed_plan_check.cpp checks them on the CPU (tests/test_embedding_host.py).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "train_plan.h"   // StagePlan, Span, AccumulateArrays, HS_TRAIN_MAX_KEYS, HS_VOCAB_MAX_ROWS

namespace hesaff_plan {

constexpr int HS_EMBED_BITS = 64;                                 // HESAFF_EMBED_BITS: the rows of P and the bits of a signature
constexpr int HS_EMBED_DIM = 128;                                 // the columns of P: a descriptor's bytes
constexpr int HS_EMBED_TILE = 32;                                 // rows of P per tile (the M of the MFMA): two tiles
constexpr size_t HS_EMBED_P_BYTES = (size_t)HS_EMBED_BITS * HS_EMBED_DIM;
constexpr int64_t HS_EMBED_MAX_TRAIN_KEYS = HS_TRAIN_MAX_KEYS;    // hesaff_train_embedding: n <= 2^24
// |z| <= 128 * 127 * 255 = 4 145 280 < 2^22: z + 2^22 lies in (0, 2^23) and orders as z does - the 23 bits the median's select walks
constexpr int32_t HS_EMBED_Z_MAX = 128 * 127 * 255;
constexpr int32_t HS_EMBED_Z_BIAS = 1 << 22;
constexpr int HS_EMBED_Z_BITS = 23;
static_assert(HS_EMBED_Z_MAX < HS_EMBED_Z_BIAS, "z + 2^22 is positive and below 2^23");

// every entry of P in -127 .. 127: -128 is refused, so that |z| stays below 2^22 and -P is a projection as well
inline bool embed_projection_ok(const int8_t *P)
{
   if (!P) return false;
   for (size_t e = 0; e < HS_EMBED_P_BYTES; e++)
      if (P[e] == -128) return false;
   return true;
}
inline bool embed_threshold_ok(int64_t t) { return t >= 0 && t <= HS_EMBED_BITS; }
inline bool embed_train_counts_ok(int64_t n, int64_t k) { return n >= 1 && n <= HS_EMBED_MAX_TRAIN_KEYS && k >= 1 && k <= HS_VOCAB_MAX_ROWS; }
// the lower median of m >= 1 values sorted ascending is element (m - 1) / 2
HS_TRAIN_HD uint32_t embed_median_rank(uint32_t m) { return (m - 1u) / 2u; }

// hesaff_embedding_projection: entry e = i * 128 + j of P is the e-th output of splitmix64 started at `seed`, its top byte less 128,
// with -128 raised to -127
inline void embedding_projection(uint64_t seed, int8_t *P)
{
   uint64_t s = seed;
   for (size_t e = 0; e < HS_EMBED_P_BYTES; e++) {
      s += 0x9E3779B97F4A7C15ull;
      uint64_t x = s;
      x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
      x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
      x ^= x >> 31;
      const int v = (int)(x >> 56) - 128;
      P[e] = (int8_t)(v == -128 ? -127 : v);
   }
}

// P as k_embed_keys reads it - the layout of the packed vocabulary (pack_vocabulary, capi_impl.h) without the XOR, because P is signed
// already: tile t (rows 32 t .. 32 t + 31), step s, lane l: bytes [32 s + 16 (l >> 5), + 16) of row 32 t + (l & 31) at
// ((t * 4 + s) * 64 + l) * 16; and bias[i] = 128 * sum_j P[i][j], what d' = d ^ 0x80 leaves out of P.d: z = P.d' + bias.
// |bias| <= 128 * 128 * 127 < 2^21 and |P.d'| <= 128 * 127 * 128 < 2^21.
inline void embed_pack_projection(const int8_t *P, uint8_t *tiles /* [HS_EMBED_P_BYTES] */, int32_t *bias /* [HS_EMBED_BITS] */)
{
   for (int row = 0; row < HS_EMBED_BITS; row++) {
      const int t = row / HS_EMBED_TILE, r = row % HS_EMBED_TILE;
      int32_t sum = 0;
      for (int j = 0; j < HS_EMBED_DIM; j++) {
         const int8_t v = P[(size_t)row * HS_EMBED_DIM + j];
         sum += v;
         const int s = j / 32, h = (j % 32) / 16, lane = r + 32 * h;
         tiles[((size_t)(t * 4 + s) * 64 + (size_t)lane) * 16 + (size_t)(j % 16)] = (uint8_t)v;
      }
      bias[row] = 128 * sum;
   }
}

// ---- the files (little-endian) ----
// Embedding: char magic[8] = "HESAFFE1"; uint32 bits = 64, dim = 128, k, reserved = 0; int8 P[64][128]; int32 tau[k][64]
// Signatures: char magic[8] = "HESAFFS1"; uint32 bits = 64; uint32 count; count x uint64
constexpr size_t HS_EMBED_FILE_HEAD = 24;
constexpr size_t HS_SIGS_FILE_HEAD = 16;
inline uint64_t embed_file_bytes(uint64_t k) { return HS_EMBED_FILE_HEAD + HS_EMBED_P_BYTES + k * (uint64_t)HS_EMBED_BITS * 4u; }
inline uint64_t sigs_file_bytes(uint64_t count) { return HS_SIGS_FILE_HEAD + count * 8u; }
inline void embed_file_head(char *head /* [24] */, uint32_t k)
{
   const uint32_t f[4] = {(uint32_t)HS_EMBED_BITS, (uint32_t)HS_EMBED_DIM, k, 0u};
   memcpy(head, "HESAFFE1", 8);
   memcpy(head + 8, f, 16);
}
// -> k, or -1 where the head is not that of a whole embedding file of `size` bytes
inline int64_t embed_file_rows(const char *head /* [24] */, uint64_t size)
{
   uint32_t f[4];
   if (memcmp(head, "HESAFFE1", 8) != 0) return -1;
   memcpy(f, head + 8, 16);
   if (f[0] != (uint32_t)HS_EMBED_BITS || f[1] != (uint32_t)HS_EMBED_DIM || f[2] < 1u || f[2] > (uint32_t)HS_VOCAB_MAX_ROWS || f[3] != 0u) return -1;
   return size == embed_file_bytes(f[2]) ? (int64_t)f[2] : -1;
}
inline void sigs_file_head(char *head /* [16] */, uint32_t count)
{
   const uint32_t f[2] = {(uint32_t)HS_EMBED_BITS, count};
   memcpy(head, "HESAFFS1", 8);
   memcpy(head + 8, f, 8);
}
// -> count, or -1 where the head is not that of a whole signatures file of `size` bytes
inline int64_t sigs_file_count(const char *head /* [16] */, uint64_t size)
{
   uint32_t f[2];
   if (memcmp(head, "HESAFFS1", 8) != 0) return -1;
   memcpy(f, head + 8, 8);
   if (f[0] != (uint32_t)HS_EMBED_BITS || f[1] > 0x7fffffffu) return -1;
   return size == sigs_file_bytes(f[1]) ? (int64_t)f[1] : -1;
}

// ---- the context's embedding, one buffer ----
struct EmbedArrays {
   Span<uint8_t> tiles;     // [64 * 128]: P as k_embed_keys reads it
   Span<int32_t> bias;      // [64]
   Span<int32_t> tau;       // [k][64]: a word's thresholds are 256 contiguous bytes
};
inline EmbedArrays embed_arrays(StagePlan &p, int64_t k)
{
   EmbedArrays a;
   a.tiles = p.add<uint8_t>(HS_EMBED_P_BYTES);
   a.bias = p.add<int32_t>((size_t)HS_EMBED_BITS);
   a.tau = p.add<int32_t>((size_t)k * HS_EMBED_BITS);
   return a;
}

// ---- the arrays of a threshold training, released before the call returns: the projection alone (tiles, bias), every key's z, the
// grouping of the keys by word (AccumulateArrays without its sums: sub, cursor, perm, block_sums, total, counts) and the result ----
struct EmbedTrainArrays {
   Span<uint8_t> tiles;         // [64 * 128]
   Span<int32_t> bias;          // [64]
   Span<int32_t> z;             // [n][64]
   Span<uint32_t> counts;       // [k]
   Span<uint32_t> sub, cursor;  // [k][slots]
   Span<uint32_t> perm;         // [n]
   Span<uint32_t> block_sums;
   Span<uint32_t> total;
   Span<int32_t> tau;           // [k][64]
   int slots;
};
inline EmbedTrainArrays embed_train_arrays(StagePlan &p, int64_t n, int64_t k)
{
   EmbedTrainArrays t;
   t.slots = accumulate_slots(k);
   const size_t entries = (size_t)k * (size_t)t.slots;
   t.tiles = p.add<uint8_t>(HS_EMBED_P_BYTES);
   t.bias = p.add<int32_t>((size_t)HS_EMBED_BITS);
   t.z = p.add<int32_t>((size_t)n * HS_EMBED_BITS);
   t.counts = p.add<uint32_t>((size_t)k);
   t.sub = p.add<uint32_t>(entries);
   t.cursor = p.add<uint32_t>(entries);
   t.perm = p.add<uint32_t>((size_t)n);
   t.block_sums = p.add<uint32_t>((entries + 4095) / 4096 + 1);
   t.total = p.add<uint32_t>(1);
   t.tau = p.add<int32_t>((size_t)k * HS_EMBED_BITS);
   return t;
}
// (n = 2^24, k = 2^20: 4.6 GB, of which z is 4)
inline size_t embed_train_working_set_bytes(int64_t n, int64_t k)
{
   StagePlan p;
   embed_train_arrays(p, n, k);
   return p.bytes();
}

// ---- the key lists of an embedded index, one buffer beside the plain index's: word-major, structure of arrays, so that a signature
// is one aligned 8-byte load ----
struct KeyListArrays {
   Span<uint32_t> offsets;              // [k + 1]: word w's keys are entries offsets[w] .. offsets[w + 1] - 1
   Span<unsigned long long> sig;        // [total]
   Span<uint32_t> image;                // [total]
};
inline KeyListArrays key_list_arrays(StagePlan &p, int64_t k, int64_t total)
{
   KeyListArrays a;
   a.offsets = p.add<uint32_t>((size_t)k + 1);
   a.sig = p.add<unsigned long long>((size_t)(total > 0 ? total : 1));
   a.image = p.add<uint32_t>((size_t)(total > 0 ? total : 1));
   return a;
}
// the scratch of a key lists' build on its own.  Inside an index build or add the lists are made in that call's scratch instead
// (build_key_lists, capi_index.h): the cursor and the block sums of IndexBuildArrays, index_plan.h, which have these counts
struct KeyListBuildArrays {
   Span<uint32_t> counts;       // [k]: keys per word, then (a copy of the offsets) each list's next free position
   Span<uint32_t> block_sums;   // the scan's
};
inline KeyListBuildArrays key_list_build_arrays(StagePlan &p, int64_t k)
{
   KeyListBuildArrays b;
   b.counts = p.add<uint32_t>((size_t)k);
   b.block_sums = p.add<uint32_t>(((size_t)k + 4095) / 4096 + 1);
   return b;
}

} // namespace hesaff_plan
