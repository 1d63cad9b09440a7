// train_plan.h -- the host arithmetic of vocabulary training (hesaff_train_vocabulary, include/hesaff_amd.h): which calls are refused,
// the sampling rule of a call without an initial vocabulary, the update rule of a word, and where the arrays of a call lie in its
// working buffer.  Pure functions and plain structs, no HIP: capi_impl.h and kernels_train.h obtain their numbers here, and
// tests/native/train_plan_check.cpp checks them on the CPU (tests/test_vocabulary_training_host.py).
#pragma once
#include <cstddef>
#include <cstdint>

#include "buffer_layouts.h"   // StagePlan, Span

#if defined(__HIPCC__)
#define HS_TRAIN_HD __host__ __device__ __forceinline__
#else
#define HS_TRAIN_HD inline
#endif

namespace hesaff_plan {

constexpr int64_t HS_TRAIN_MAX_KEYS = (int64_t)1 << 24;   // sums are uint32: 2^24 * 255 < 2^32
constexpr int64_t HS_VOCAB_MAX_ROWS = (int64_t)1 << 20;   // hesaff_set_vocabulary's bound
constexpr int HS_TRAIN_TILE = 32;                         // rows per tile of the packed vocabulary (HS_WORD_TILE, kernels_words.h)

// n keys into k words: the bounds of the accumulation (hesaff_stage_accumulate_words) and of a training call
inline bool accumulate_counts_ok(int64_t n, int64_t k) { return n >= 1 && n <= HS_TRAIN_MAX_KEYS && k >= 1 && k <= HS_VOCAB_MAX_ROWS; }
// ... and the rest of a training call: at least one iteration, and without an initial vocabulary a key for every row to be sampled
inline bool train_counts_ok(int64_t n, int64_t k, int64_t iterations, bool has_init)
{
   return accumulate_counts_ok(n, k) && iterations >= 1 && (has_init || n >= k);
}
// descriptor i is the 128 bytes at base + i * stride + offset, read as aligned dwords (hesaff_assign_words_device's rule)
inline bool word_source_ok(int64_t stride, int64_t offset)
{
   return stride >= 128 && offset >= 0 && offset <= stride - 128 && stride % 4 == 0 && offset % 4 == 0;
}

// row `row` of a sampled initial vocabulary is key floor(row * n / k), the product in 64 bits (row < k <= 2^20, n <= 2^24: below 2^44)
HS_TRAIN_HD int64_t train_sample_index(int64_t row, int64_t n, int64_t k) { return (int64_t)((uint64_t)row * (uint64_t)n / (uint64_t)k); }

// the mean sum / count rounded half up, count > 0, evaluated in 64 bits (2 sum + count may reach 2^33): for bytes summed over `count`
// keys the result is a byte, and it is the integer that minimises sum_i (d_i - v)^2
HS_TRAIN_HD uint32_t train_rounded_mean(uint32_t sum, uint32_t count) { return (uint32_t)((2 * (uint64_t)sum + count) / (2 * (uint64_t)count)); }

// what the host reads back after an iteration, in one copy
struct TrainStats {
   long long distortion;   // sum of dist2 over the keys, under the vocabulary the iteration started from
   uint32_t empty;         // words without a key
   uint32_t changed;       // rows the update changed
};
static_assert(sizeof(TrainStats) == 16, "one 16-byte copy");

// The arrays of a call in the context's training buffer, each 256-byte aligned.  The accumulation alone (sums .. block_sums) is what
// hesaff_stage_accumulate_words needs beside the caller's keys and words; a training call adds its private vocabulary and the
// assignment's rows.
struct AccumulateArrays {
   Span<uint32_t> sums;         // [k][128]
   Span<uint32_t> counts;       // [k]
   Span<uint32_t> sub;          // [k][slots]: the keys of word k counted by the waves with wave index % slots == slot
   Span<uint32_t> cursor;       // [k][slots]: the scan of sub, then each entry's next free position
   Span<uint32_t> perm;         // [n]: the key indices grouped by word
   Span<uint32_t> block_sums;   // the scan's, one per 4096 entries and one more
   Span<TrainStats> stats;
   Span<uint32_t> total;        // the scan's total (n)
   int slots;                   // accumulate_slots(k)
   int chunks;                  // accumulate_chunks(n)
};
// Launch geometry of the accumulation, which no result depends on.  A word's counter is split into `slots` sub-counters, taken by the
// waves in turn: with few words every wave holds every word, and n / 64 atomics on each of K neighbouring counters would queue up in
// one or two cache lines (K = 33: 20 ms for 3.78 M keys).  A power of two, 64 at most, with k * slots <= 8192 where that is possible.
inline int accumulate_slots(int64_t k)
{
   int s = 1;
   while (s < 64 && 2 * (int64_t)s * k <= 8192) s *= 2;
   return s;
}
// A half-wave of k_accumulate_words walks `chunks` x 32 consecutive positions of perm before it flushes: the longer its walk, the
// fewer additions a word with many keys receives (K = 1 at 32 positions: n / 32 x 128 atomics on 128 addresses, 10 ms for 3.78 M keys).
inline int accumulate_chunks(int64_t n) { return (int)(n < 4096 ? 1 : (n >= 16384 ? 8 : n / 2048)); }
inline AccumulateArrays accumulate_arrays(StagePlan &p, int64_t n, int64_t k)
{
   AccumulateArrays a;
   a.slots = accumulate_slots(k);
   a.chunks = accumulate_chunks(n);
   const size_t entries = (size_t)k * (size_t)a.slots;
   a.sums = p.add<uint32_t>((size_t)k * 128);
   a.counts = p.add<uint32_t>((size_t)k);
   a.sub = p.add<uint32_t>(entries);
   a.cursor = p.add<uint32_t>(entries);
   a.perm = p.add<uint32_t>((size_t)n);
   a.block_sums = p.add<uint32_t>((entries + 4095) / 4096 + 1);
   a.stats = p.add<TrainStats>(1);
   a.total = p.add<uint32_t>(1);
   return a;
}
struct TrainArrays {
   AccumulateArrays acc;
   Span<uint8_t> rows;          // [k][128]: the vocabulary as the caller sees it
   Span<uint8_t> tiles;         // the vocabulary as k_assign_words reads it: whole tiles of 32 rows ...
   Span<int32_t> norms;         // ... and |w'|^2 per row of them
   Span<int32_t> assigned;      // [n][2]: (word, dist2)
   int n_tiles;
};
inline TrainArrays train_arrays(StagePlan &p, int64_t n, int64_t k)
{
   TrainArrays t;
   t.acc = accumulate_arrays(p, n, k);
   t.n_tiles = (int)((k + HS_TRAIN_TILE - 1) / HS_TRAIN_TILE);
   t.rows = p.add<uint8_t>((size_t)k * 128);
   t.tiles = p.add<uint8_t>((size_t)t.n_tiles * HS_TRAIN_TILE * 128);
   t.norms = p.add<int32_t>((size_t)t.n_tiles * HS_TRAIN_TILE);
   t.assigned = p.add<int32_t>((size_t)n * 2);
   return t;
}
// the bytes of a training call's working set (n = 2^24, k = 2^20: 972 MB, of which the sums are 512)
inline size_t train_working_set_bytes(int64_t n, int64_t k)
{
   StagePlan p;
   train_arrays(p, n, k);
   return p.bytes();
}

} // namespace hesaff_plan
