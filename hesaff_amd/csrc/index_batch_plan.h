// index_batch_plan.h -- the host arithmetic of a batch of index queries (hesaff_index_query_batch*, include/hesaff_amd.h): which
// batches are refused, how a batch is cut into chunks of consecutive queries, and where the arrays of a chunk lie in the batch scratch.
// Pure functions and plain structs, no HIP, in the manner of index_plan.h: capi_index_batch.h and kernels_index_batch.h obtain their
// numbers here, and tests/native/index_batch_plan_check.cpp checks them on the CPU (tests/test_index_batch_host.py).
#pragma once
#include <cstddef>
#include <cstdint>

#include "index_plan.h"

namespace hesaff_plan {

constexpr int64_t HS_BATCH_MAX_QUERIES = (int64_t)1 << 16;   // a chunk's query number takes the image's place in the hash key: 16 of its 20 bits
// The device scratch a batch may hold unless hesaff_index_set_batch_budget says otherwise.  A design choice, not a measured optimum:
// large enough that 1000 queries against 100 000 images are one chunk (16 bytes per query and image), small beside the device's memory.
constexpr size_t HS_BATCH_DEFAULT_BUDGET = (size_t)1 << 30;

inline bool index_batch_ok(int64_t n_queries, int64_t top) { return n_queries >= 1 && n_queries <= HS_BATCH_MAX_QUERIES && top >= 1 && top <= HS_INDEX_MAX_TOP; }
// counts[n_queries] -> the words of the batch, or -1 where a query or the sum is out of bounds (a query's bound is an image's, the
// sum's is a build's)
inline int64_t index_batch_total(const int32_t *counts, int64_t n_queries) { return index_total_keys(counts, n_queries); }
inline size_t index_batch_budget(size_t set) { return set ? set : HS_BATCH_DEFAULT_BUDGET; }

// ---- the scratch of a chunk: b queries of `words` words in all against n_images images, keep = min(top, n_images) ranked per query.
// dot, heads and hash_tf are consecutive, so one memset zeroes what a chunk needs zero (zero_off, zero_bytes).  The ranked rows are
// one block - b * keep scores, then b * keep images - so one copy of b * keep * 12 bytes brings them to the host. ----
struct IndexBatchArrays {
   Span<unsigned long long> dot;         // [b][n_images]
   Span<IndexResultHead> heads;          // [b]
   Span<uint32_t> hash_tf;               // [slots]: the count of each distinct (query, word); exchanged for 0 by the scoring
   Span<unsigned long long> hash_keys;   // [slots]: HS_INDEX_EMPTY or index_key(query in chunk, word)
   Span<double> score;                   // [b][n_images]
   Span<char> ranked;                    // double [b][keep], then int32 [b][keep]
   size_t ranked_images_off;             // the images' byte offset in the scratch
   size_t zero_off, zero_bytes;
   uint64_t slots;
   int bits;
};
inline size_t index_batch_ranked_bytes(int64_t b, int64_t keep) { return (size_t)b * (size_t)keep * 12; }
inline IndexBatchArrays index_batch_arrays(StagePlan &p, int64_t b, int64_t n_images, int64_t keep, int64_t words)
{
   IndexBatchArrays a;
   a.bits = index_hash_bits(words);
   a.slots = (uint64_t)1 << a.bits;
   a.dot = p.add<unsigned long long>((size_t)b * (size_t)n_images);
   a.heads = p.add<IndexResultHead>((size_t)b);
   a.hash_tf = p.add<uint32_t>((size_t)a.slots);
   a.zero_off = a.dot.off;
   a.zero_bytes = p.bytes() - a.dot.off;
   a.hash_keys = p.add<unsigned long long>((size_t)a.slots);
   a.score = p.add<double>((size_t)b * (size_t)n_images);
   a.ranked = p.add<char>(index_batch_ranked_bytes(b, keep));
   a.ranked_images_off = a.ranked.off + (size_t)b * (size_t)keep * 8;
   return a;
}
inline size_t index_batch_chunk_bytes(int64_t b, int64_t n_images, int64_t keep, int64_t words)
{
   StagePlan p;
   index_batch_arrays(p, b, n_images, keep, words);
   return p.bytes();
}

// ---- the chunk rule: from query `first` on, the longest run of consecutive queries whose scratch fits the budget; one query is always
// allowed.  (The bytes do not fall when a query joins: every array grows with b or with the words.) ----
struct IndexBatchChunk {
   int64_t first, count;        // queries first .. first + count - 1
   int64_t word_first, words;   // their words in the batch's concatenation
   size_t bytes;                // index_batch_chunk_bytes of the chunk
};
inline IndexBatchChunk index_batch_next_chunk(const int32_t *counts, int64_t n_queries, int64_t first, int64_t word_first, int64_t n_images, int64_t keep,
                                              size_t budget)
{
   IndexBatchChunk c;
   c.first = first; c.count = 1; c.word_first = word_first; c.words = counts[first];
   c.bytes = index_batch_chunk_bytes(1, n_images, keep, c.words);
   while (first + c.count < n_queries) {
      const int64_t words = c.words + counts[first + c.count];
      const size_t bytes = index_batch_chunk_bytes(c.count + 1, n_images, keep, words);
      if (bytes > budget) break;
      c.count++; c.words = words; c.bytes = bytes;
   }
   return c;
}
// the number of chunks of a batch (arguments inside their bounds), and the largest chunk's bytes
inline int64_t index_batch_chunks(const int32_t *counts, int64_t n_queries, int64_t n_images, int64_t keep, size_t budget, size_t *max_bytes = nullptr)
{
   int64_t n = 0, first = 0, word_first = 0;
   size_t most = 0;
   while (first < n_queries) {
      const IndexBatchChunk c = index_batch_next_chunk(counts, n_queries, first, word_first, n_images, keep, budget);
      first += c.count; word_first += c.words;
      if (c.bytes > most) most = c.bytes;
      n++;
   }
   if (max_bytes) *max_bytes = most;
   return n;
}

} // namespace hesaff_plan
