// index_batch_plan_check.cpp -- the host arithmetic of batched index queries (hesaff_amd/csrc/index_batch_plan.h) on the CPU: the
// bounds of a batch on both sides, the chunk rule (chunks non-empty, consecutive, covering; a chunk of several queries inside the
// budget; one query always a chunk), the layout of a chunk's scratch (disjoint, aligned, inside its bytes) and the sizes at the
// largest case checked in 128 bits.  tests/test_index_batch_host.py builds it with AddressSanitizer + UBSan and runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../hesaff_amd/csrc/index_batch_plan.h"

using namespace hesaff_plan;

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

typedef unsigned __int128 u128;

static void check_bounds()
{
   const int64_t Q = (int64_t)1 << 16, C = (int64_t)1 << 18, T = (int64_t)1 << 28;
   CHECK(index_batch_ok(1, 1) && index_batch_ok(Q, 1024), "the smallest and the largest batch");
   CHECK(!index_batch_ok(0, 1) && !index_batch_ok(-1, 1) && !index_batch_ok(Q + 1, 1), "Q outside 1 .. 2^16");
   CHECK(!index_batch_ok(1, 0) && !index_batch_ok(1, -1) && !index_batch_ok(1, 1025), "top outside 1 .. 1024");
   const int32_t ok[3] = {0, (int32_t)C, 5}, over[2] = {3, (int32_t)C + 1}, neg[2] = {4, -1}, none[1] = {0};
   CHECK(index_batch_total(ok, 3) == C + 5 && index_batch_total(none, 1) == 0, "counts 0 and 2^18");
   CHECK(index_batch_total(over, 2) == -1 && index_batch_total(neg, 2) == -1, "a count outside 0 .. 2^18");
   std::vector<int32_t> full(1025, (int32_t)C);   // 1024 x 2^18 = 2^28 words: the largest batch; one query more is refused
   CHECK(index_batch_total(full.data(), 1024) == T && index_batch_total(full.data(), 1025) == -1, "2^28 words and 2^28 + 2^18");
   std::vector<int32_t> many((size_t)Q, 4096);    // 2^16 queries of 2^12 words: 2^28 as well
   CHECK(index_batch_total(many.data(), Q) == T, "2^16 queries");
   many[7] += 1;
   CHECK(index_batch_total(many.data(), Q) == -1, "2^28 + 1 words");
   CHECK(index_batch_budget(0) == HS_BATCH_DEFAULT_BUDGET && index_batch_budget(1) == 1 && index_batch_budget((size_t)5 << 30) == ((size_t)5 << 30), "0 is the default");
   CHECK(HS_BATCH_MAX_QUERIES <= HS_INDEX_MAX_IMAGES, "a chunk's query number fits the image bits of the hash key");
}

// the arrays of a chunk: inside the bytes, 256-byte aligned, disjoint, in the order the zeroing relies on; the sizes against 128 bits
static void check_layout(int64_t b, int64_t n_images, int64_t keep, int64_t words)
{
   StagePlan p;
   const IndexBatchArrays a = index_batch_arrays(p, b, n_images, keep, words);
   const size_t bytes = p.bytes();
   CHECK(bytes == index_batch_chunk_bytes(b, n_images, keep, words), "one function, one size");
   CHECK(a.slots >= 1024 && a.slots >= 2 * (uint64_t)words && (a.slots & (a.slots - 1)) == 0 && a.slots == (uint64_t)1 << a.bits, "the table: %llu slots for %lld words",
         (unsigned long long)a.slots, (long long)words);
   CHECK(a.slots < 4 * (uint64_t)(words > 256 ? words : 256) + 1, "the table is not larger than it must be");
   struct Block { size_t off, bytes; const char *name; };
   const Block blocks[6] = {{a.dot.off, a.dot.bytes(), "dot"},       {a.heads.off, a.heads.bytes(), "heads"}, {a.hash_tf.off, a.hash_tf.bytes(), "hash_tf"},
                            {a.hash_keys.off, a.hash_keys.bytes(), "hash_keys"}, {a.score.off, a.score.bytes(), "score"}, {a.ranked.off, a.ranked.bytes(), "ranked"}};
   const u128 want[6] = {(u128)b * n_images * 8, (u128)b * 16, (u128)a.slots * 4, (u128)a.slots * 8, (u128)b * n_images * 8, (u128)b * keep * 12};
   size_t end = 0;
   for (int i = 0; i < 6; i++) {
      CHECK((u128)blocks[i].bytes == want[i], "%s: its bytes in 128 bits", blocks[i].name);
      CHECK(blocks[i].off % 256 == 0, "%s is 256-byte aligned", blocks[i].name);
      CHECK(blocks[i].off >= end, "%s begins behind the array before it", blocks[i].name);
      CHECK(blocks[i].off + blocks[i].bytes <= bytes, "%s lies inside the scratch", blocks[i].name);
      end = blocks[i].off + blocks[i].bytes;
   }
   CHECK(a.zero_off == a.dot.off && a.zero_off + a.zero_bytes == a.hash_tf.off + a.hash_tf.bytes(), "one memset zeroes dot, the heads and the counts ...");
   CHECK(a.zero_off + a.zero_bytes <= a.hash_keys.off, "... and stops before the keys");
   CHECK(a.ranked_images_off == a.ranked.off + (size_t)b * (size_t)keep * 8 && a.ranked_images_off % 4 == 0 && a.ranked.off % 8 == 0, "the ranked images behind the ranked scores");
   CHECK(a.ranked.bytes() == index_batch_ranked_bytes(b, keep), "one copy of b x keep x 12 bytes");
}

// the chunks of a batch: non-empty, consecutive, covering; several queries only inside the budget; the rule is greedy (the next
// query would not have fitted)
static int64_t check_chunks(const std::vector<int32_t> &counts, int64_t n_images, int64_t keep, size_t budget)
{
   const int64_t nq = (int64_t)counts.size();
   int64_t first = 0, word_first = 0, n = 0;
   size_t most = 0;
   while (first < nq) {
      const IndexBatchChunk c = index_batch_next_chunk(counts.data(), nq, first, word_first, n_images, keep, budget);
      CHECK(c.count >= 1 && c.first == first && c.word_first == word_first && first + c.count <= nq, "chunk %lld is non-empty and consecutive", (long long)n);
      int64_t words = 0;
      for (int64_t q = 0; q < c.count; q++) words += counts[(size_t)(first + q)];
      CHECK(c.words == words, "chunk %lld: its words", (long long)n);
      CHECK(c.bytes == index_batch_chunk_bytes(c.count, n_images, keep, c.words), "chunk %lld: its bytes", (long long)n);
      CHECK(c.count == 1 || c.bytes <= budget, "chunk %lld of %lld queries fits the budget", (long long)n, (long long)c.count);
      if (first + c.count < nq)
         CHECK(index_batch_chunk_bytes(c.count + 1, n_images, keep, c.words + counts[(size_t)(first + c.count)]) > budget, "chunk %lld is the longest run", (long long)n);
      if (c.bytes > most) most = c.bytes;
      first += c.count; word_first += c.words;
      n++;
   }
   CHECK(first == nq, "the chunks cover the batch");
   size_t reported = 0;
   CHECK(index_batch_chunks(counts.data(), nq, n_images, keep, budget, &reported) == n && reported == most, "index_batch_chunks agrees");
   return n;
}

int main()
{
   check_bounds();
   // layouts: the smallest, around the smallest table, odd sizes, and the largest sizes of every kind
   const int64_t C = (int64_t)1 << 18, N = (int64_t)1 << 20;
   check_layout(1, 1, 1, 0);
   check_layout(1, 1, 1, 1);
   for (int64_t words : {511, 512, 513}) check_layout(2, 3, 3, words);
   check_layout(67, 1025, 1024, 4099);
   check_layout(1, N, 1024, C);                             // one query of 2^18 words against 2^20 images
   check_layout(64, N, 1024, 64 * C);                       // 1 GiB of rows
   check_layout((int64_t)1 << 16, N, 1024, (int64_t)1 << 28);   // everything at its bound: 2^37-byte rows, no wrap in size_t
   CHECK(sizeof(size_t) >= 8, "the sizes above need a 64-bit size_t");
   // the bytes do not fall when a query joins
   for (int64_t b = 1; b < 40; b++)
      CHECK(index_batch_chunk_bytes(b + 1, 257, 10, 100 * b + 100) >= index_batch_chunk_bytes(b, 257, 10, 100 * b), "monotone at b = %lld", (long long)b);
   // chunks
   std::vector<int32_t> one = {5}, two = {0, 7}, small(67);
   for (size_t q = 0; q < small.size(); q++) small[q] = (int32_t)(q % 8);
   const size_t b1 = index_batch_chunk_bytes(1, 257, 10, 0), b2 = index_batch_chunk_bytes(2, 257, 10, 0), b5 = index_batch_chunk_bytes(5, 257, 10, 0);
   CHECK(check_chunks(one, 257, 10, HS_BATCH_DEFAULT_BUDGET) == 1 && check_chunks(one, 257, 10, 1) == 1, "Q = 1");
   CHECK(check_chunks(two, 257, 10, HS_BATCH_DEFAULT_BUDGET) == 1 && check_chunks(two, 257, 10, 1) == 2 && check_chunks(two, 257, 10, b2) == 1 &&
         check_chunks(two, 257, 10, b2 - 1) == 2, "Q = 2 on both sides of its size");
   CHECK(check_chunks(small, 257, 10, 1) == 67 && check_chunks(small, 257, 10, b1) == 67, "a budget too small for two queries: one query per chunk");
   CHECK(check_chunks(small, 257, 10, 0) == 67, "a budget of no bytes still yields one-query chunks");
   CHECK(check_chunks(small, 257, 10, b2) == 34 && check_chunks(small, 257, 10, b5) == 14 && check_chunks(small, 257, 10, HS_BATCH_DEFAULT_BUDGET) == 1, "chunks of 2, of 5, of all");
   // a query of 2^18 words in the middle widens its chunk's table: the chunks before and behind it stay small
   std::vector<int32_t> mixed = {3, 4, (int32_t)C, 0, 5, 6};
   CHECK(check_chunks(mixed, 1025, 1024, index_batch_chunk_bytes(2, 1025, 1024, 7)) == 4, "{3, 4} {2^18} {0, 5} {6}");
   // the bounds: 2^16 queries; 2^28 words; N = 2^20 with 2^18-word queries at the default budget (one query needs 16 MiB of rows and
   // 6 MiB of table), and at a budget below one query
   std::vector<int32_t> many((size_t)1 << 16, 4096), big(1024, (int32_t)C);
   CHECK(check_chunks(many, 1000, 10, HS_BATCH_DEFAULT_BUDGET) >= 2, "2^16 queries of 2^12 words");
   CHECK(check_chunks(many, 1, 1, ~(size_t)0) == 1, "2^16 queries, no budget to speak of: one chunk of 2^28 words");
   const int64_t at_default = check_chunks(big, N, 1024, HS_BATCH_DEFAULT_BUDGET);
   CHECK(at_default >= 1024 / 64 && at_default <= 1024 / 16, "N = 2^20, 2^18-word queries, 1 GiB: %lld chunks", (long long)at_default);
   CHECK(check_chunks(big, N, 1024, 1 << 20) == 1024, "N = 2^20, 1 MiB: one query per chunk");
   if (g_failed) {
      fprintf(stderr, "index_batch_plan_check: %d checks failed\n", g_failed);
      return 1;
   }
   printf("index_batch_plan_check ok\n");
   return 0;
}
