// kernels_neighbours.h -- vocabulary neighbours (hesaff_set_vocabulary_neighbours, include/hesaff_amd.h): for every key the R
// lexicographically least pairs (dist2(k), k) over the rows of the vocabulary, ascending, in ONE pass over the vocabulary.  Rank 0 is
// what k_assign_words (kernels_words.h) gives, bit for bit: the same integers, the same order.
//
// k_assign_neighbours is the frame of kernels_words.h - keys and stream - with another memory.  k_assign_words keeps a running best
// per accumulator ELEMENT (2 x 16 x 2 registers); R of them per element would be 64 R registers.  Here a lane keeps, per key tile, ONE
// list of CAP >= R pairs (score, k) sorted ascending - 2 x 2 x CAP registers, 32 at CAP = 8 - over all the rows it sees: 16 of every
// tile.  A key's rows are split between lanes l and l ^ 32, so its R least pairs lie in the union of the two lists' first R entries;
// the last step merges them across the halves.
//
// The visit pays one compare per element, score <= the score of the list's last entry.  Only where it fires is the pair decided
// exactly - rows do NOT reach a lane in ascending k (within a tile they come in element order, and the order of insertion is free
// anyway), so a tie in score is decided by k, never by strict < - and inserted by CAP compare-and-shift steps with static indices.  A
// list keeps CAP entries even where R < CAP: the surplus entries are candidates that cannot be wrong, and only the first R are written.
// Once the lists are warm an insertion is rare (the expected count per list grows like CAP ln(tiles)), so the loop runs at little
// more than k_assign_words' pace.
//
// Pad rows (norm 2^30, score exactly 2^30 since their bytes are zero) enter a list only while it holds fewer than CAP real rows, and
// never displace one: a real score is below 2^23.  They and the untouched slots (0x7fffffff) come out as (-1, 2^31 - 1).  No row is
// seen twice - every (tile, row) is one element of one lane - so the rows of a key's list are distinct.
#pragma once
#include "kernels_words.h"

#define HS_NEIGH_MAX 8                  // the largest R (and the largest list)
#define HS_NEIGH_NONE_DIST 0x7fffffff   // dist2 of a rank that does not exist (K < R); its word is -1

// (s, k) into the sorted list ls / lk: the entries behind its place move down one, the last falls out
template <int CAP>
__device__ __forceinline__ void hs_neigh_insert(int (&ls)[CAP], int (&lk)[CAP], int s, int k)
{
   const auto before = [&](int i) { return s < ls[i] || (s == ls[i] && k < lk[i]); };
#pragma unroll
   for (int i = CAP - 1; i > 0; i--) {   // (entry i - 1 is still the old one when entry i is decided)
      const bool before_prev = before(i - 1), before_this = before(i);
      ls[i] = before_prev ? ls[i - 1] : (before_this ? s : ls[i]);
      lk[i] = before_prev ? lk[i - 1] : (before_this ? k : lk[i]);
   }
   const bool first = before(0);
   ls[0] = first ? s : ls[0];
   lk[0] = first ? k : lk[0];
}

// desc, n, stride, offset, tiles, norms, n_tiles: as for k_assign_words.  1 <= R <= CAP.  out: int32[n][R][2], (word, dist2) per rank.
// words: nullptr, or int32[n][2] that receives rank 0 as well (the (word, dist2) array of the entry points that hand one out).
template <int CAP>
__global__ __launch_bounds__(HS_WORD_BLOCK_WAVES * 64) void k_assign_neighbours(const uint8_t *__restrict__ desc, long long n, long long stride, long long offset,
                                                                               const hs_v4i *__restrict__ tiles, const int32_t *__restrict__ norms, int n_tiles,
                                                                               int R, int32_t *__restrict__ out, int32_t *__restrict__ words)
{
   const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
   const int r = lane & 31, h = lane >> 5;
   const long long key0 = ((long long)blockIdx.x * HS_WORD_BLOCK_WAVES + wave) * HS_WORD_WAVE_KEYS;
   if (key0 >= n) return;   // (wave-uniform)

   // a lane beyond the last key reads the last key again and stores nothing
   hs_v4i kf[2][4];
   int knorm[2];
   int ls[2][CAP], lk[2][CAP];
#pragma unroll
   for (int j = 0; j < 2; j++) {
      hs_key_load(desc, min(key0 + 32 * j + r, n - 1), stride, offset, h, kf[j]);
      knorm[j] = hs_key_norm(kf[j]);
#pragma unroll
      for (int i = 0; i < CAP; i++) { ls[j][i] = 0x7fffffff; lk[j][i] = 0x7fffffff; }
   }

   hs_word_stream(tiles, norms, 0, n_tiles - 1, lane, kf, [&](int t, int j, int (&score)[16]) {
#pragma unroll
      for (int e = 0; e < 16; e++)
         if (score[e] <= ls[j][CAP - 1])   // rare once the list is warm; the exact decision, by (score, k), is the insertion's
            hs_neigh_insert<CAP>(ls[j], lk[j], score[e], t * HS_WORD_TILE + hs_word_row(e, h));
   });

#pragma unroll
   for (int j = 0; j < 2; j++) {
      // the other half's list (all lanes take part in the exchange), merged into the lane's own: both halves end with the key's list
      int os[CAP], ok[CAP];
#pragma unroll
      for (int i = 0; i < CAP; i++) { os[i] = __shfl_xor(ls[j][i], 32, 64); ok[i] = __shfl_xor(lk[j][i], 32, 64); }
#pragma unroll
      for (int i = 0; i < CAP; i++) hs_neigh_insert<CAP>(ls[j], lk[j], os[i], ok[i]);
      const long long key = key0 + 32 * j + r;
      if (h == 0 && key < n) {
#pragma unroll
         for (int i = 0; i < CAP; i++) {
            if (i >= R) break;
            const bool real = ls[j][i] < HS_WORD_PAD_NORM;   // a pad row or an empty slot: fewer than i + 1 real rows exist
            const int w = real ? lk[j][i] : -1, d2 = real ? ls[j][i] + knorm[j] : HS_NEIGH_NONE_DIST;
            out[(key * R + i) * 2] = w;
            out[(key * R + i) * 2 + 1] = d2;
            if (i == 0 && words) { words[2 * key] = w; words[2 * key + 1] = d2; }
         }
      }
   }
}
