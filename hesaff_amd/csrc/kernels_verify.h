// kernels_verify.h -- spatial verification (hesaff_verify_matches of include/hesaff_amd.h): the candidates of a tf-idf shortlist ranked by
// how many tentative correspondences agree with the best single-correspondence affine hypothesis.  Every accumulation is an integer
// count and every float is made by the same operations in the same order for whichever thread makes it, so no result depends on the
// launch geometry, on the tiling or on the order of atomics.
//
// Pairs.  k_verify_query_count adds the live query keys into tfq[word]; exclusive_scan (pipeline.hip) turns tfq into the group
// offsets, k_verify_query_scatter writes every live key's index into its word's group in the order of arrival, and k_verify_sort_groups
// puts the groups of at most HS_VERIFY_MAX_PAIRS keys - the only ones ever read - into ascending order.  k_verify_insert counts
// tf_r(w) over the live keys of every candidate in the open-addressing table of the index build (index_plan.h: the key is
// candidate << 20 | word), for the words a pair can come from (1 <= tfq(w) <= P) only, and counts the inert keys.  k_verify_pairs runs
// one block per candidate: it walks the candidate's keys in j order, 256 at a time, scans the per-key pair counts (tfq(w) where
// tfq(w) tf_r(w) <= P, else 0), and writes the pairs whose position in the (j, i) order is below 4096 - as (i, j) and as the ten
// floats the hypothesis kernel reads - and the total, found_r.
//
// Hypotheses.  k_verify_hypotheses runs one candidate and HS_VERIFY_TILE hypotheses per block, one hypothesis per lane: L11, L21, L22
// and the lane's own four coordinates stay in registers, the candidate's used correspondences pass through LDS HS_VERIFY_CHUNK at a
// time as (xq, yq, xd, yd), and every lane of a wave reads the same LDS address per step - a broadcast, no bank conflicts, no memory
// traffic in the loop.  The best hypothesis is the maximum of (inl << 32 | ~h) over h: a wave reduction and one atomicMax per wave.
// k_verify_finish writes out, hyp and the ranking (R <= 1024 values: one block, ranked by counting).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "verify_plan.h"

using hesaff_plan::VerifyRow;

#define HS_VERIFY_TILE 256     // hypotheses of a block
#define HS_VERIFY_CHUNK 1024   // correspondences in LDS at a time: 16 KB

// tfq[word] += 1 per live query key (zeroed by the caller); *inert += the others.  Grid: ceil(nq / 256).
__global__ __launch_bounds__(256) void k_verify_query_count(const VerifyRow *__restrict__ rows, int nq, uint32_t *__restrict__ tfq, uint32_t *__restrict__ inert)
{
   const int i = (int)(blockIdx.x * 256u + threadIdx.x);
   bool dead = false;
   if (i < nq) {
      const VerifyRow k = rows[i];
      if (hesaff_plan::verify_frame(k.x, k.y, k.a, k.b, k.c).live) atomicAdd(&tfq[k.word], 1u);
      else dead = true;
   }
   const unsigned long long m = __ballot(dead);
   if (m != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(inert, (uint32_t)__popcll(m));
}

// members[cursor[word]++] = i per live query key; cursor: a copy of the offsets on entry.  Grid: ceil(nq / 256).
__global__ __launch_bounds__(256) void k_verify_query_scatter(const VerifyRow *__restrict__ rows, int nq, uint32_t *__restrict__ cursor, uint32_t *__restrict__ members)
{
   const int i = (int)(blockIdx.x * 256u + threadIdx.x);
   if (i >= nq) return;
   const VerifyRow k = rows[i];
   if (hesaff_plan::verify_frame(k.x, k.y, k.a, k.b, k.c).live) members[atomicAdd(&cursor[k.word], 1u)] = (uint32_t)i;
}

// the groups of 2 .. HS_VERIFY_MAX_PAIRS keys in ascending order (insertion sort, one thread per word).  Grid: ceil(k / 256).
__global__ __launch_bounds__(256) void k_verify_sort_groups(const uint32_t *__restrict__ offsets, int k, uint32_t *__restrict__ members)
{
   const int w = (int)(blockIdx.x * 256u + threadIdx.x);
   if (w >= k) return;
   const uint32_t lo = offsets[w], g = offsets[w + 1] - lo;
   if (g < 2u || g > (uint32_t)hesaff_plan::HS_VERIFY_MAX_PAIRS) return;
   for (uint32_t a = 1; a < g; a++) {
      const uint32_t v = members[lo + a];
      uint32_t b = a;
      while (b > 0u && members[lo + b - 1u] > v) { members[lo + b] = members[lo + b - 1u]; b--; }
      members[lo + b] = v;
   }
}

// the candidate of key j: the r with starts[r] <= j < starts[r + 1] (candidates without keys repeat a start and are never found)
__device__ __forceinline__ uint32_t hs_verify_candidate_of(const uint32_t *__restrict__ starts, int n_candidates, uint32_t j)
{
   uint32_t lo = 0, hi = (uint32_t)n_candidates;   // starts[lo] <= j < starts[hi]
   while (hi - lo > 1u) {
      const uint32_t mid = (lo + hi) >> 1;
      if (starts[mid] <= j) lo = mid; else hi = mid;
   }
   return lo;
}

// Every live candidate key whose word has 1 <= tfq <= P into the table (hash_keys all-ones, hash_tf zero on entry; slots >= 2 T, so a
// probe always meets an empty slot); inert[r] += 1 per key that is not live.  Grid: ceil(total / 256).
__global__ __launch_bounds__(256) void k_verify_insert(const VerifyRow *__restrict__ rows, const uint32_t *__restrict__ starts, int n_candidates, uint32_t total,
                                                       const uint32_t *__restrict__ tfq, int max_pairs, int bits, unsigned long long *__restrict__ hash_keys,
                                                       uint32_t *__restrict__ hash_tf, uint32_t *__restrict__ inert)
{
   const uint32_t j = blockIdx.x * 256u + threadIdx.x;
   if (j >= total) return;
   const VerifyRow k = rows[j];
   const uint32_t r = hs_verify_candidate_of(starts, n_candidates, j);
   if (!hesaff_plan::verify_frame(k.x, k.y, k.a, k.b, k.c).live) { atomicAdd(&inert[r], 1u); return; }
   const uint32_t g = tfq[k.word];
   if (g < 1u || g > (uint32_t)max_pairs) return;
   const unsigned long long key = hesaff_plan::index_key(r, k.word);
   const unsigned long long mask = (1ull << bits) - 1ull;
   unsigned long long slot = hesaff_plan::index_hash_slot(key, bits);
   for (;;) {
      const unsigned long long seen = atomicCAS(&hash_keys[slot], (unsigned long long)hesaff_plan::HS_INDEX_EMPTY, key);
      if (seen == hesaff_plan::HS_INDEX_EMPTY || seen == key) break;
      slot = (slot + 1ull) & mask;
   }
   atomicAdd(&hash_tf[slot], 1u);
}

// One block per candidate.  pairs[r][4096][2] = (i, j) and corr[r][4096][10] of the used correspondences, found[r], used[r].
__global__ __launch_bounds__(256) void k_verify_pairs(const VerifyRow *__restrict__ qrows, const VerifyRow *__restrict__ crows, const uint32_t *__restrict__ starts,
                                                      const uint32_t *__restrict__ tfq, const uint32_t *__restrict__ offsets, const uint32_t *__restrict__ members,
                                                      int max_pairs, int bits, const unsigned long long *__restrict__ hash_keys, const uint32_t *__restrict__ hash_tf,
                                                      int32_t *__restrict__ pairs, float *__restrict__ corr, uint32_t *__restrict__ found, uint32_t *__restrict__ used)
{
   __shared__ uint32_t s_wsum[4];
   const uint32_t r = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
   const uint32_t j0 = starts[r], n = starts[r + 1] - j0;
   const unsigned long long mask = (1ull << bits) - 1ull;
   const uint32_t cap = (uint32_t)hesaff_plan::HS_VERIFY_MAX_USED;
   int32_t *const my_pairs = pairs + (size_t)r * cap * 2;
   float *const my_corr = corr + (size_t)r * cap * hesaff_plan::HS_VERIFY_PAIR_FLOATS;
   uint32_t base = 0;   // pairs of the keys before this chunk (block-uniform)
   for (uint32_t c0 = 0; c0 < n; c0 += 256u) {
      const uint32_t jl = c0 + tid;
      uint32_t cnt = 0, word = 0;
      hesaff_plan::VerifyFrame fd = {};
      if (jl < n) {
         const VerifyRow k = crows[(size_t)j0 + jl];
         fd = hesaff_plan::verify_frame(k.x, k.y, k.a, k.b, k.c);
         word = k.word;
         const uint32_t g = fd.live ? tfq[word] : 0u;
         if (g >= 1u && g <= (uint32_t)max_pairs) {
            // the key was inserted under the same condition, so the probe finds it before an empty slot
            const unsigned long long key = hesaff_plan::index_key(r, word);
            unsigned long long slot = hesaff_plan::index_hash_slot(key, bits);
            unsigned long long seen = hash_keys[slot];
            while (seen != key && seen != hesaff_plan::HS_INDEX_EMPTY) { slot = (slot + 1ull) & mask; seen = hash_keys[slot]; }
            if (seen == key && g * hash_tf[slot] <= (uint32_t)max_pairs) cnt = g;
         }
      }
      uint32_t inc = cnt;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
         const uint32_t t = __shfl_up(inc, d, 64);
         if (lane >= (uint32_t)d) inc += t;
      }
      if (lane == 63u) s_wsum[wv] = inc;
      __syncthreads();
      uint32_t at = base + inc - cnt, sum = 0;
      for (uint32_t v = 0; v < 4u; v++) { if (v < wv) at += s_wsum[v]; sum += s_wsum[v]; }
      for (uint32_t t = 0; t < cnt && at + t < cap; t++) {
         const uint32_t i = members[offsets[word] + t];
         const VerifyRow q = qrows[i];
         const hesaff_plan::VerifyFrame fq = hesaff_plan::verify_frame(q.x, q.y, q.a, q.b, q.c);
         const size_t pos = (size_t)(at + t);
         my_pairs[pos * 2] = (int32_t)i; my_pairs[pos * 2 + 1] = (int32_t)jl;
         float *c = my_corr + pos * hesaff_plan::HS_VERIFY_PAIR_FLOATS;
         c[0] = fq.x; c[1] = fq.y; c[2] = fq.p; c[3] = fq.q; c[4] = fq.r;
         c[5] = fd.x; c[6] = fd.y; c[7] = fd.p; c[8] = fd.q; c[9] = fd.r;
      }
      base += sum;
      __syncthreads();   // s_wsum is written again
   }
   if (tid == 0u) { found[r] = base; used[r] = min(base, cap); }
}

// Grid: (ceil(max M / HS_VERIFY_TILE), candidates).  corr[r][4096][10], used[r] = M_r, best[r] zero on entry; inl_out NULL or
// [r][4096]: inl(h) of every h < M_r.
__global__ __launch_bounds__(HS_VERIFY_TILE) void k_verify_hypotheses(const float *__restrict__ corr, const uint32_t *__restrict__ used, float tol2,
                                                                      int32_t *__restrict__ inl_out, unsigned long long *__restrict__ best)
{
   __shared__ float4 s_c[HS_VERIFY_CHUNK];
   const uint32_t r = blockIdx.y, tid = threadIdx.x;
   const uint32_t m = min(used[r], (uint32_t)hesaff_plan::HS_VERIFY_MAX_USED);
   const uint32_t h0 = blockIdx.x * HS_VERIFY_TILE;
   if (h0 >= m) return;   // (the whole block)
   const float *const my = corr + (size_t)r * hesaff_plan::HS_VERIFY_MAX_USED * hesaff_plan::HS_VERIFY_PAIR_FLOATS;
   const uint32_t h = h0 + tid;
   const bool own = h < m;
   const float *const c = my + (size_t)(own ? h : h0) * hesaff_plan::HS_VERIFY_PAIR_FLOATS;   // (a lane without a hypothesis computes the tile's first and drops it)
   const float xq = c[0], yq = c[1], xd = c[5], yd = c[6];
   const hesaff_plan::VerifyMap L = hesaff_plan::verify_map(c[2], c[3], c[4], c[7], c[8], c[9]);
   uint32_t inl = 0;
   for (uint32_t k0 = 0; k0 < m; k0 += HS_VERIFY_CHUNK) {
      const uint32_t kn = min((uint32_t)HS_VERIFY_CHUNK, m - k0);
      __syncthreads();   // the previous chunk has been read
      for (uint32_t t = tid; t < kn; t += HS_VERIFY_TILE) {
         const float *e = my + (size_t)(k0 + t) * hesaff_plan::HS_VERIFY_PAIR_FLOATS;
         s_c[t] = make_float4(e[0], e[1], e[5], e[6]);
      }
      __syncthreads();
      // (no vectorisation across k: the packed v_pk_mul_f32 / v_pk_add_f32 it produces issue in the time of two scalar operations on
      // gfx950 and cost eight register moves per pair of steps on top)
#pragma clang loop vectorize(disable) interleave(disable) unroll_count(4)
      for (uint32_t k = 0; k < kn; k++) {
         const float4 e = s_c[k];   // the same address in every lane
         const float dx = e.x - xq;
         const float dy = e.y - yq;
         const float u = L.L11 * dx;
         const float v1 = L.L21 * dx;
         const float v2 = L.L22 * dy;
         const float v = v1 + v2;
         const float ex = (xd + u) - e.z;
         const float ey = (yd + v) - e.w;
         const float exx = ex * ex;
         const float eyy = ey * ey;
         const float e2 = exx + eyy;
         inl += e2 <= tol2 ? 1u : 0u;
      }
   }
   if (own && inl_out) inl_out[(size_t)r * hesaff_plan::HS_VERIFY_MAX_USED + h] = (int32_t)inl;
   unsigned long long key = own ? hesaff_plan::verify_best_key(inl, h) : 0ull;
#pragma unroll
   for (int d = 32; d >= 1; d >>= 1) {
      const unsigned long long o = __shfl_xor(key, d, 64);
      key = o > key ? o : key;
   }
   if ((tid & 63u) == 0u) atomicMax(&best[r], key);
}

// One block of 1024 threads, thread r for candidate r: out[r][6], hyp[r][3], and order[] = the candidates by (inliers descending,
// position ascending), ranked by counting.
__global__ __launch_bounds__(1024) void k_verify_finish(int n_candidates, const unsigned long long *__restrict__ best, const uint32_t *__restrict__ used,
                                                        const uint32_t *__restrict__ found, const uint32_t *__restrict__ inert, const int32_t *__restrict__ pairs,
                                                        const float *__restrict__ corr, int32_t *__restrict__ out, float *__restrict__ hyp, int32_t *__restrict__ order)
{
   __shared__ uint32_t s_inl[hesaff_plan::HS_VERIFY_MAX_CANDIDATES];
   const uint32_t r = threadIdx.x, n = (uint32_t)n_candidates;
   uint32_t inl = 0;
   if (r < n) {
      const unsigned long long key = best[r];
      inl = hesaff_plan::verify_best_inliers(key);
      const int32_t h = hesaff_plan::verify_best_h(key);
      int32_t qi = -1, dj = -1;
      hesaff_plan::VerifyMap L = {0.0f, 0.0f, 0.0f};
      if (h >= 0) {
         const size_t pos = (size_t)r * hesaff_plan::HS_VERIFY_MAX_USED + (size_t)h;
         qi = pairs[pos * 2]; dj = pairs[pos * 2 + 1];
         const float *c = corr + pos * hesaff_plan::HS_VERIFY_PAIR_FLOATS;
         L = hesaff_plan::verify_map(c[2], c[3], c[4], c[7], c[8], c[9]);
      }
      int32_t *o = out + (size_t)r * 6;
      o[0] = (int32_t)inl; o[1] = (int32_t)used[r]; o[2] = (int32_t)found[r]; o[3] = qi; o[4] = dj; o[5] = (int32_t)inert[r];
      hyp[r * 3] = L.L11; hyp[r * 3 + 1] = L.L21; hyp[r * 3 + 2] = L.L22;
      s_inl[r] = inl;
   }
   __syncthreads();
   if (r < n) {
      uint32_t rank = 0;
      for (uint32_t v = 0; v < n; v++) {
         const uint32_t o = s_inl[v];
         rank += (o > inl || (o == inl && v < r)) ? 1u : 0u;
      }
      order[rank] = (int32_t)r;
   }
}
