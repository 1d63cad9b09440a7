// capi_verify.h -- spatial verification (hesaff_verify_*, hesaff_stage_verify_pairs and hesaff_get_verify_ms of include/hesaff_amd.h)
// over the kernels of kernels_verify.h, with every number from verify_plan.h.  Included at the end of pipeline.hip, behind
// capi_index.h (same translation unit).  A call works in a scratch buffer of its own that it releases before it returns; only the
// result of the last call stays in the context (hesaff_ctx::verify), so a context that never verifies allocates, launches and copies
// nothing here, and the vocabulary and the index are neither read nor written.
#pragma once

namespace {

static_assert(sizeof(VerifyRow) == 24, "a words-file row");

// rows in host memory: false where a word lies outside 0 .. k - 1
bool verify_words_ok(const void *rows, int64_t n, int k)
{
   const VerifyRow *p = (const VerifyRow *)rows;
   for (int64_t j = 0; j < n; j++)
      if (p[j].word >= (uint32_t)k) return false;
   return true;
}

// the verification of R candidates over rows in device memory (arguments and words checked by the caller)
void verify_on_device(hesaff_ctx *c, int nq, const VerifyRow *d_query, int n_candidates, const int32_t *counts, const VerifyRow *d_rows, int64_t total, int k,
                      int max_pairs, float tol, int32_t *out, float *hyp, int32_t *order)
{
   hesaff_ctx::Verify &v = c->verify;
   // everything that can be refused for memory comes first: the scratch, and a result buffer where the context's is too small
   TrainArena m;   // the scratch of the call, released when it returns
   const VerifyScratchArrays s = verify_scratch_arrays(m, n_candidates, k, nq, total);
   m.ensure();
   StagePlan rp;
   const VerifyResultArrays ra = verify_result_arrays(rp, n_candidates);
   if (v.result.bytes < rp.bytes()) {
      DevBuf fresh;
      fresh.ensure(rp.bytes());   // (HESAFF_ERR_NOMEM: the last call's result stays)
      HIP_TRY(hipStreamSynchronize(c->stream()));
      v.result = std::move(fresh);
   }
   v.done = false;
   v.a = ra;
   hipStream_t st = c->stream();
   const bool timed = c->profiling >= 1;
   DevEvent ev[3];
   if (timed) for (DevEvent &e : ev) e = DevEvent(hipEventDefault);
   std::vector<uint32_t> starts((size_t)n_candidates + 1);
   starts[0] = 0;
   for (int i = 0; i < n_candidates; i++) starts[(size_t)i + 1] = starts[(size_t)i] + (uint32_t)counts[i];
   HIP_TRY(hipMemcpyAsync(m.ptr(s.starts), starts.data(), starts.size() * 4, hipMemcpyHostToDevice, st));
   HIP_TRY(hipMemsetAsync(m.ptr(s.hash_keys), 0xFF, s.hash_keys.bytes(), st));
   HIP_TRY(hipMemsetAsync(m.ptr(s.hash_tf), 0, s.hash_tf.bytes(), st));
   HIP_TRY(hipMemsetAsync(m.ptr(s.tfq), 0, s.tfq.bytes(), st));
   HIP_TRY(hipMemsetAsync(m.ptr(s.inert), 0, s.inert.bytes(), st));
   HIP_TRY(hipMemsetAsync(m.ptr(s.best), 0, s.best.bytes(), st));
   HIP_TRY(hipMemsetAsync(v.ptr(ra.qinert), 0, 4, st));
   // the query's keys grouped by word, the candidates' tf, the pairs
   if (timed) HIP_TRY(hipEventRecord(ev[0], st));
   if (nq > 0) hipLaunchKernelGGL(k_verify_query_count, dim3((uint32_t)((nq + 255) / 256)), dim3(256), 0, st, d_query, nq, m.ptr(s.tfq), v.ptr(ra.qinert));
   LoadU32 load;
   load.p = m.ptr(s.tfq);
   exclusive_scan(c, load, (long long)k, m.ptr(s.offsets), m.ptr(s.offsets) + k, m.ptr(s.block_sums));
   HIP_TRY(hipMemcpyAsync(m.ptr(s.cursor), m.ptr(s.offsets), (size_t)k * 4, hipMemcpyDeviceToDevice, st));
   if (nq > 0) {
      hipLaunchKernelGGL(k_verify_query_scatter, dim3((uint32_t)((nq + 255) / 256)), dim3(256), 0, st, d_query, nq, m.ptr(s.cursor), m.ptr(s.members));
      hipLaunchKernelGGL(k_verify_sort_groups, dim3((uint32_t)((k + 255) / 256)), dim3(256), 0, st, (const uint32_t *)m.ptr(s.offsets), k, m.ptr(s.members));
   }
   if (total > 0)
      hipLaunchKernelGGL(k_verify_insert, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, st, d_rows, (const uint32_t *)m.ptr(s.starts), n_candidates, (uint32_t)total,
                         (const uint32_t *)m.ptr(s.tfq), max_pairs, s.bits, m.ptr(s.hash_keys), m.ptr(s.hash_tf), m.ptr(s.inert));
   hipLaunchKernelGGL(k_verify_pairs, dim3((uint32_t)n_candidates), dim3(256), 0, st, d_query, d_rows, (const uint32_t *)m.ptr(s.starts), (const uint32_t *)m.ptr(s.tfq),
                      (const uint32_t *)m.ptr(s.offsets), (const uint32_t *)m.ptr(s.members), max_pairs, s.bits, (const unsigned long long *)m.ptr(s.hash_keys),
                      (const uint32_t *)m.ptr(s.hash_tf), v.ptr(ra.pairs), m.ptr(s.corr), m.ptr(s.found), m.ptr(s.used));
   if (timed) HIP_TRY(hipEventRecord(ev[1], st));
   // the hypotheses, the result and the ranking
   hipLaunchKernelGGL(k_verify_hypotheses, dim3(HS_VERIFY_MAX_USED / HS_VERIFY_TILE, (uint32_t)n_candidates), dim3(HS_VERIFY_TILE), 0, st, (const float *)m.ptr(s.corr),
                      (const uint32_t *)m.ptr(s.used), tol * tol, (int32_t *)nullptr, m.ptr(s.best));
   hipLaunchKernelGGL(k_verify_finish, dim3(1), dim3(1024), 0, st, n_candidates, (const unsigned long long *)m.ptr(s.best), (const uint32_t *)m.ptr(s.used),
                      (const uint32_t *)m.ptr(s.found), (const uint32_t *)m.ptr(s.inert), (const int32_t *)v.ptr(ra.pairs), (const float *)m.ptr(s.corr), v.ptr(ra.out),
                      v.ptr(ra.hyp), v.ptr(ra.order));
   if (timed) HIP_TRY(hipEventRecord(ev[2], st));
   // out, hyp, order and the query's inert count cross to the host: 40 bytes per candidate
   const size_t R = (size_t)n_candidates;
   char *h = (char *)c->h_small_end.ensure_small((size_t)HS_VERIFY_MAX_CANDIDATES * 40 + 4);
   HIP_TRY(hipMemcpyAsync(h, v.ptr(ra.out), R * 24, hipMemcpyDeviceToHost, st));
   HIP_TRY(hipMemcpyAsync(h + R * 24, v.ptr(ra.hyp), R * 12, hipMemcpyDeviceToHost, st));
   HIP_TRY(hipMemcpyAsync(h + R * 36, v.ptr(ra.order), R * 4, hipMemcpyDeviceToHost, st));
   HIP_TRY(hipMemcpyAsync(h + R * 40, v.ptr(ra.qinert), 4, hipMemcpyDeviceToHost, st));
   finish_stream(c);
   c->verify_ms[0] = c->verify_ms[1] = 0.0f;
   if (timed) {
      HIP_TRY(hipEventElapsedTime(&c->verify_ms[0], ev[0], ev[1]));
      HIP_TRY(hipEventElapsedTime(&c->verify_ms[1], ev[1], ev[2]));
   }
   v.used.resize(R);
   for (size_t r = 0; r < R; r++) memcpy(&v.used[r], h + r * 24 + 4, 4);
   memcpy(&v.query_inert, h + R * 40, 4);
   v.n_candidates = n_candidates;
   v.done = true;
   if (out) memcpy(out, h, R * 24);
   if (hyp) memcpy(hyp, h + R * 24, R * 12);
   if (order) memcpy(order, h + R * 36, R * 4);
}

bool verify_args_ok(const hesaff_ctx *c, int nq, const void *query_rows, int n_candidates, const int32_t *counts, int k, int max_pairs, float tol)
{
   return c && counts && verify_counts_ok(n_candidates, k) && verify_image_keys_ok(nq) && (nq == 0 || query_rows) && verify_pairs_ok(max_pairs) && verify_tolerance_ok(tol);
}

} // namespace

extern "C" {

int hesaff_verify_matches_device(hesaff_ctx *c, int nq, const void *d_query_rows, int n_candidates, const int32_t *counts, const void *d_candidate_rows,
                                 int vocabulary_size, int max_pairs, float tolerance, int32_t *out, float *hyp, int32_t *order)
{
   if (!verify_args_ok(c, nq, d_query_rows, n_candidates, counts, vocabulary_size, max_pairs, tolerance)) return HESAFF_ERR_ARG;
   const int64_t total = verify_total_keys(counts, n_candidates);
   if (total < 0 || (total > 0 && !d_candidate_rows) || (uintptr_t)d_candidate_rows % 4 != 0 || (uintptr_t)d_query_rows % 4 != 0) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   // (a row is six 4-byte words, its word the sixth)
   check_device_words(c, (const int32_t *)d_query_rows + 5, 6, nq, vocabulary_size, "hesaff_verify_matches_device");
   check_device_words(c, (const int32_t *)d_candidate_rows + 5, 6, (long long)total, vocabulary_size, "hesaff_verify_matches_device");
   verify_on_device(c, nq, (const VerifyRow *)d_query_rows, n_candidates, counts, (const VerifyRow *)d_candidate_rows, total, vocabulary_size, max_pairs, tolerance, out,
                    hyp, order);
   HS_API_END(c)
}

int hesaff_verify_matches(hesaff_ctx *c, int nq, const void *query_rows, int n_candidates, const int32_t *counts, const void *candidate_rows, int vocabulary_size,
                          int max_pairs, float tolerance, int32_t *out, float *hyp, int32_t *order)
{
   if (!verify_args_ok(c, nq, query_rows, n_candidates, counts, vocabulary_size, max_pairs, tolerance)) return HESAFF_ERR_ARG;
   const int64_t total = verify_total_keys(counts, n_candidates);
   if (total < 0 || (total > 0 && !candidate_rows)) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   if (!verify_words_ok(query_rows, nq, vocabulary_size) || !verify_words_ok(candidate_rows, total, vocabulary_size))
      throw HsError(HESAFF_ERR_ARG, "hesaff_verify_matches: a word lies outside 0 .. vocabulary_size - 1");
   bind_device(c);
   DevBuf dq, dr;
   dq.ensure(std::max<size_t>((size_t)nq * sizeof(VerifyRow), 256));
   dr.ensure(std::max<size_t>((size_t)total * sizeof(VerifyRow), 256));
   if (nq > 0) HIP_TRY(hipMemcpyAsync(dq.p, query_rows, (size_t)nq * sizeof(VerifyRow), hipMemcpyHostToDevice, c->stream()));
   if (total > 0) HIP_TRY(hipMemcpyAsync(dr.p, candidate_rows, (size_t)total * sizeof(VerifyRow), hipMemcpyHostToDevice, c->stream()));
   verify_on_device(c, nq, dq.as<VerifyRow>(), n_candidates, counts, dr.as<VerifyRow>(), total, vocabulary_size, max_pairs, tolerance, out, hyp, order);
   HS_API_END(c)
}

int hesaff_verify_get_pairs(hesaff_ctx *c, int candidate, const int32_t **pairs, int *count)
{
   if (!c || !pairs || !count || !c->verify.done || candidate < 0 || candidate >= c->verify.n_candidates) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   hesaff_ctx::Verify &v = c->verify;
   const size_t n = (size_t)v.used[(size_t)candidate];
   v.h_pairs.resize(std::max<size_t>(n * 2, 2));
   if (n > 0) HIP_TRY(hipMemcpy(v.h_pairs.data(), v.ptr(v.a.pairs) + (size_t)candidate * HS_VERIFY_MAX_USED * 2, n * 8, hipMemcpyDeviceToHost));
   *pairs = v.h_pairs.data();
   *count = (int)n;
   HS_API_END(c)
}

int hesaff_verify_get_query_inert(const hesaff_ctx *c, int *n)
{
   if (!c || !n || !c->verify.done) return HESAFF_ERR_ARG;
   *n = (int)c->verify.query_inert;
   return HESAFF_OK;
}

int hesaff_stage_verify_pairs(hesaff_ctx *c, int m, const float *pairs, float tolerance, int32_t *inl_out, int32_t *best_out)
{
   if (!c || !verify_used_ok(m) || (m > 0 && !pairs) || !verify_tolerance_ok(tolerance)) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   TrainArena a;
   const Span<float> corr = a.add<float>((size_t)std::max(m, 1) * HS_VERIFY_PAIR_FLOATS);
   const Span<int32_t> inl = a.add<int32_t>((size_t)HS_VERIFY_MAX_USED);
   const Span<uint32_t> used = a.add<uint32_t>(1);
   const Span<unsigned long long> best = a.add<unsigned long long>(1);
   a.ensure();
   hipStream_t st = c->stream();
   const uint32_t mu = (uint32_t)m;
   unsigned long long key = 0ull;
   HIP_TRY(hipMemcpyAsync(a.ptr(used), &mu, 4, hipMemcpyHostToDevice, st));
   HIP_TRY(hipMemsetAsync(a.ptr(best), 0, 8, st));
   if (m > 0) {
      HIP_TRY(hipMemcpyAsync(a.ptr(corr), pairs, (size_t)m * HS_VERIFY_PAIR_FLOATS * 4, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(k_verify_hypotheses, dim3((uint32_t)((m + HS_VERIFY_TILE - 1) / HS_VERIFY_TILE), 1), dim3(HS_VERIFY_TILE), 0, st, (const float *)a.ptr(corr),
                         (const uint32_t *)a.ptr(used), tolerance * tolerance, a.ptr(inl), a.ptr(best));
      if (inl_out) HIP_TRY(hipMemcpyAsync(inl_out, a.ptr(inl), (size_t)m * 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(&key, a.ptr(best), 8, hipMemcpyDeviceToHost, st));
   }
   finish_stream(c);
   if (best_out) *best_out = verify_best_h(key);
   HS_API_END(c)
}

int hesaff_get_verify_ms(const hesaff_ctx *c, float *pairs_ms, float *hypotheses_ms)
{
   if (!c || !pairs_ms || !hypotheses_ms) return HESAFF_ERR_ARG;
   *pairs_ms = c->verify_ms[0];
   *hypotheses_ms = c->verify_ms[1];
   return HESAFF_OK;
}

} // extern "C"
