// capi_expand.h -- query expansion (hesaff_expand_query, hesaff_expand_query_device and hesaff_get_expand_ms of include/hesaff_amd.h)
// over the kernels of kernels_expand.h, with every number from expand_plan.h.  Included at the end of pipeline.hip, behind
// capi_verify.h (same translation unit).  A call works in a scratch buffer of its own that it releases before it returns and keeps
// nothing in the context but the two event times: a context that never expands allocates, launches and copies nothing here, and
// the vocabulary, the index and the result of the last verify call are neither read nor written.
#pragma once

namespace {

// what both forms of a call share; `device` says where rows, signatures and the three outputs lie
struct ExpandCall {
   bool device;
   int nq;
   const void *query_rows, *query_sigs;
   int n_candidates;
   const int32_t *counts;
   const void *candidate_rows, *candidate_sigs;
   const int32_t *verify_out;
   const float *hyp;
   int min_inliers, max_images;
   const float *roi;
   int k, max_rows;
   void *rows_out, *words_out, *sigs_out;
   int *n_out;
   int32_t *info_out;
};

bool expand_args_ok(const hesaff_ctx *c, const ExpandCall &a)
{
   if (!c || !a.counts || !a.verify_out || !a.hyp || !a.roi || !a.rows_out || !a.words_out || !a.n_out) return false;
   if (!verify_counts_ok(a.n_candidates, a.k) || !verify_image_keys_ok(a.nq) || (a.nq > 0 && !a.query_rows)) return false;
   if (!expand_min_inliers_ok(a.min_inliers) || !expand_max_images_ok(a.max_images) || !expand_roi_ok(a.roi) || !expand_max_rows_ok(a.nq, a.max_rows)) return false;
   const int64_t total = verify_total_keys(a.counts, a.n_candidates);
   if (total < 0 || (total > 0 && !a.candidate_rows)) return false;
   // the signatures: of both sides or of neither, and then an output for them
   const bool with_sigs = a.sigs_out != nullptr;
   if ((a.nq > 0 && (a.query_sigs != nullptr) != with_sigs) || (total > 0 && (a.candidate_sigs != nullptr) != with_sigs)) return false;
   if (a.device) {
      for (const void *p : {a.query_rows, a.candidate_rows, (const void *)a.rows_out, (const void *)a.words_out})
         if ((uintptr_t)p % 4 != 0) return false;
      for (const void *p : {a.query_sigs, a.candidate_sigs, (const void *)a.sigs_out})
         if ((uintptr_t)p % 8 != 0) return false;
   }
   return true;
}

void expand_run(hesaff_ctx *c, const ExpandCall &a, const char *who)
{
   const int R = a.n_candidates, nq = a.nq;
   const int64_t total = verify_total_keys(a.counts, R);
   const bool with_sigs = a.sigs_out != nullptr;
   hipStream_t st = c->stream();
   bind_device(c);
   std::vector<int64_t> first((size_t)R + 1, 0);   // candidate r's rows begin at row first[r] of the caller's array
   for (int r = 0; r < R; r++) first[(size_t)r + 1] = first[(size_t)r] + a.counts[r];
   // the words, and step 1: the selection, with the eligible candidates' anchors checked on the host
   ExpandSelection sel;
   if (a.device) {
      check_device_words(c, (const int32_t *)a.query_rows + 5, 6, nq, a.k, who);
      check_device_words(c, (const int32_t *)a.candidate_rows + 5, 6, (long long)total, a.k, who);
      TrainArena g;
      const Span<uint32_t> starts = g.add<uint32_t>((size_t)R + 1);
      const Span<int32_t> out = g.add<int32_t>((size_t)R * 6);
      const Span<VerifyRow> anchors = g.add<VerifyRow>((size_t)R * 2);
      g.ensure();
      const std::vector<uint32_t> h_starts(first.begin(), first.end());
      std::vector<VerifyRow> h_anchors((size_t)R * 2);
      HIP_TRY(hipMemcpyAsync(g.ptr(starts), h_starts.data(), h_starts.size() * 4, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(g.ptr(out), a.verify_out, (size_t)R * 24, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemsetAsync(g.ptr(anchors), 0, anchors.bytes(), st));
      hipLaunchKernelGGL(k_expand_anchors, dim3(1), dim3(1024), 0, st, (const VerifyRow *)a.query_rows, (const VerifyRow *)a.candidate_rows,
                         (const uint32_t *)g.ptr(starts), (const int32_t *)g.ptr(out), R, nq, a.min_inliers, g.ptr(anchors));
      HIP_TRY(hipMemcpyAsync(h_anchors.data(), g.ptr(anchors), anchors.bytes(), hipMemcpyDeviceToHost, st));
      finish_stream(c);
      sel = expand_select(a.verify_out, a.hyp, a.counts, R, nq, a.min_inliers, a.max_images, [&](int64_t r, int32_t, int32_t, VerifyRow &q, VerifyRow &d) {
         q = h_anchors[(size_t)r * 2];
         d = h_anchors[(size_t)r * 2 + 1];
      });
   } else {
      if (!verify_words_ok(a.query_rows, nq, a.k) || !verify_words_ok(a.candidate_rows, total, a.k)) throw HsError(HESAFF_ERR_ARG, word_outside(who, "vocabulary_size"));
      sel = expand_select(a.verify_out, a.hyp, a.counts, R, nq, a.min_inliers, a.max_images, [&](int64_t r, int32_t qk, int32_t ck, VerifyRow &q, VerifyRow &d) {
         q = ((const VerifyRow *)a.query_rows)[qk];
         d = ((const VerifyRow *)a.candidate_rows)[first[(size_t)r] + ck];
      });
   }
   if (sel.bad >= 0)
      throw HsError(HESAFF_ERR_ARG, std::string(who) + ": candidate " + std::to_string(sel.bad) + " is eligible, but its keys, its anchor rows or its map lie outside "
                                                       "what hesaff_verify_matches returns");
   // the tiles, the scratch and - in the host form - the staged rows and the outputs: everything that can be refused for memory
   const ExpandTiles tiles = expand_tiles(sel, a.counts, R, !a.device);
   const int E = (int)sel.r.size();
   const int64_t out_rows = expand_output_rows(nq, tiles.rows, a.max_rows);
   TrainArena m;
   const ExpandScratchArrays s = expand_scratch_arrays(m, E, tiles.tiles);
   ExpandStagedArrays h = {};
   if (!a.device) h = expand_staged_arrays(m, tiles.rows, out_rows, with_sigs);
   m.ensure();
   const VerifyRow *d_rows = a.device ? (const VerifyRow *)a.candidate_rows : m.ptr(h.rows);
   const unsigned long long *d_sigs = !with_sigs ? nullptr : a.device ? (const unsigned long long *)a.candidate_sigs : m.ptr(h.sigs);
   VerifyRow *d_rows_out = a.device ? (VerifyRow *)a.rows_out : m.ptr(h.rows_out);
   int32_t *d_words_out = a.device ? (int32_t *)a.words_out : m.ptr(h.words_out);
   unsigned long long *d_sigs_out = !with_sigs ? nullptr : a.device ? (unsigned long long *)a.sigs_out : m.ptr(h.sigs_out);
   const hipMemcpyKind in = a.device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
   // step 4, first half: the query's rows byte for byte, their words and signatures
   if (nq > 0) {
      HIP_TRY(hipMemcpyAsync(d_rows_out, a.query_rows, (size_t)nq * sizeof(VerifyRow), in, st));
      if (with_sigs) HIP_TRY(hipMemcpyAsync(d_sigs_out, a.query_sigs, (size_t)nq * 8, in, st));
      hipLaunchKernelGGL(k_expand_query_words, dim3((uint32_t)((nq + 255) / 256)), dim3(256), 0, st, (const VerifyRow *)d_rows_out, nq, d_words_out);
   }
   if (!a.device) {
      for (const ExpandCand &e : tiles.cand) {
         if (e.count == 0) continue;
         HIP_TRY(hipMemcpyAsync(m.ptr(h.rows) + e.start, (const VerifyRow *)a.candidate_rows + first[e.r], (size_t)e.count * sizeof(VerifyRow), hipMemcpyHostToDevice, st));
         if (with_sigs)
            HIP_TRY(hipMemcpyAsync(m.ptr(h.sigs) + e.start, (const unsigned long long *)a.candidate_sigs + first[e.r], (size_t)e.count * 8, hipMemcpyHostToDevice, st));
      }
   }
   const bool timed = c->profiling >= 1;
   DevEvent ev[3];
   if (timed) for (DevEvent &e : ev) e = DevEvent(hipEventDefault);
   if (E > 0) HIP_TRY(hipMemcpyAsync(m.ptr(s.cand), tiles.cand.data(), (size_t)E * sizeof(ExpandCand), hipMemcpyHostToDevice, st));
   HIP_TRY(hipMemcpyAsync(m.ptr(s.prefix), tiles.prefix.data(), tiles.prefix.size() * 4, hipMemcpyHostToDevice, st));
   HIP_TRY(hipMemsetAsync(m.ptr(s.info), 0, s.info.bytes(), st));
   const ExpandRoi roi = {a.roi[0], a.roi[1], a.roi[2], a.roi[3]};
   const uint32_t blocks = (tiles.tiles + HS_EXPAND_BLOCK_TILES - 1) / HS_EXPAND_BLOCK_TILES;
   if (timed) HIP_TRY(hipEventRecord(ev[0], st));
   if (blocks > 0)
      hipLaunchKernelGGL(k_expand_flags, dim3(blocks), dim3(256), 0, st, d_rows, (const ExpandCand *)m.ptr(s.cand), (const uint32_t *)m.ptr(s.prefix), E, tiles.tiles, roi,
                         m.ptr(s.mask), m.ptr(s.info));
   LoadPopc load;
   load.p = m.ptr(s.mask);
   exclusive_scan(c, load, (long long)tiles.tiles, m.ptr(s.base), m.ptr(s.base) + tiles.tiles, m.ptr(s.block_sums));
   if (timed) HIP_TRY(hipEventRecord(ev[1], st));
   if (blocks > 0)
      hipLaunchKernelGGL(k_expand_scatter, dim3(blocks), dim3(256), 0, st, d_rows, d_sigs, (const ExpandCand *)m.ptr(s.cand), (const uint32_t *)m.ptr(s.prefix), E, tiles.tiles,
                         roi, (const unsigned long long *)m.ptr(s.mask), (const uint32_t *)m.ptr(s.base), (uint32_t)nq, (uint32_t)a.max_rows, d_rows_out, d_words_out,
                         d_sigs_out, m.ptr(s.info));
   if (timed) HIP_TRY(hipEventRecord(ev[2], st));
   // kept_total and the counts cross to the host: 4 + 12 E bytes
   uint32_t *back = (uint32_t *)c->h_small_end.ensure_small((size_t)(1 + HS_EXPAND_MAX_IMAGES * HS_EXPAND_INFO) * 4);
   HIP_TRY(hipMemcpyAsync(back, m.ptr(s.base) + tiles.tiles, 4, hipMemcpyDeviceToHost, st));
   if (E > 0) HIP_TRY(hipMemcpyAsync(back + 1, m.ptr(s.info), (size_t)E * HS_EXPAND_INFO * 4, hipMemcpyDeviceToHost, st));
   finish_stream(c);
   const int64_t n_out = std::min<int64_t>((int64_t)nq + (int64_t)back[0], a.max_rows);
   if (!a.device && n_out > 0) {
      HIP_TRY(hipMemcpyAsync(a.rows_out, d_rows_out, (size_t)n_out * sizeof(VerifyRow), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(a.words_out, d_words_out, (size_t)n_out * 4, hipMemcpyDeviceToHost, st));
      if (with_sigs) HIP_TRY(hipMemcpyAsync(a.sigs_out, d_sigs_out, (size_t)n_out * 8, hipMemcpyDeviceToHost, st));
      finish_stream(c);
   }
   c->expand_ms[0] = c->expand_ms[1] = 0.0f;
   if (timed) {
      HIP_TRY(hipEventElapsedTime(&c->expand_ms[0], ev[0], ev[1]));
      HIP_TRY(hipEventElapsedTime(&c->expand_ms[1], ev[1], ev[2]));
   }
   *a.n_out = (int)n_out;
   if (a.info_out) {
      for (int r = 0; r < R; r++) { int32_t *o = a.info_out + (size_t)r * 4; o[0] = -1; o[1] = o[2] = o[3] = 0; }
      for (int e = 0; e < E; e++) {
         int32_t *o = a.info_out + (size_t)sel.r[(size_t)e] * 4;
         o[0] = e;
         for (int i = 0; i < HS_EXPAND_INFO; i++) o[1 + i] = (int32_t)back[1 + (size_t)e * HS_EXPAND_INFO + i];
      }
   }
}

} // namespace

extern "C" {

int hesaff_expand_query(hesaff_ctx *c, int nq, const void *query_rows, const uint64_t *query_sigs, int n_candidates, const int32_t *counts, const void *candidate_rows,
                        const uint64_t *candidate_sigs, const int32_t *verify_out, const float *hyp, int min_inliers, int max_images, const float *roi,
                        int vocabulary_size, int max_rows, void *rows_out, int32_t *words_out, uint64_t *sigs_out, int *n_out, int32_t *info_out)
{
   const ExpandCall a = {false, nq, query_rows, query_sigs, n_candidates, counts, candidate_rows, candidate_sigs, verify_out, hyp, min_inliers, max_images, roi,
                         vocabulary_size, max_rows, rows_out, words_out, sigs_out, n_out, info_out};
   if (!expand_args_ok(c, a)) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   expand_run(c, a, "hesaff_expand_query");
   HS_API_END(c)
}

int hesaff_expand_query_device(hesaff_ctx *c, int nq, const void *d_query_rows, const void *d_query_sigs, int n_candidates, const int32_t *counts,
                               const void *d_candidate_rows, const void *d_candidate_sigs, const int32_t *verify_out, const float *hyp, int min_inliers, int max_images,
                               const float *roi, int vocabulary_size, int max_rows, void *d_rows_out, void *d_words_out, void *d_sigs_out, int *n_out, int32_t *info_out)
{
   const ExpandCall a = {true, nq, d_query_rows, d_query_sigs, n_candidates, counts, d_candidate_rows, d_candidate_sigs, verify_out, hyp, min_inliers, max_images, roi,
                         vocabulary_size, max_rows, d_rows_out, d_words_out, d_sigs_out, n_out, info_out};
   if (!expand_args_ok(c, a)) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   expand_run(c, a, "hesaff_expand_query_device");
   HS_API_END(c)
}

int hesaff_get_expand_ms(const hesaff_ctx *c, float *flags_ms, float *scatter_ms)
{
   if (!c || !flags_ms || !scatter_ms) return HESAFF_ERR_ARG;
   *flags_ms = c->expand_ms[0];
   *scatter_ms = c->expand_ms[1];
   return HESAFF_OK;
}

} // extern "C"
