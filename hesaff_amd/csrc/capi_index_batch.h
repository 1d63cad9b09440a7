// capi_index_batch.h -- batched index queries (hesaff_index_query_batch*, hesaff_index_set_batch_budget and the getters declared with
// them in include/hesaff_amd.h) over the kernels of kernels_index_batch.h, with every number from index_batch_plan.h.  Included at the
// end of pipeline.hip, behind capi_index_grow.h (same translation unit).  A batch runs in chunks of consecutive queries; everything a
// batch needs - the staged words, the chunks' query starts, the scratch of its largest chunk, the pinned block of the ranked rows - is
// allocated before the first chunk runs, so a refused or failed call leaves the index and the last query's scores as they were.  The
// single-query entry points do not come through here, and a context that makes no batch call allocates, launches and copies nothing.
#pragma once

namespace {

// nq queries of counts[q] checked words each in device memory; the ranked rows go to the caller's arrays
void query_batch_on_device(hesaff_ctx *c, int nq, const int32_t *counts, const QuerySource &src, int top, int32_t *images_out, double *scores_out, int *count_out)
{
   hesaff_ctx::Index &ix = c->index;
   const int n_images = ix.n_images, keep = std::min(top, n_images);
   const size_t budget = index_batch_budget(c->index_batch_budget);
   // the chunks, and each chunk's query starts counted from its own first word: chunk number ci's are starts[first + ci ..]
   std::vector<IndexBatchChunk> chunks;
   std::vector<uint32_t> starts;
   starts.reserve((size_t)nq + 64);
   size_t scratch_bytes = 0, ranked_bytes = 0;
   for (int64_t first = 0, word_first = 0; first < nq;) {
      const IndexBatchChunk ch = index_batch_next_chunk(counts, nq, first, word_first, n_images, keep, budget);
      const size_t at = starts.size();
      starts.resize(at + (size_t)ch.count + 1);
      index_starts(counts + first, ch.count, &starts[at]);
      scratch_bytes = std::max(scratch_bytes, ch.bytes);
      ranked_bytes = std::max(ranked_bytes, index_batch_ranked_bytes(ch.count, keep));
      chunks.push_back(ch);
      first += ch.count; word_first += ch.words;
   }
   // everything the batch holds, before anything runs (HESAFF_ERR_NOMEM: nothing has changed)
   ix.batch_scratch.ensure(std::max<size_t>(scratch_bytes, 256));
   ix.batch_starts.ensure(std::max<size_t>(starts.size() * 4, 256));
   ix.batch_ranked.ensure(std::max<size_t>(ranked_bytes, 4096));
   hipStream_t st = c->stream();
   const bool timed = c->profiling >= 1;
   DevEvent ev[4], whole[2];   // of a chunk: grouping 0 .. 1, scoring 1 .. 2, finish and selection 2 .. 3
   if (timed) {
      for (DevEvent &e : ev) e = DevEvent(hipEventDefault);
      for (DevEvent &e : whole) e = DevEvent(hipEventDefault);
   }
   float part_ms[3] = {0.0f, 0.0f, 0.0f};
   if (timed) HIP_TRY(hipEventRecord(whole[0], st));
   HIP_TRY(hipMemcpyAsync(ix.batch_starts.p, starts.data(), starts.size() * 4, hipMemcpyHostToDevice, st));
   char *const base = ix.batch_scratch.as<char>();
   const char *const h = (const char *)ix.batch_ranked.p;
   for (size_t ci = 0; ci < chunks.size(); ci++) {
      const IndexBatchChunk &ch = chunks[ci];
      const bool last = ci + 1 == chunks.size();
      const int b = (int)ch.count;
      StagePlan plan;
      const IndexBatchArrays a = index_batch_arrays(plan, ch.count, n_images, keep, ch.words);
      unsigned long long *dot = (unsigned long long *)(base + a.dot.off), *hash_keys = (unsigned long long *)(base + a.hash_keys.off);
      IndexResultHead *heads = (IndexResultHead *)(base + a.heads.off);
      uint32_t *hash_tf = (uint32_t *)(base + a.hash_tf.off);
      double *score = (double *)(base + a.score.off), *ranked_scores = (double *)(base + a.ranked.off);
      int32_t *ranked_images = (int32_t *)(base + a.ranked_images_off);
      const uint32_t *d_starts = ix.batch_starts.as<uint32_t>() + ch.first + (int64_t)ci;
      const int32_t *d_words = src.w.d_words + ch.word_first * src.w.word_stride;
      const uint32_t words = (uint32_t)ch.words;
      // step 1: the distinct (query, word) pairs of the chunk and their counts
      if (timed) HIP_TRY(hipEventRecord(ev[0], st));
      HIP_TRY(hipMemsetAsync(base + a.zero_off, 0, a.zero_bytes, st));   // dot, the heads and the counts
      if (words > 0) {
         HIP_TRY(hipMemsetAsync(hash_keys, 0xFF, a.hash_keys.bytes(), st));
         hipLaunchKernelGGL(k_index_insert, dim3((words + 255u) / 256u), dim3(256), 0, st, d_words, src.w.word_stride, d_starts, b, words, a.bits, hash_keys, hash_tf);
      }
      if (timed) HIP_TRY(hipEventRecord(ev[1], st));
      // step 2: a wavefront per key
      if (words > 0) {
         if (src.embedded)
            hipLaunchKernelGGL(k_query_score_embedded_batch, dim3((words + 3u) / 4u), dim3(256), 0, st, d_words, src.w.word_stride, src.w.d_sigs + ch.word_first, d_starts, b,
                               words, src.threshold, a.bits, (const unsigned long long *)hash_keys, hash_tf, (const uint32_t *)ix.ptr(ix.a.idf),
                               (const uint32_t *)ix.kptr(ix.ka.offsets), (const unsigned long long *)ix.kptr(ix.ka.sig), (const uint32_t *)ix.kptr(ix.ka.image), n_images,
                               dot, heads);
         else
            hipLaunchKernelGGL(k_query_score_batch, dim3((words + 3u) / 4u), dim3(256), 0, st, d_words, src.w.word_stride, d_starts, b, words, a.bits,
                               (const unsigned long long *)hash_keys, hash_tf, (const uint32_t *)ix.ptr(ix.a.idf), (const uint32_t *)ix.ptr(ix.a.offsets),
                               (const IndexPosting *)ix.lists.as<IndexPosting>(), n_images, dot, heads);
      }
      if (timed) HIP_TRY(hipEventRecord(ev[2], st));
      // step 3: the scores of every (query, image), and a block per query ranks its row
      const unsigned long long pairs = (unsigned long long)b * (unsigned long long)n_images;
      hipLaunchKernelGGL(k_query_finish_batch, dim3(grid_for(pairs)), dim3(256), 0, st, (const unsigned long long *)dot, (const unsigned long long *)ix.ptr(ix.a.norm2),
                         (const IndexResultHead *)heads, n_images, pairs, score);
      hipLaunchKernelGGL(k_index_select_batch, dim3((uint32_t)b), dim3(HS_ISEL_THREADS), 0, st, (const double *)score, n_images, top, keep, ranked_images, ranked_scores, heads);
      if (timed) HIP_TRY(hipEventRecord(ev[3], st));
      if (last) {
         // the state Q single calls would leave: the last query's dot, score and head are the index's
         const size_t row = (size_t)(b - 1) * (size_t)n_images;
         HIP_TRY(hipMemcpyAsync(ix.ptr(ix.a.dot), dot + row, (size_t)n_images * 8, hipMemcpyDeviceToDevice, st));
         HIP_TRY(hipMemcpyAsync(ix.ptr(ix.a.score), score + row, (size_t)n_images * 8, hipMemcpyDeviceToDevice, st));
         HIP_TRY(hipMemcpyAsync(ix.ptr(ix.a.head), heads + (b - 1), sizeof(IndexResultHead), hipMemcpyDeviceToDevice, st));
         if (timed) HIP_TRY(hipEventRecord(whole[1], st));
      }
      // the ranked rows alone cross to the host: one copy of b x keep x 12 bytes, one sync
      const size_t rows = (size_t)b * (size_t)keep;
      HIP_TRY(hipMemcpyAsync(ix.batch_ranked.p, ranked_scores, rows * 12, hipMemcpyDeviceToHost, st));
      finish_stream(c);
      if (timed)
         for (int s = 0; s < 3; s++) {
            float ms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&ms, ev[s], ev[s + 1]));
            part_ms[s] += ms;
         }
      for (int q = 0; q < b; q++) {
         memcpy(scores_out + (size_t)(ch.first + q) * (size_t)top, h + (size_t)q * (size_t)keep * 8, (size_t)keep * 8);
         memcpy(images_out + (size_t)(ch.first + q) * (size_t)top, h + rows * 8 + (size_t)q * (size_t)keep * 4, (size_t)keep * 4);
      }
   }
   c->index_ms[2] = 0.0f;
   if (timed) HIP_TRY(hipEventElapsedTime(&c->index_ms[2], whole[0], whole[1]));
   for (int s = 0; s < 3; s++) c->index_batch_ms[s] = part_ms[s];
   c->index_batch_chunks = (int)chunks.size();
   *count_out = keep;
}

// the four batch forms: what they refuse before anything is staged, the staging - a host form's words and signatures in the index's
// own batch buffers - and the batch (src.n: set here)
int batch_from(hesaff_ctx *c, int n_queries, const int32_t *counts, WordSource src, int hamming, int top, int32_t *images_out, double *scores_out, int *count_out)
{
   if (!c || !counts || !images_out || !scores_out || !count_out || !index_batch_ok(n_queries, top) || !index_word_stride_ok(src.word_stride)) return HESAFF_ERR_ARG;
   if (!c->index.built || (src.with_sigs && (!embed_threshold_ok(hamming) || !c->index.embedded))) return HESAFF_ERR_ARG;
   src.n = index_batch_total(counts, n_queries);
   if (src.n < 0 || !source_ok(src)) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   const QuerySource q = {stage_source(c, src, c->index.k, c->index.batch_words, &c->index.batch_sigs), hamming, src.with_sigs};
   query_batch_on_device(c, n_queries, counts, q, top, images_out, scores_out, count_out);
   HS_API_END(c)
}

} // namespace

extern "C" {

int hesaff_index_query_batch_device(hesaff_ctx *c, int n_queries, const int32_t *counts, const void *d_words, int word_stride, int top, int32_t *images_out,
                                    double *scores_out, int *count_out)
{
   return batch_from(c, n_queries, counts, {"hesaff_index_query_batch_device", true, d_words, word_stride, 0, nullptr, false}, 0, top, images_out, scores_out, count_out);
}

int hesaff_index_query_batch(hesaff_ctx *c, int n_queries, const int32_t *counts, const int32_t *words, int word_stride, int top, int32_t *images_out,
                             double *scores_out, int *count_out)
{
   return batch_from(c, n_queries, counts, {"hesaff_index_query_batch", false, words, word_stride, 0, nullptr, false}, 0, top, images_out, scores_out, count_out);
}

int hesaff_index_query_batch_embedded_device(hesaff_ctx *c, int n_queries, const int32_t *counts, const void *d_words, int word_stride, const void *d_sigs, int hamming,
                                             int top, int32_t *images_out, double *scores_out, int *count_out)
{
   return batch_from(c, n_queries, counts, {"hesaff_index_query_batch_embedded_device", true, d_words, word_stride, 0, d_sigs, true}, hamming, top, images_out, scores_out,
                     count_out);
}

int hesaff_index_query_batch_embedded(hesaff_ctx *c, int n_queries, const int32_t *counts, const int32_t *words, int word_stride, const uint64_t *sigs, int hamming,
                                      int top, int32_t *images_out, double *scores_out, int *count_out)
{
   return batch_from(c, n_queries, counts, {"hesaff_index_query_batch_embedded", false, words, word_stride, 0, sigs, true}, hamming, top, images_out, scores_out, count_out);
}

// the device scratch a chunk may hold (0: the plan's default); what the batches so far allocated is released
int hesaff_index_set_batch_budget(hesaff_ctx *c, size_t bytes)
{
   if (!c) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   HIP_TRY(hipStreamSynchronize(c->stream()));
   c->index.release_batch();
   c->index_batch_budget = bytes;
   HS_API_END(c)
}

int hesaff_index_get_batch_budget(const hesaff_ctx *c, size_t *bytes)
{
   if (!c || !bytes) return HESAFF_ERR_ARG;
   *bytes = index_batch_budget(c->index_batch_budget);
   return HESAFF_OK;
}

int hesaff_index_get_batch_chunks(const hesaff_ctx *c, int *chunks)
{
   if (!c || !chunks) return HESAFF_ERR_ARG;
   *chunks = c->index_batch_chunks;
   return HESAFF_OK;
}

int hesaff_get_index_batch_ms(const hesaff_ctx *c, float *group_ms, float *score_ms, float *select_ms)
{
   if (!c || !group_ms || !score_ms || !select_ms) return HESAFF_ERR_ARG;
   *group_ms = c->index_batch_ms[0]; *score_ms = c->index_batch_ms[1]; *select_ms = c->index_batch_ms[2];
   return HESAFF_OK;
}

} // extern "C"
