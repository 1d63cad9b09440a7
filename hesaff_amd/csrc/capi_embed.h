// capi_embed.h -- Hamming embedding (hesaff_set_embedding, hesaff_embed_device, hesaff_train_embedding*, hesaff_index_build_embedded*,
// hesaff_index_query_embedded* and the getters declared with them in include/hesaff_amd.h): the entry points over the kernels of
// kernels_embed.h, with every number from embed_plan.h.  Included at the end of pipeline.hip, behind capi_verify.h (same translation
// unit).  The embedding is context state beside the vocabulary (hesaff_ctx::embed); a context without one allocates, launches and
// copies nothing here, and its assignment, its index and its queries are those of a context that never had one.
#pragma once

namespace {

void need_embedding(const hesaff_ctx *c)
{
   if (!c->embed.set) throw HsError(HESAFF_ERR_ARG, "no embedding is set (hesaff_set_embedding)");
}

// z[n][64] of n descriptors in device memory against a packed projection, into d_z
void project_on_device(hipStream_t st, const void *tiles, const int32_t *bias, const void *d_desc, long long n, long long stride, long long offset, int32_t *d_z)
{
   if (n > 0) launch_embed_kernel<true>(st, tiles, bias, nullptr, d_desc, n, stride, offset, nullptr, 1, d_z);
}

// the thresholds of k words from n descriptors and their checked words in device memory (arguments checked by the caller)
void train_embedding_on_device(hesaff_ctx *c, int n, const uint8_t *d_desc, long long stride, long long offset, const int32_t *d_words, int word_stride, int k,
                               const int8_t *P, int32_t *tau_out, uint32_t *counts_out)
{
   TrainArena m;
   const EmbedTrainArrays t = embed_train_arrays(m, n, k);
   m.ensure();
   hipStream_t st = c->stream();
   const bool timed = c->profiling >= 1;
   DevEvent ev[4];
   if (timed) for (DevEvent &e : ev) e = DevEvent(hipEventDefault);
   c->embed_train_ms[0] = c->embed_train_ms[1] = c->embed_train_ms[2] = 0.0f;
   std::vector<uint8_t> tiles(HS_EMBED_P_BYTES);
   int32_t bias[HS_EMBED_BITS];
   embed_pack_projection(P, tiles.data(), bias);
   HIP_TRY(hipMemcpyAsync(m.ptr(t.tiles), tiles.data(), tiles.size(), hipMemcpyHostToDevice, st));
   HIP_TRY(hipMemcpyAsync(m.ptr(t.bias), bias, sizeof bias, hipMemcpyHostToDevice, st));
   HIP_TRY(hipStreamSynchronize(st));   // (the pageable sources have been read)
   // step 1: every key's z
   if (timed) HIP_TRY(hipEventRecord(ev[0], st));
   project_on_device(st, m.ptr(t.tiles), m.ptr(t.bias), d_desc, n, stride, offset, m.ptr(t.z));
   if (timed) HIP_TRY(hipEventRecord(ev[1], st));
   // step 2: the keys grouped by word (k_word_histogram and k_word_scatter: the same grid, so that a key's slot is the same in both)
   HIP_TRY(hipMemsetAsync(m.ptr(t.sub), 0, t.sub.bytes(), st));
   const uint32_t key_blocks = (uint32_t)((n + 255) / 256);
   hipLaunchKernelGGL(k_word_histogram, dim3(key_blocks), dim3(256), 0, st, d_words, word_stride, n, m.ptr(t.sub), t.slots, (unsigned long long *)nullptr);
   LoadU32 load;
   load.p = m.ptr(t.sub);
   exclusive_scan(c, load, (long long)t.sub.count, m.ptr(t.cursor), m.ptr(t.total), m.ptr(t.block_sums));
   hipLaunchKernelGGL(k_word_scatter, dim3(key_blocks), dim3(256), 0, st, d_words, word_stride, n, m.ptr(t.cursor), t.slots, m.ptr(t.perm));
   if (timed) HIP_TRY(hipEventRecord(ev[2], st));
   // step 3: the lower median per (word, bit)
   hipLaunchKernelGGL(k_embed_medians, dim3((uint32_t)k), dim3(HS_EMBED_MEDIAN_WAVES * 64), 0, st, (const int32_t *)m.ptr(t.z), (const uint32_t *)m.ptr(t.perm),
                      (const uint32_t *)m.ptr(t.cursor), t.slots, m.ptr(t.tau), m.ptr(t.counts));
   if (timed) HIP_TRY(hipEventRecord(ev[3], st));
   HIP_TRY(hipMemcpyAsync(tau_out, m.ptr(t.tau), t.tau.bytes(), hipMemcpyDeviceToHost, st));
   if (counts_out) HIP_TRY(hipMemcpyAsync(counts_out, m.ptr(t.counts), t.counts.bytes(), hipMemcpyDeviceToHost, st));
   finish_stream(c);
   if (timed)
      for (int q = 0; q < 3; q++) HIP_TRY(hipEventElapsedTime(&c->embed_train_ms[q], ev[q], ev[q + 1]));
}

// the key lists of a new index (not yet the context's) over `total` checked words and their signatures in device memory
void build_key_lists(hesaff_ctx *c, hesaff_ctx::Index &nx, int n_images, const int32_t *counts, const int32_t *d_words, int word_stride,
                     const unsigned long long *d_sigs, int k, int64_t total)
{
   StagePlan persistent;
   nx.ka = key_list_arrays(persistent, k, total);
   nx.keys.ensure(std::max<size_t>(persistent.bytes(), 256));   // (HESAFF_ERR_NOMEM: the context's index is untouched)
   TrainArena m;
   const KeyListBuildArrays b = key_list_build_arrays(m, k);
   const Span<uint32_t> a_starts = m.add<uint32_t>((size_t)n_images + 1);
   m.ensure();
   hipStream_t st = c->stream();
   std::vector<uint32_t> starts((size_t)n_images + 1);
   starts[0] = 0;
   for (int i = 0; i < n_images; i++) starts[(size_t)i + 1] = starts[(size_t)i] + (uint32_t)counts[i];
   HIP_TRY(hipMemcpyAsync(m.ptr(a_starts), starts.data(), starts.size() * 4, hipMemcpyHostToDevice, st));
   HIP_TRY(hipMemsetAsync(m.ptr(b.counts), 0, b.counts.bytes(), st));
   const uint32_t key_blocks = (uint32_t)((total + 255) / 256);
   if (total > 0)
      hipLaunchKernelGGL(k_word_histogram, dim3(key_blocks), dim3(256), 0, st, d_words, word_stride, (int)total, m.ptr(b.counts), 1, (unsigned long long *)nullptr);
   LoadU32 load;
   load.p = m.ptr(b.counts);
   uint32_t *offsets = nx.kptr(nx.ka.offsets);
   exclusive_scan(c, load, (long long)k, offsets, offsets + k, m.ptr(b.block_sums));
   HIP_TRY(hipMemcpyAsync(m.ptr(b.counts), offsets, (size_t)k * 4, hipMemcpyDeviceToDevice, st));   // (the scan has read the counts: now the cursor)
   if (total > 0)
      hipLaunchKernelGGL(k_keylist_scatter, dim3(key_blocks), dim3(256), 0, st, d_words, word_stride, d_sigs, (const uint32_t *)m.ptr(a_starts), n_images,
                         (uint32_t)total, m.ptr(b.counts), nx.kptr(nx.ka.sig), nx.kptr(nx.ka.image));
   finish_stream(c);   // (the scratch and `starts` go with this frame)
   nx.embedded = true;
}

// the embedded query over n checked words and their signatures in device memory; the ranked result goes to the caller's arrays
void query_embedded_on_device(hesaff_ctx *c, int n, const int32_t *d_words, int word_stride, const unsigned long long *d_sigs, int threshold, int top,
                              int32_t *images_out, double *scores_out, int *count_out)
{
   hesaff_ctx::Index &ix = c->index;
   hipStream_t st = c->stream();
   const bool timed = c->profiling >= 1;
   DevEvent ev[2];
   if (timed) for (DevEvent &e : ev) e = DevEvent(hipEventDefault);
   IndexResultHead *head = ix.ptr(ix.a.head);
   if (timed) HIP_TRY(hipEventRecord(ev[0], st));
   HIP_TRY(hipMemsetAsync(ix.ptr(ix.a.dot), 0, ix.a.dot.bytes(), st));
   HIP_TRY(hipMemsetAsync(head, 0, sizeof(IndexResultHead), st));
   if (n > 0) {
      hipLaunchKernelGGL(k_query_count, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, d_words, word_stride, n, ix.ptr(ix.a.tfq));
      hipLaunchKernelGGL(k_query_score_embedded, dim3((uint32_t)((n + 3) / 4)), dim3(256), 0, st, d_words, word_stride, d_sigs, n, threshold, ix.ptr(ix.a.tfq),
                         (const uint32_t *)ix.ptr(ix.a.idf), (const uint32_t *)ix.kptr(ix.ka.offsets), (const unsigned long long *)ix.kptr(ix.ka.sig),
                         (const uint32_t *)ix.kptr(ix.ka.image), ix.ptr(ix.a.dot), head);
   }
   hipLaunchKernelGGL(k_query_finish, dim3((uint32_t)((ix.n_images + 255) / 256)), dim3(256), 0, st, (const unsigned long long *)ix.ptr(ix.a.dot),
                      (const unsigned long long *)ix.ptr(ix.a.norm2), (const IndexResultHead *)head, ix.n_images, ix.ptr(ix.a.score));
   hipLaunchKernelGGL(k_index_select, dim3(1), dim3(HS_ISEL_THREADS), 0, st, (const double *)ix.ptr(ix.a.score), ix.n_images, top, ix.ptr(ix.a.top_images), ix.ptr(ix.a.top_scores), head);
   if (timed) HIP_TRY(hipEventRecord(ev[1], st));
   const int count = std::min(top, ix.n_images);
   char *h = (char *)c->h_small_end.ensure_small((size_t)HS_INDEX_MAX_TOP * 12);
   HIP_TRY(hipMemcpyAsync(h, ix.ptr(ix.a.top_scores), (size_t)count * 8, hipMemcpyDeviceToHost, st));
   HIP_TRY(hipMemcpyAsync(h + (size_t)HS_INDEX_MAX_TOP * 8, ix.ptr(ix.a.top_images), (size_t)count * 4, hipMemcpyDeviceToHost, st));
   finish_stream(c);
   c->index_ms[2] = 0.0f;
   if (timed) HIP_TRY(hipEventElapsedTime(&c->index_ms[2], ev[0], ev[1]));
   memcpy(scores_out, h, (size_t)count * 8);
   memcpy(images_out, h + (size_t)HS_INDEX_MAX_TOP * 8, (size_t)count * 4);
   *count_out = count;
}

bool embed_source_ok(int64_t n, const void *d_desc, int64_t stride, int64_t offset)
{
   return n >= 0 && (n == 0 || d_desc) && word_source_ok(stride, offset) && (uintptr_t)d_desc % 4 == 0 && n <= ((int64_t)1 << 38);
}

} // namespace

extern "C" {

int hesaff_set_embedding(hesaff_ctx *c, const int8_t *P, const int32_t *tau)
{
   if (!c || (P == nullptr) != (tau == nullptr)) return HESAFF_ERR_ARG;
   if (P && (c->vocab.k == 0 || !embed_projection_ok(P))) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   hesaff_ctx::Embedding e;
   if (P) {
      StagePlan plan;
      e.a = embed_arrays(plan, c->vocab.k);
      e.buf.ensure(plan.bytes());   // (throws HESAFF_ERR_NOMEM with the context's embedding untouched)
      std::vector<uint8_t> tiles(HS_EMBED_P_BYTES);
      int32_t bias[HS_EMBED_BITS];
      embed_pack_projection(P, tiles.data(), bias);
      HIP_TRY(hipMemcpy(e.ptr(e.a.tiles), tiles.data(), tiles.size(), hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(e.ptr(e.a.bias), bias, sizeof bias, hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(e.ptr(e.a.tau), tau, e.a.tau.bytes(), hipMemcpyHostToDevice));
      e.P.assign(P, P + HS_EMBED_P_BYTES);
      e.k = c->vocab.k;
      e.set = true;
   }
   HIP_TRY(hipStreamSynchronize(c->stream()));   // nothing still reads the embedding that goes
   c->embed = std::move(e);
   if (!c->embed.set) c->b_sigs.release();
   c->sig_spans.clear();
   c->sigs_device_total = -1;
   c->embed_timed = false;
   HS_API_END(c)
}

int hesaff_get_embedding(const hesaff_ctx *c, int *k, int8_t *P, int32_t *tau)
{
   if (!c || !k) return HESAFF_ERR_ARG;
   *k = c->embed.set ? c->embed.k : 0;
   if (!c->embed.set || (!P && !tau)) return HESAFF_OK;
   hesaff_ctx *m = const_cast<hesaff_ctx *>(c);   // (the error string is the context's)
   HS_API_BEGIN
   bind_device(m);
   if (P) memcpy(P, c->embed.P.data(), HS_EMBED_P_BYTES);
   if (tau) HIP_TRY(hipMemcpy(tau, c->embed.ptr(c->embed.a.tau), c->embed.a.tau.bytes(), hipMemcpyDeviceToHost));
   HS_API_END(m)
}

int hesaff_get_signatures(const hesaff_ctx *c, int image, const uint64_t **sigs, int *count)
{
   if (!c || !sigs || !count || !c->embed.set) return HESAFF_ERR_ARG;
   if (image < 0 || (size_t)image >= c->sig_spans.size() || c->sig_spans[(size_t)image].n < 0) return HESAFF_ERR_ARG;
   *sigs = c->sig_spans[(size_t)image].p;
   *count = c->sig_spans[(size_t)image].n;
   return HESAFF_OK;
}

int hesaff_get_signatures_device(const hesaff_ctx *c, const void **d_sigs, int64_t *total)
{
   if (!c || !d_sigs || !total || !c->embed.set || c->sigs_device_total < 0) return HESAFF_ERR_ARG;
   *d_sigs = c->sigs_device_total > 0 ? c->b_sigs.p : nullptr;
   *total = c->sigs_device_total;
   return HESAFF_OK;
}

int hesaff_embed_device(hesaff_ctx *c, int64_t n, const void *d_desc, int64_t stride, int64_t offset, const void *d_words, int word_stride, void *d_sigs_out)
{
   if (!c || !embed_source_ok(n, d_desc, stride, offset) || !index_word_stride_ok(word_stride)) return HESAFF_ERR_ARG;
   if ((n > 0 && (!d_words || !d_sigs_out)) || (uintptr_t)d_words % 4 != 0 || (uintptr_t)d_sigs_out % 8 != 0) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   need_vocabulary(c);
   need_embedding(c);
   bind_device(c);
   check_device_words(c, (const int32_t *)d_words, word_stride, (long long)n, c->embed.k, "hesaff_embed_device");
   launch_embed_keys(c, d_desc, (long long)n, (long long)stride, (long long)offset, (const int32_t *)d_words, word_stride, d_sigs_out);
   finish_stream(c);
   HS_API_END(c)
}

int hesaff_stage_embed(hesaff_ctx *c, int n, const uint8_t *desc, const int32_t *words, int word_stride, uint64_t *sigs_out)
{
   if (!c || n < 0 || !index_word_stride_ok(word_stride) || (n > 0 && (!desc || !words || !sigs_out))) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   need_vocabulary(c);
   need_embedding(c);
   std::vector<int32_t> packed;
   if (!stage_words(words, word_stride, n, c->embed.k, packed)) throw HsError(HESAFF_ERR_ARG, "hesaff_stage_embed: a word lies outside 0 .. vocabulary_size - 1");
   bind_device(c);
   if (n == 0) return HESAFF_OK;
   const size_t N = (size_t)n;
   StageArena a(c);
   const Span<uint8_t> a_desc = a.add<uint8_t>(N * 128);
   const Span<int32_t> a_words = a.add<int32_t>(N);
   const Span<uint64_t> a_out = a.add<uint64_t>(N);
   a.ensure();
   a.upload(a_desc, desc);
   a.upload(a_words, (const int32_t *)packed.data());
   launch_embed_keys(c, a.ptr(a_desc), n, 128, 0, a.ptr(a_words), 1, a.ptr(a_out));
   a.download(sigs_out, a_out);
   finish_stream(c);
   HS_API_END(c)
}

// the test seam: z[n][64] = P . d of the caller's descriptors, by the kernel that makes the signatures
int hesaff_stage_project(hesaff_ctx *c, int n, const uint8_t *desc, const int8_t *P, int32_t *z_out)
{
   if (!c || n < 0 || !embed_projection_ok(P) || (n > 0 && (!desc || !z_out))) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   if (n == 0) return HESAFF_OK;
   const size_t N = (size_t)n;
   StageArena a(c);
   const Span<uint8_t> a_desc = a.add<uint8_t>(N * 128), a_tiles = a.add<uint8_t>(HS_EMBED_P_BYTES);
   const Span<int32_t> a_bias = a.add<int32_t>((size_t)HS_EMBED_BITS), a_z = a.add<int32_t>(N * HS_EMBED_BITS);
   a.ensure();
   std::vector<uint8_t> tiles(HS_EMBED_P_BYTES);
   int32_t bias[HS_EMBED_BITS];
   embed_pack_projection(P, tiles.data(), bias);
   a.upload(a_desc, desc);
   a.upload(a_tiles, (const uint8_t *)tiles.data());
   a.upload(a_bias, (const int32_t *)bias);
   project_on_device(c->stream(), a.ptr(a_tiles), a.ptr(a_bias), a.ptr(a_desc), n, 128, 0, a.ptr(a_z));
   a.download(z_out, a_z);
   finish_stream(c);
   HS_API_END(c)
}

int hesaff_train_embedding_device(hesaff_ctx *c, int64_t n, const void *d_desc, int64_t stride, int64_t offset, const void *d_words, int word_stride, int k,
                                  const int8_t *P, int32_t *tau_out, uint32_t *counts_out)
{
   if (!c || !d_desc || !d_words || !tau_out || !embed_train_counts_ok(n, k) || !embed_projection_ok(P)) return HESAFF_ERR_ARG;
   if (!word_source_ok(stride, offset) || !index_word_stride_ok(word_stride) || (uintptr_t)d_desc % 4 != 0 || (uintptr_t)d_words % 4 != 0) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   check_device_words(c, (const int32_t *)d_words, word_stride, (long long)n, k, "hesaff_train_embedding_device");
   train_embedding_on_device(c, (int)n, (const uint8_t *)d_desc, (long long)stride, (long long)offset, (const int32_t *)d_words, word_stride, k, P, tau_out, counts_out);
   HS_API_END(c)
}

int hesaff_train_embedding(hesaff_ctx *c, int64_t n, const uint8_t *desc, const int32_t *words, int word_stride, int k, const int8_t *P, int32_t *tau_out,
                           uint32_t *counts_out)
{
   if (!c || !desc || !words || !tau_out || !embed_train_counts_ok(n, k) || !embed_projection_ok(P) || !index_word_stride_ok(word_stride)) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   std::vector<int32_t> packed;
   if (!stage_words(words, word_stride, n, k, packed)) throw HsError(HESAFF_ERR_ARG, "hesaff_train_embedding: a word lies outside 0 .. k - 1");
   bind_device(c);
   DevBuf d, w;
   d.ensure((size_t)n * 128);
   w.ensure(std::max<size_t>((size_t)n * 4, 256));
   HIP_TRY(hipMemcpyAsync(d.p, desc, (size_t)n * 128, hipMemcpyHostToDevice, c->stream()));
   HIP_TRY(hipMemcpyAsync(w.p, packed.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream()));
   train_embedding_on_device(c, (int)n, d.as<uint8_t>(), 128, 0, w.as<int32_t>(), 1, k, P, tau_out, counts_out);
   HS_API_END(c)
}

// embed_ms: the last k_embed_keys launch of a batch or of hesaff_embed_device; the other three: the last threshold training
int hesaff_get_embedding_ms(const hesaff_ctx *c, float *embed_ms, float *project_ms, float *group_ms, float *median_ms)
{
   if (!c || !embed_ms || !project_ms || !group_ms || !median_ms) return HESAFF_ERR_ARG;
   *embed_ms = 0.0f;
   *project_ms = c->embed_train_ms[0]; *group_ms = c->embed_train_ms[1]; *median_ms = c->embed_train_ms[2];
   if (!c->embed_timed) return HESAFF_OK;
   if (hipEventSynchronize(c->ev_embed[1]) != hipSuccess || hipEventElapsedTime(embed_ms, c->ev_embed[0], c->ev_embed[1]) != hipSuccess) {
      (void)hipGetLastError();
      *embed_ms = 0.0f;
   }
   return HESAFF_OK;
}

int hesaff_index_build_embedded_device(hesaff_ctx *c, int n_images, const int32_t *counts, const void *d_words, int word_stride, const void *d_sigs,
                                       int vocabulary_size)
{
   if (!c || !counts || !index_counts_ok(n_images, vocabulary_size) || !index_word_stride_ok(word_stride)) return HESAFF_ERR_ARG;
   const int64_t total = index_total_keys(counts, n_images);
   if (total < 0 || (total > 0 && (!d_words || !d_sigs)) || (uintptr_t)d_words % 4 != 0 || (uintptr_t)d_sigs % 8 != 0) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   check_device_words(c, (const int32_t *)d_words, word_stride, (long long)total, vocabulary_size, "hesaff_index_build_embedded_device");
   build_index_on_device(c, n_images, counts, (const int32_t *)d_words, word_stride, vocabulary_size, total, (const unsigned long long *)d_sigs, true);
   HS_API_END(c)
}

int hesaff_index_build_embedded(hesaff_ctx *c, int n_images, const int32_t *counts, const int32_t *words, int word_stride, const uint64_t *sigs,
                                int vocabulary_size)
{
   if (!c || !counts || !index_counts_ok(n_images, vocabulary_size) || !index_word_stride_ok(word_stride)) return HESAFF_ERR_ARG;
   const int64_t total = index_total_keys(counts, n_images);
   if (total < 0 || (total > 0 && (!words || !sigs))) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   std::vector<int32_t> packed;
   if (!stage_words(words, word_stride, total, vocabulary_size, packed)) throw HsError(HESAFF_ERR_ARG, "hesaff_index_build_embedded: a word lies outside 0 .. vocabulary_size - 1");
   bind_device(c);
   DevBuf d, g;
   d.ensure(std::max<size_t>((size_t)total * 4, 256));
   g.ensure(std::max<size_t>((size_t)total * 8, 256));
   if (total > 0) {
      HIP_TRY(hipMemcpyAsync(d.p, packed.data(), (size_t)total * 4, hipMemcpyHostToDevice, c->stream()));
      HIP_TRY(hipMemcpyAsync(g.p, sigs, (size_t)total * 8, hipMemcpyHostToDevice, c->stream()));
   }
   build_index_on_device(c, n_images, counts, d.as<int32_t>(), 1, vocabulary_size, total, g.as<unsigned long long>(), true);
   HS_API_END(c)
}

int hesaff_index_query_embedded_device(hesaff_ctx *c, int n, const void *d_words, int word_stride, const void *d_sigs, int hamming, int top,
                                       int32_t *images_out, double *scores_out, int *count_out)
{
   if (!c || !images_out || !scores_out || !count_out || !index_query_ok(n, top) || !index_word_stride_ok(word_stride) || !embed_threshold_ok(hamming)) return HESAFF_ERR_ARG;
   if ((n > 0 && (!d_words || !d_sigs)) || (uintptr_t)d_words % 4 != 0 || (uintptr_t)d_sigs % 8 != 0 || !c->index.built || !c->index.embedded) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   check_device_words(c, (const int32_t *)d_words, word_stride, n, c->index.k, "hesaff_index_query_embedded_device");
   query_embedded_on_device(c, n, (const int32_t *)d_words, word_stride, (const unsigned long long *)d_sigs, hamming, top, images_out, scores_out, count_out);
   HS_API_END(c)
}

int hesaff_index_query_embedded(hesaff_ctx *c, int n, const int32_t *words, int word_stride, const uint64_t *sigs, int hamming, int top, int32_t *images_out,
                                double *scores_out, int *count_out)
{
   if (!c || !images_out || !scores_out || !count_out || !index_query_ok(n, top) || !index_word_stride_ok(word_stride) || !embed_threshold_ok(hamming)) return HESAFF_ERR_ARG;
   if ((n > 0 && (!words || !sigs)) || !c->index.built || !c->index.embedded) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   std::vector<int32_t> packed;
   if (!stage_words(words, word_stride, n, c->index.k, packed)) throw HsError(HESAFF_ERR_ARG, "hesaff_index_query_embedded: a word lies outside 0 .. vocabulary_size - 1");
   bind_device(c);
   c->index.qwords.ensure(std::max<size_t>((size_t)n * 4, 256));
   c->index.qsigs.ensure(std::max<size_t>((size_t)n * 8, 256));
   if (n > 0) {
      HIP_TRY(hipMemcpyAsync(c->index.qwords.p, packed.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream()));
      HIP_TRY(hipMemcpyAsync(c->index.qsigs.p, sigs, (size_t)n * 8, hipMemcpyHostToDevice, c->stream()));
   }
   query_embedded_on_device(c, n, c->index.qwords.as<int32_t>(), 1, c->index.qsigs.as<unsigned long long>(), hamming, top, images_out, scores_out, count_out);
   HS_API_END(c)
}

// *embedded: whether the index holds key lists; offsets[K + 1], and per entry of the lists its image and its signature (each may be
// NULL; the order inside a list is unspecified)
int hesaff_index_get_embedded(const hesaff_ctx *c, int *embedded, uint32_t *offsets, uint32_t *images, uint64_t *sigs)
{
   if (!c || !embedded || !c->index.built) return HESAFF_ERR_ARG;
   *embedded = c->index.embedded ? 1 : 0;
   if (!c->index.embedded) return (offsets || images || sigs) ? HESAFF_ERR_ARG : HESAFF_OK;
   hesaff_ctx *m = const_cast<hesaff_ctx *>(c);
   HS_API_BEGIN
   bind_device(m);
   const hesaff_ctx::Index &ix = c->index;
   const size_t total = (size_t)ix.n_keys;
   if (offsets) HIP_TRY(hipMemcpy(offsets, ix.kptr(ix.ka.offsets), ((size_t)ix.k + 1) * 4, hipMemcpyDeviceToHost));
   if (images && total) HIP_TRY(hipMemcpy(images, ix.kptr(ix.ka.image), total * 4, hipMemcpyDeviceToHost));
   if (sigs && total) HIP_TRY(hipMemcpy(sigs, ix.kptr(ix.ka.sig), total * 8, hipMemcpyDeviceToHost));
   HS_API_END(m)
}

} // extern "C"
