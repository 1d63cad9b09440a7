// capi_embed.h -- Hamming embedding (hesaff_set_embedding, hesaff_embed_device, hesaff_train_embedding*, hesaff_index_build_embedded*,
// hesaff_index_query_embedded* and the getters declared with them in include/hesaff_amd.h): the entry points over the kernels of
// kernels_embed.h, with every number from embed_plan.h.  Included at the end of pipeline.hip, behind capi_verify.h (same translation
// unit).  The index forms are entry points alone: staging, build, key lists and the query driver are capi_index.h's, which the plain
// forms share.  The embedding is context state beside the vocabulary (hesaff_ctx::embed); a context without one allocates, launches
// and copies nothing here, and its assignment, its index and its queries are those of a context that never had one.
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
   DevBuf none;
   const DeviceWords w = stage_source(c, {"hesaff_embed_device", true, d_words, word_stride, n, nullptr, false}, c->embed.k, none);
   launch_embed_keys(c, d_desc, (long long)n, (long long)stride, (long long)offset, w.d_words, w.word_stride, d_sigs_out);
   finish_stream(c);
   HS_API_END(c)
}

int hesaff_stage_embed(hesaff_ctx *c, int n, const uint8_t *desc, const int32_t *words, int word_stride, uint64_t *sigs_out)
{
   if (!c || n < 0 || !index_word_stride_ok(word_stride) || (n > 0 && (!desc || !words || !sigs_out))) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   need_vocabulary(c);
   need_embedding(c);
   std::vector<int32_t> packed;   // (into the stage arena with the descriptors, not into a buffer of their own: the check alone is shared)
   pack_host_words({"hesaff_stage_embed", false, words, word_stride, n, nullptr, false}, c->embed.k, packed);
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
   DevBuf none;
   const DeviceWords w = stage_source(c, {"hesaff_train_embedding_device", true, d_words, word_stride, n, nullptr, false}, k, none);
   train_embedding_on_device(c, (int)n, (const uint8_t *)d_desc, (long long)stride, (long long)offset, w.d_words, w.word_stride, k, P, tau_out, counts_out);
   HS_API_END(c)
}

int hesaff_train_embedding(hesaff_ctx *c, int64_t n, const uint8_t *desc, const int32_t *words, int word_stride, int k, const int8_t *P, int32_t *tau_out,
                           uint32_t *counts_out)
{
   if (!c || !desc || !words || !tau_out || !embed_train_counts_ok(n, k) || !embed_projection_ok(P) || !index_word_stride_ok(word_stride)) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   DevBuf d, g;
   const DeviceWords w = stage_source(c, {"hesaff_train_embedding", false, words, word_stride, n, nullptr, false, "k"}, k, g);
   d.ensure((size_t)n * 128);
   HIP_TRY(hipMemcpyAsync(d.p, desc, (size_t)n * 128, hipMemcpyHostToDevice, c->stream()));
   train_embedding_on_device(c, (int)n, d.as<uint8_t>(), 128, 0, w.d_words, w.word_stride, k, P, tau_out, counts_out);
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
   return build_from(c, n_images, counts, {"hesaff_index_build_embedded_device", true, d_words, word_stride, 0, d_sigs, true}, vocabulary_size);
}

int hesaff_index_build_embedded(hesaff_ctx *c, int n_images, const int32_t *counts, const int32_t *words, int word_stride, const uint64_t *sigs,
                                int vocabulary_size)
{
   return build_from(c, n_images, counts, {"hesaff_index_build_embedded", false, words, word_stride, 0, sigs, true}, vocabulary_size);
}

int hesaff_index_query_embedded_device(hesaff_ctx *c, int n, const void *d_words, int word_stride, const void *d_sigs, int hamming, int top,
                                       int32_t *images_out, double *scores_out, int *count_out)
{
   return query_from(c, {"hesaff_index_query_embedded_device", true, d_words, word_stride, n, d_sigs, true}, hamming, top, images_out, scores_out, count_out);
}

int hesaff_index_query_embedded(hesaff_ctx *c, int n, const int32_t *words, int word_stride, const uint64_t *sigs, int hamming, int top, int32_t *images_out,
                                double *scores_out, int *count_out)
{
   return query_from(c, {"hesaff_index_query_embedded", false, words, word_stride, n, sigs, true}, hamming, top, images_out, scores_out, count_out);
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
