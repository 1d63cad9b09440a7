// capi_index.h -- the image index (hesaff_index_* and hesaff_get_index_ms of include/hesaff_amd.h): the build and the query over the
// kernels of kernels_index.h, with every number from index_plan.h.  Included at the end of pipeline.hip, behind capi_train.h (same
// translation unit).  The index is context state (hesaff_ctx::index); a build works on a new one and installs it when it is whole, so
// a refused or failed call leaves the previous index as it was, and a context that never builds one allocates, launches and copies
// nothing here.
#pragma once

namespace {

uint32_t grid_for(unsigned long long items, uint32_t cap = 1u << 16) { return (uint32_t)std::max<unsigned long long>(1, std::min<unsigned long long>((items + 255) / 256, cap)); }

// the read-only check of the device forms: a word outside 0 .. k - 1 is HESAFF_ERR_ARG before anything is built or scored
void check_device_words(hesaff_ctx *c, const int32_t *d_words, int word_stride, long long n, int k, const char *who)
{
   if (n == 0) return;
   DevBuf flag;
   flag.ensure(256);
   hipStream_t st = c->stream();
   HIP_TRY(hipMemsetAsync(flag.p, 0, 4, st));
   hipLaunchKernelGGL(k_index_check_words, dim3(grid_for((unsigned long long)n, 4096)), dim3(256), 0, st, d_words, word_stride, n, k, flag.as<uint32_t>());
   uint32_t *h = (uint32_t *)c->h_small_end.ensure_small(4);
   HIP_TRY(hipMemcpyAsync(h, flag.p, 4, hipMemcpyDeviceToHost, st));
   finish_stream(c);
   if (*h) throw HsError(HESAFF_ERR_ARG, std::string(who) + ": a word lies outside 0 .. vocabulary_size - 1");
}

// words in host memory -> packed, checked against 0 .. k - 1 on the way (false: one lies outside)
bool stage_words(const int32_t *words, int word_stride, int64_t n, int k, std::vector<int32_t> &out)
{
   out.resize((size_t)n);
   for (int64_t j = 0; j < n; j++) {
      const int32_t w = words[j * word_stride];
      if (w < 0 || w >= k) return false;
      out[(size_t)j] = w;
   }
   return true;
}

// the key lists of an embedded build (capi_embed.h), made in the new index before it becomes the context's
void build_key_lists(hesaff_ctx *c, hesaff_ctx::Index &nx, int n_images, const int32_t *counts, const int32_t *d_words, int word_stride,
                     const unsigned long long *d_sigs, int k, int64_t total);

// the build over `total` checked words in device memory (arguments checked by the caller); embedded: with the key lists of
// hesaff_index_build_embedded over the signatures at d_sigs, behind the plain build's steps, which are the same either way
void build_index_on_device(hesaff_ctx *c, int n_images, const int32_t *counts, const int32_t *d_words, int word_stride, int k, int64_t total,
                           const unsigned long long *d_sigs = nullptr, bool embedded = false)
{
   hesaff_ctx::Index nx;
   StagePlan persistent;
   nx.a = index_arrays(persistent, n_images, k);
   nx.tables.ensure(std::max<size_t>(persistent.bytes(), 256));   // (HESAFF_ERR_NOMEM: the context's index is untouched)
   TrainArena m;   // the scratch of the call, released when it returns
   const IndexBuildArrays b = index_build_arrays(m, n_images, k, total);
   m.ensure();
   hipStream_t st = c->stream();
   const bool timed = c->profiling >= 1;
   DevEvent ev[3];
   if (timed) for (DevEvent &e : ev) e = DevEvent(hipEventDefault);
   std::vector<uint32_t> starts((size_t)n_images + 1);
   starts[0] = 0;
   for (int i = 0; i < n_images; i++) starts[(size_t)i + 1] = starts[(size_t)i] + (uint32_t)counts[i];
   HIP_TRY(hipMemcpyAsync(m.ptr(b.starts), starts.data(), starts.size() * 4, hipMemcpyHostToDevice, st));
   HIP_TRY(hipMemsetAsync(nx.tables.p, 0, persistent.bytes(), st));   // df, norm2, tfq, dot, score and the head start at zero
   HIP_TRY(hipMemsetAsync(m.ptr(b.hash_keys), 0xFF, b.hash_keys.bytes(), st));
   HIP_TRY(hipMemsetAsync(m.ptr(b.hash_tf), 0, b.hash_tf.bytes(), st));
   // step 1: the distinct (image, word) pairs and their tf
   if (timed) HIP_TRY(hipEventRecord(ev[0], st));
   if (total > 0)
      hipLaunchKernelGGL(k_index_insert, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, st, d_words, word_stride, (const uint32_t *)m.ptr(b.starts), n_images,
                         (uint32_t)total, b.bits, m.ptr(b.hash_keys), m.ptr(b.hash_tf));
   if (timed) HIP_TRY(hipEventRecord(ev[1], st));
   // step 2: df, idf, the list offsets; then the lists and the norms in a second pass over the table
   const uint32_t slot_grid = grid_for(b.slots);
   hipLaunchKernelGGL(k_index_df, dim3(slot_grid), dim3(256), 0, st, (const unsigned long long *)m.ptr(b.hash_keys), (unsigned long long)b.slots, nx.ptr(nx.a.df));
   hipLaunchKernelGGL(k_index_idf, dim3((uint32_t)((k + 255) / 256)), dim3(256), 0, st, (const uint32_t *)nx.ptr(nx.a.df), k, n_images, nx.ptr(nx.a.idf));
   LoadU32 load;
   load.p = nx.ptr(nx.a.df);
   exclusive_scan(c, load, (long long)k, nx.ptr(nx.a.offsets), nx.ptr(nx.a.offsets) + k, m.ptr(b.block_sums));
   HIP_TRY(hipMemcpyAsync(m.ptr(b.cursor), nx.ptr(nx.a.offsets), (size_t)k * 4, hipMemcpyDeviceToDevice, st));
   uint32_t *h_postings = (uint32_t *)c->h_small_end.ensure_small(4);
   HIP_TRY(hipMemcpyAsync(h_postings, nx.ptr(nx.a.offsets) + k, 4, hipMemcpyDeviceToHost, st));
   finish_stream(c);
   const int64_t n_postings = (int64_t)*h_postings;
   if (n_postings > total) throw HsError(HESAFF_ERR_DEVICE, "hesaff_index_build: more postings than keys");
   nx.lists.ensure(index_lists_bytes(n_postings));
   hipLaunchKernelGGL(k_index_postings, dim3(slot_grid), dim3(256), 0, st, (const unsigned long long *)m.ptr(b.hash_keys), (const uint32_t *)m.ptr(b.hash_tf),
                      (unsigned long long)b.slots, (const uint32_t *)nx.ptr(nx.a.idf), m.ptr(b.cursor), nx.lists.as<IndexPosting>(), nx.ptr(nx.a.norm2));
   if (timed) HIP_TRY(hipEventRecord(ev[2], st));
   finish_stream(c);
   c->index_ms[0] = c->index_ms[1] = c->index_ms[2] = 0.0f;
   if (timed) {
      HIP_TRY(hipEventElapsedTime(&c->index_ms[0], ev[0], ev[1]));
      HIP_TRY(hipEventElapsedTime(&c->index_ms[1], ev[1], ev[2]));
   }
   nx.n_images = n_images; nx.k = k; nx.n_keys = total; nx.n_postings = n_postings; nx.built = true;
   if (embedded) build_key_lists(c, nx, n_images, counts, d_words, word_stride, d_sigs, k, total);
   c->index = std::move(nx);
}

// the query over n checked words in device memory; the ranked result goes to the caller's arrays
void query_index_on_device(hesaff_ctx *c, int n, const int32_t *d_words, int word_stride, int top, int32_t *images_out, double *scores_out, int *count_out)
{
   hesaff_ctx::Index &ix = c->index;
   hipStream_t st = c->stream();
   const bool timed = c->profiling >= 1;
   DevEvent ev[2];
   if (timed) for (DevEvent &e : ev) e = DevEvent(hipEventDefault);
   IndexResultHead *head = ix.ptr(ix.a.head);
   if (timed) HIP_TRY(hipEventRecord(ev[0], st));
   HIP_TRY(hipMemsetAsync(ix.ptr(ix.a.dot), 0, ix.a.dot.bytes(), st));   // the last query's values were readable until now
   HIP_TRY(hipMemsetAsync(head, 0, sizeof(IndexResultHead), st));
   if (n > 0) {
      hipLaunchKernelGGL(k_query_count, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, d_words, word_stride, n, ix.ptr(ix.a.tfq));
      hipLaunchKernelGGL(k_query_score, dim3((uint32_t)((n + 3) / 4)), dim3(256), 0, st, d_words, word_stride, n, ix.ptr(ix.a.tfq), (const uint32_t *)ix.ptr(ix.a.idf),
                         (const uint32_t *)ix.ptr(ix.a.offsets), (const IndexPosting *)ix.lists.as<IndexPosting>(), ix.ptr(ix.a.dot), head);
   }
   hipLaunchKernelGGL(k_query_finish, dim3((uint32_t)((ix.n_images + 255) / 256)), dim3(256), 0, st, (const unsigned long long *)ix.ptr(ix.a.dot),
                      (const unsigned long long *)ix.ptr(ix.a.norm2), (const IndexResultHead *)head, ix.n_images, ix.ptr(ix.a.score));
   hipLaunchKernelGGL(k_index_select, dim3(1), dim3(HS_ISEL_THREADS), 0, st, (const double *)ix.ptr(ix.a.score), ix.n_images, top, ix.ptr(ix.a.top_images), ix.ptr(ix.a.top_scores), head);
   if (timed) HIP_TRY(hipEventRecord(ev[1], st));
   // the ranked result alone crosses to the host: min(top, N) x 12 bytes
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

} // namespace

extern "C" {

int hesaff_index_build_device(hesaff_ctx *c, int n_images, const int32_t *counts, const void *d_words, int word_stride, int vocabulary_size)
{
   if (!c || !counts || !index_counts_ok(n_images, vocabulary_size) || !index_word_stride_ok(word_stride)) return HESAFF_ERR_ARG;
   const int64_t total = index_total_keys(counts, n_images);
   if (total < 0 || (total > 0 && !d_words) || (uintptr_t)d_words % 4 != 0) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   check_device_words(c, (const int32_t *)d_words, word_stride, (long long)total, vocabulary_size, "hesaff_index_build_device");
   build_index_on_device(c, n_images, counts, (const int32_t *)d_words, word_stride, vocabulary_size, total);
   HS_API_END(c)
}

int hesaff_index_build(hesaff_ctx *c, int n_images, const int32_t *counts, const int32_t *words, int word_stride, int vocabulary_size)
{
   if (!c || !counts || !index_counts_ok(n_images, vocabulary_size) || !index_word_stride_ok(word_stride)) return HESAFF_ERR_ARG;
   const int64_t total = index_total_keys(counts, n_images);
   if (total < 0 || (total > 0 && !words)) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   std::vector<int32_t> packed;
   if (!stage_words(words, word_stride, total, vocabulary_size, packed)) throw HsError(HESAFF_ERR_ARG, "hesaff_index_build: a word lies outside 0 .. vocabulary_size - 1");
   bind_device(c);
   DevBuf d;
   d.ensure(std::max<size_t>((size_t)total * 4, 256));
   if (total > 0) HIP_TRY(hipMemcpyAsync(d.p, packed.data(), (size_t)total * 4, hipMemcpyHostToDevice, c->stream()));
   build_index_on_device(c, n_images, counts, d.as<int32_t>(), 1, vocabulary_size, total);
   HS_API_END(c)
}

int hesaff_index_query_device(hesaff_ctx *c, int n, const void *d_words, int word_stride, int top, int32_t *images_out, double *scores_out, int *count_out)
{
   if (!c || !images_out || !scores_out || !count_out || !index_query_ok(n, top) || !index_word_stride_ok(word_stride)) return HESAFF_ERR_ARG;
   if ((n > 0 && !d_words) || (uintptr_t)d_words % 4 != 0 || !c->index.built) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   check_device_words(c, (const int32_t *)d_words, word_stride, n, c->index.k, "hesaff_index_query_device");
   query_index_on_device(c, n, (const int32_t *)d_words, word_stride, top, images_out, scores_out, count_out);
   HS_API_END(c)
}

int hesaff_index_query(hesaff_ctx *c, int n, const int32_t *words, int word_stride, int top, int32_t *images_out, double *scores_out, int *count_out)
{
   if (!c || !images_out || !scores_out || !count_out || !index_query_ok(n, top) || !index_word_stride_ok(word_stride)) return HESAFF_ERR_ARG;
   if ((n > 0 && !words) || !c->index.built) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   std::vector<int32_t> packed;
   if (!stage_words(words, word_stride, n, c->index.k, packed)) throw HsError(HESAFF_ERR_ARG, "hesaff_index_query: a word lies outside 0 .. vocabulary_size - 1");
   bind_device(c);
   c->index.qwords.ensure(std::max<size_t>((size_t)n * 4, 256));
   if (n > 0) HIP_TRY(hipMemcpyAsync(c->index.qwords.p, packed.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream()));
   query_index_on_device(c, n, c->index.qwords.as<int32_t>(), 1, top, images_out, scores_out, count_out);
   HS_API_END(c)
}

int hesaff_index_get_scores(const hesaff_ctx *c, uint64_t *dots, double *scores, uint64_t *query_norm2)
{
   if (!c || !c->index.built) return HESAFF_ERR_ARG;
   hesaff_ctx *m = const_cast<hesaff_ctx *>(c);   // (the error string and the stream are the context's)
   HS_API_BEGIN
   bind_device(m);
   const hesaff_ctx::Index &ix = c->index;
   const size_t n = (size_t)ix.n_images;
   if (dots) HIP_TRY(hipMemcpy(dots, ix.tables.at<char>(ix.a.dot.off), n * 8, hipMemcpyDeviceToHost));
   if (scores) HIP_TRY(hipMemcpy(scores, ix.tables.at<char>(ix.a.score.off), n * 8, hipMemcpyDeviceToHost));
   if (query_norm2) HIP_TRY(hipMemcpy(query_norm2, ix.tables.at<char>(ix.a.head.off), 8, hipMemcpyDeviceToHost));
   HS_API_END(m)
}

int hesaff_index_get_tables(const hesaff_ctx *c, uint32_t *df, uint32_t *idf, uint64_t *norm2)
{
   if (!c || !c->index.built) return HESAFF_ERR_ARG;
   hesaff_ctx *m = const_cast<hesaff_ctx *>(c);
   HS_API_BEGIN
   bind_device(m);
   const hesaff_ctx::Index &ix = c->index;
   if (df) HIP_TRY(hipMemcpy(df, ix.tables.at<char>(ix.a.df.off), (size_t)ix.k * 4, hipMemcpyDeviceToHost));
   if (idf) HIP_TRY(hipMemcpy(idf, ix.tables.at<char>(ix.a.idf.off), (size_t)ix.k * 4, hipMemcpyDeviceToHost));
   if (norm2) HIP_TRY(hipMemcpy(norm2, ix.tables.at<char>(ix.a.norm2.off), (size_t)ix.n_images * 8, hipMemcpyDeviceToHost));
   HS_API_END(m)
}

int hesaff_index_get_info(const hesaff_ctx *c, int *n_images, int *vocabulary_size, int64_t *n_keys, int64_t *n_postings)
{
   if (!c || !c->index.built) return HESAFF_ERR_ARG;
   if (n_images) *n_images = c->index.n_images;
   if (vocabulary_size) *vocabulary_size = c->index.k;
   if (n_keys) *n_keys = c->index.n_keys;
   if (n_postings) *n_postings = c->index.n_postings;
   return HESAFF_OK;
}

int hesaff_index_clear(hesaff_ctx *c)
{
   if (!c) return HESAFF_ERR_ARG;
   if (!c->index.built) return HESAFF_OK;
   HS_API_BEGIN
   bind_device(c);
   HIP_TRY(hipStreamSynchronize(c->stream()));
   c->index = hesaff_ctx::Index();
   HS_API_END(c)
}

int hesaff_get_index_ms(const hesaff_ctx *c, float *build_ms, float *query_ms)
{
   if (!c || !build_ms || !query_ms) return HESAFF_ERR_ARG;
   *build_ms = c->index_ms[0] + c->index_ms[1];
   *query_ms = c->index_ms[2];
   return HESAFF_OK;
}

} // extern "C"
