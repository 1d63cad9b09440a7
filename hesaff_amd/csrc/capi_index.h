// capi_index.h -- the image index (hesaff_index_* and hesaff_get_index_ms of include/hesaff_amd.h): the build and the query over the
// kernels of kernels_index.h, with every number from index_plan.h.  Included at the end of pipeline.hip, behind capi_train.h (same
// translation unit).  The index is context state (hesaff_ctx::index); a build works on a new one and installs it when it is whole, so
// a refused or failed call leaves the previous index as it was, and a context that never builds one allocates, launches and copies
// nothing here.  What the later index files share is here as well, once: the words of a call and their staging (WordSource,
// stage_source), the halves a build and an add (capi_index_grow.h) have in common, the key lists of an embedded index, and the one
// driver of a single query, plain or embedded (capi_embed.h holds the embedded entry points alone).
#pragma once

namespace {

uint32_t grid_for(unsigned long long items, uint32_t cap = 1u << 16) { return (uint32_t)std::max<unsigned long long>(1, std::min<unsigned long long>((items + 255) / 256, cap)); }
uint32_t tile_grid(unsigned long long items) { return (uint32_t)std::max<unsigned long long>(1, (items + HS_GROW_TILE - 1) / HS_GROW_TILE); }

std::string word_outside(const char *who, const char *bound) { return std::string(who) + ": a word lies outside 0 .. " + bound + " - 1"; }

// the read-only check of device words: one outside 0 .. k - 1 is HESAFF_ERR_ARG before anything is built or scored
void check_device_words(hesaff_ctx *c, const int32_t *d_words, int word_stride, long long n, int k, const char *who, const char *bound = "vocabulary_size")
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
   if (*h) throw HsError(HESAFF_ERR_ARG, word_outside(who, bound));
}

// The words of a call as its caller gave them: every entry point that takes words describes them so and has stage_source make
// checked device words of them.
struct WordSource {
   const char *who;        // the entry point's public name, for the error text
   bool device;            // words and sigs lie in device memory (else in host memory)
   const void *words;      // key j's word: the int32 at index j * word_stride
   int word_stride;
   int64_t n;              // keys
   const void *sigs;       // with_sigs: a uint64 per key, packed
   bool with_sigs;
   const char *bound = "vocabulary_size";   // what the error text calls k
};
// n keys in device memory, every word inside 0 .. k - 1
struct DeviceWords {
   const int32_t *d_words;
   int word_stride;
   const unsigned long long *d_sigs;   // NULL without signatures
};

// what every entry point refuses (HESAFF_ERR_ARG, nothing touched) of a source whose n and word_stride are in bounds
bool source_ok(const WordSource &s)
{
   if (s.n > 0 && (!s.words || (s.with_sigs && !s.sigs))) return false;
   return !s.device || ((uintptr_t)s.words % 4 == 0 && (uintptr_t)s.sigs % 8 == 0);
}

// host words -> packed; one outside 0 .. k - 1 is HESAFF_ERR_ARG before the device is touched
void pack_host_words(const WordSource &s, int k, std::vector<int32_t> &packed)
{
   if (!index_stage_words((const int32_t *)s.words, s.word_stride, s.n, k, packed)) throw HsError(HESAFF_ERR_ARG, word_outside(s.who, s.bound));
}

// A source -> checked device words, with the device bound on the way.  Host words are checked and packed on the CPU and uploaded
// into words_to (and the signatures into *sigs_to), which the caller names and owns - at least 256 bytes each, nothing copied where
// n is 0; device words are checked where they lie and the two buffers are not touched.
DeviceWords stage_source(hesaff_ctx *c, const WordSource &s, int k, DevBuf &words_to, DevBuf *sigs_to = nullptr)
{
   if (s.device) {
      bind_device(c);
      check_device_words(c, (const int32_t *)s.words, s.word_stride, (long long)s.n, k, s.who, s.bound);
      return {(const int32_t *)s.words, s.word_stride, (const unsigned long long *)s.sigs};
   }
   std::vector<int32_t> packed;
   pack_host_words(s, k, packed);
   bind_device(c);
   const size_t n = (size_t)s.n;
   words_to.ensure(std::max<size_t>(n * 4, 256));
   if (s.with_sigs) sigs_to->ensure(std::max<size_t>(n * 8, 256));
   if (n > 0) {
      HIP_TRY(hipMemcpyAsync(words_to.p, packed.data(), n * 4, hipMemcpyHostToDevice, c->stream()));
      if (s.with_sigs) HIP_TRY(hipMemcpyAsync(sigs_to->p, s.sigs, n * 8, hipMemcpyHostToDevice, c->stream()));
   }
   return {words_to.as<int32_t>(), 1, s.with_sigs ? sigs_to->as<unsigned long long>() : nullptr};
}

// The front half of a build and of an add (ox: the index that grows, NULL for a build): the tables of nx (n_images and k set by
// the caller) and the scratch of the call are allocated, the `total` new words - of the images behind ox's - go into the hash
// table, and df (on top of ox's), idf and the posting offsets follow.  -> the postings of nx, read back on the host.  ev (profiling,
// else NULL): [0] before the hash step, [1] behind it, [2] behind the tables.  A build's cursor starts at the offsets; an add's is
// left to its merge.
int64_t index_tables_on_device(hesaff_ctx *c, hesaff_ctx::Index &nx, const hesaff_ctx::Index *ox, TrainArena &m, IndexBuildArrays &b, const int32_t *counts,
                               const DeviceWords &w, int64_t total, const DevEvent *ev)
{
   const int k = nx.k, n_new = nx.n_images - (ox ? ox->n_images : 0);
   StagePlan persistent;
   nx.a = index_arrays(persistent, nx.n_images, k);
   nx.tables.ensure(std::max<size_t>(persistent.bytes(), 256));   // (HESAFF_ERR_NOMEM: the context's index is untouched)
   b = index_build_arrays(m, n_new, k, total);   // (the hash table is sized for the new keys alone)
   m.ensure();
   hipStream_t st = c->stream();
   std::vector<uint32_t> starts((size_t)n_new + 1);
   index_starts(counts, n_new, starts.data());
   HIP_TRY(hipMemcpyAsync(m.ptr(b.starts), starts.data(), starts.size() * 4, hipMemcpyHostToDevice, st));
   HIP_TRY(hipMemsetAsync(nx.tables.p, 0, persistent.bytes(), st));   // df, norm2, tfq, dot, score and the head start at zero
   HIP_TRY(hipMemsetAsync(m.ptr(b.hash_keys), 0xFF, b.hash_keys.bytes(), st));
   HIP_TRY(hipMemsetAsync(m.ptr(b.hash_tf), 0, b.hash_tf.bytes(), st));
   // the distinct (image, word) pairs of the new images, numbered from 0 inside the table, and their tf
   if (ev) HIP_TRY(hipEventRecord(ev[0], st));
   if (total > 0)
      hipLaunchKernelGGL(k_index_insert, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, st, w.d_words, w.word_stride, (const uint32_t *)m.ptr(b.starts), n_new,
                         (uint32_t)total, b.bits, m.ptr(b.hash_keys), m.ptr(b.hash_tf));
   if (ev) HIP_TRY(hipEventRecord(ev[1], st));
   // df (= old + new), idf over all the images, the list offsets
   if (ox) HIP_TRY(hipMemcpyAsync(nx.ptr(nx.a.df), ox->ptr(ox->a.df), (size_t)k * 4, hipMemcpyDeviceToDevice, st));
   hipLaunchKernelGGL(k_index_df, dim3(grid_for(b.slots)), dim3(256), 0, st, (const unsigned long long *)m.ptr(b.hash_keys), (unsigned long long)b.slots, nx.ptr(nx.a.df));
   hipLaunchKernelGGL(k_index_idf, dim3((uint32_t)((k + 255) / 256)), dim3(256), 0, st, (const uint32_t *)nx.ptr(nx.a.df), k, nx.n_images, nx.ptr(nx.a.idf));
   LoadU32 load;
   load.p = nx.ptr(nx.a.df);
   exclusive_scan(c, load, (long long)k, nx.ptr(nx.a.offsets), nx.ptr(nx.a.offsets) + k, m.ptr(b.block_sums));
   if (!ox) HIP_TRY(hipMemcpyAsync(m.ptr(b.cursor), nx.ptr(nx.a.offsets), (size_t)k * 4, hipMemcpyDeviceToDevice, st));
   uint32_t *h_postings = (uint32_t *)c->h_small_end.ensure_small(4);
   HIP_TRY(hipMemcpyAsync(h_postings, nx.ptr(nx.a.offsets) + k, 4, hipMemcpyDeviceToHost, st));
   if (ev) HIP_TRY(hipEventRecord(ev[2], st));
   finish_stream(c);   // (`starts` has been read)
   return (int64_t)*h_postings;
}

// The second half, behind the merge of an add: the table's slots to their lists, the new images numbered behind ox's
void scatter_postings(hesaff_ctx *c, hesaff_ctx::Index &nx, const hesaff_ctx::Index *ox, const TrainArena &m, const IndexBuildArrays &b)
{
   hipLaunchKernelGGL(k_index_postings, dim3(grid_for(b.slots)), dim3(256), 0, c->stream(), (const unsigned long long *)m.ptr(b.hash_keys),
                      (const uint32_t *)m.ptr(b.hash_tf), (unsigned long long)b.slots, (uint32_t)(ox ? ox->n_images : 0), (const uint32_t *)nx.ptr(nx.a.idf), m.ptr(b.cursor),
                      nx.lists.as<IndexPosting>(), nx.ptr(nx.a.norm2));
}

// The key lists of an embedded nx (n_images, k and n_keys set) in the scratch of its build or add, behind the posting scatter, which
// is done with the cursor: per-word key counts (ox's lengths + the new words'), a scan, ox's keys to their new places (a build has
// none: the cursor starts at the offsets), and the scatter of the new keys behind them.  Enqueued only: the caller waits.
void build_key_lists(hesaff_ctx *c, hesaff_ctx::Index &nx, const hesaff_ctx::Index *ox, const TrainArena &m, const IndexBuildArrays &b, const DeviceWords &w,
                     int64_t total)
{
   const int k = nx.k, n_old = ox ? ox->n_images : 0;
   StagePlan persistent;
   nx.ka = key_list_arrays(persistent, k, nx.n_keys);
   nx.keys.ensure(std::max<size_t>(persistent.bytes(), 256));   // (HESAFF_ERR_NOMEM: the context's index is untouched)
   hipStream_t st = c->stream();
   const uint32_t key_blocks = (uint32_t)((total + 255) / 256);
   uint32_t *cursor = m.ptr(b.cursor), *offsets = nx.kptr(nx.ka.offsets);
   if (ox) hipLaunchKernelGGL(k_list_lengths, dim3((uint32_t)((k + 255) / 256)), dim3(256), 0, st, (const uint32_t *)ox->kptr(ox->ka.offsets), k, cursor);
   else HIP_TRY(hipMemsetAsync(cursor, 0, (size_t)k * 4, st));
   if (total > 0)
      hipLaunchKernelGGL(k_word_histogram, dim3(key_blocks), dim3(256), 0, st, w.d_words, w.word_stride, (int)total, cursor, 1, (unsigned long long *)nullptr);
   LoadU32 load;
   load.p = cursor;
   exclusive_scan(c, load, (long long)k, offsets, offsets + k, m.ptr(b.block_sums));
   if (ox)
      hipLaunchKernelGGL(k_keylist_merge, dim3(tile_grid(std::max<unsigned long long>((unsigned long long)ox->n_keys, (unsigned long long)k))), dim3(256), 0, st,
                         (const uint32_t *)ox->kptr(ox->ka.offsets), (const uint32_t *)offsets, k, (uint32_t)ox->n_keys, (const unsigned long long *)ox->kptr(ox->ka.sig),
                         (const uint32_t *)ox->kptr(ox->ka.image), nx.kptr(nx.ka.sig), nx.kptr(nx.ka.image), cursor);
   else HIP_TRY(hipMemcpyAsync(cursor, offsets, (size_t)k * 4, hipMemcpyDeviceToDevice, st));   // (the scan has read the counts)
   if (total > 0)
      hipLaunchKernelGGL(k_keylist_scatter, dim3(key_blocks), dim3(256), 0, st, w.d_words, w.word_stride, w.d_sigs, (const uint32_t *)m.ptr(b.starts), nx.n_images - n_old,
                         (uint32_t)total, (uint32_t)n_old, cursor, nx.kptr(nx.ka.sig), nx.kptr(nx.ka.image));
   nx.embedded = true;
}

// the build over `total` checked words in device memory (arguments checked by the caller); embedded: with the key lists of
// hesaff_index_build_embedded over the words' signatures, behind the plain build's steps, which are the same either way
void build_index_on_device(hesaff_ctx *c, int n_images, const int32_t *counts, const DeviceWords &w, int k, int64_t total, bool embedded)
{
   hesaff_ctx::Index nx;
   nx.n_images = n_images; nx.k = k; nx.n_keys = total;
   TrainArena m;   // the scratch of the call, released when it returns
   IndexBuildArrays b;
   const bool timed = c->profiling >= 1;
   DevEvent ev[4];   // the hash step: 0 .. 1, the list steps: 1 .. 3 (2: behind the tables, where the host reads the number of postings)
   if (timed) for (DevEvent &e : ev) e = DevEvent(hipEventDefault);
   // steps 1 and 2: the distinct (image, word) pairs and their tf; df, idf, the list offsets
   const int64_t n_postings = index_tables_on_device(c, nx, nullptr, m, b, counts, w, total, timed ? ev : nullptr);
   if (n_postings > total) throw HsError(HESAFF_ERR_DEVICE, "hesaff_index_build: more postings than keys");
   nx.lists.ensure(index_lists_bytes(n_postings));
   // then the lists and the norms in a second pass over the table
   scatter_postings(c, nx, nullptr, m, b);
   if (timed) HIP_TRY(hipEventRecord(ev[3], c->stream()));
   nx.n_postings = n_postings; nx.built = true;
   if (embedded) build_key_lists(c, nx, nullptr, m, b, w, total);
   finish_stream(c);   // (the scratch goes with this frame)
   c->index_ms[0] = c->index_ms[1] = c->index_ms[2] = 0.0f;
   if (timed) {
      HIP_TRY(hipEventElapsedTime(&c->index_ms[0], ev[0], ev[1]));
      HIP_TRY(hipEventElapsedTime(&c->index_ms[1], ev[1], ev[3]));
   }
   c->index = std::move(nx);
}

// the words of a query, or of a batch of them (capi_index_batch.h), and how they are scored
struct QuerySource {
   DeviceWords w;    // checked
   int threshold;    // embedded: the largest Hamming distance that still counts
   bool embedded;    // over the key lists, with a signature per word
};

// the query over n words; the ranked result goes to the caller's arrays
void query_index_on_device(hesaff_ctx *c, int n, const QuerySource &src, int top, int32_t *images_out, double *scores_out, int *count_out)
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
      hipLaunchKernelGGL(k_query_count, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, src.w.d_words, src.w.word_stride, n, ix.ptr(ix.a.tfq));
      if (src.embedded)
         hipLaunchKernelGGL(k_query_score_embedded, dim3((uint32_t)((n + 3) / 4)), dim3(256), 0, st, src.w.d_words, src.w.word_stride, src.w.d_sigs, n, src.threshold,
                            ix.ptr(ix.a.tfq), (const uint32_t *)ix.ptr(ix.a.idf), (const uint32_t *)ix.kptr(ix.ka.offsets), (const unsigned long long *)ix.kptr(ix.ka.sig),
                            (const uint32_t *)ix.kptr(ix.ka.image), ix.ptr(ix.a.dot), head);
      else
         hipLaunchKernelGGL(k_query_score, dim3((uint32_t)((n + 3) / 4)), dim3(256), 0, st, src.w.d_words, src.w.word_stride, n, ix.ptr(ix.a.tfq),
                            (const uint32_t *)ix.ptr(ix.a.idf), (const uint32_t *)ix.ptr(ix.a.offsets), (const IndexPosting *)ix.lists.as<IndexPosting>(), ix.ptr(ix.a.dot), head);
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

// the four build forms: what they refuse, the staging, the build (src.n: set here)
int build_from(hesaff_ctx *c, int n_images, const int32_t *counts, WordSource src, int vocabulary_size)
{
   if (!c || !counts || !index_counts_ok(n_images, vocabulary_size) || !index_word_stride_ok(src.word_stride)) return HESAFF_ERR_ARG;
   src.n = index_total_keys(counts, n_images);
   if (src.n < 0 || !source_ok(src)) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   DevBuf d, g;   // the staged words and signatures of a host form go with the call
   const DeviceWords w = stage_source(c, src, vocabulary_size, d, &g);
   build_index_on_device(c, n_images, counts, w, vocabulary_size, src.n, src.with_sigs);
   HS_API_END(c)
}

// the four single-query forms: a host form's words and signatures are staged in the index's own buffers
int query_from(hesaff_ctx *c, const WordSource &src, int hamming, int top, int32_t *images_out, double *scores_out, int *count_out)
{
   if (!c || !images_out || !scores_out || !count_out || !index_query_ok(src.n, top) || !index_word_stride_ok(src.word_stride)) return HESAFF_ERR_ARG;
   if ((src.with_sigs && (!embed_threshold_ok(hamming) || !c->index.embedded)) || !source_ok(src) || !c->index.built) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   const QuerySource q = {stage_source(c, src, c->index.k, c->index.qwords, &c->index.qsigs), hamming, src.with_sigs};
   query_index_on_device(c, (int)src.n, q, top, images_out, scores_out, count_out);
   HS_API_END(c)
}

} // namespace

extern "C" {

int hesaff_index_build_device(hesaff_ctx *c, int n_images, const int32_t *counts, const void *d_words, int word_stride, int vocabulary_size)
{
   return build_from(c, n_images, counts, {"hesaff_index_build_device", true, d_words, word_stride, 0, nullptr, false}, vocabulary_size);
}

int hesaff_index_build(hesaff_ctx *c, int n_images, const int32_t *counts, const int32_t *words, int word_stride, int vocabulary_size)
{
   return build_from(c, n_images, counts, {"hesaff_index_build", false, words, word_stride, 0, nullptr, false}, vocabulary_size);
}

int hesaff_index_query_device(hesaff_ctx *c, int n, const void *d_words, int word_stride, int top, int32_t *images_out, double *scores_out, int *count_out)
{
   return query_from(c, {"hesaff_index_query_device", true, d_words, word_stride, n, nullptr, false}, 0, top, images_out, scores_out, count_out);
}

int hesaff_index_query(hesaff_ctx *c, int n, const int32_t *words, int word_stride, int top, int32_t *images_out, double *scores_out, int *count_out)
{
   return query_from(c, {"hesaff_index_query", false, words, word_stride, n, nullptr, false}, 0, top, images_out, scores_out, count_out);
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
