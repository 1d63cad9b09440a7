// capi_index_grow.h -- the image index as a durable, growing object (hesaff_index_add*, hesaff_index_get_postings, hesaff_index_save,
// hesaff_index_load and hesaff_get_index_growth_ms of include/hesaff_amd.h) over the kernels of kernels_index_grow.h, with every
// number from index_plan.h.  Included at the end of pipeline.hip, behind capi_embed.h (same translation unit).  The build's rule
// holds: an add and a load work on a new index and install it when it is whole, so a refused or failed call leaves the context's
// index byte for byte as it was; a context that calls none of these allocates, launches and copies nothing here.
#pragma once

namespace {

// m images of `total` checked words (and, for an embedded index, their signatures) in device memory behind the context's index
void add_to_index_on_device(hesaff_ctx *c, int m, const int32_t *counts, const DeviceWords &w, int64_t total)
{
   const hesaff_ctx::Index &ox = c->index;
   const int k = ox.k;
   hesaff_ctx::Index nx;
   nx.n_images = ox.n_images + m; nx.k = k; nx.n_keys = ox.n_keys + total;
   TrainArena s;   // the scratch of the call: its hash table is sized for the new keys alone
   IndexBuildArrays b;
   hipStream_t st = c->stream();
   const bool timed = c->profiling >= 1;
   DevEvent ev[6];   // insert: 0 .. 1, tables: 1 .. 2, (the host reads the number of postings and allocates the lists) merge: 3 .. 4, scatter: 4 .. 5
   if (timed) for (DevEvent &e : ev) e = DevEvent(hipEventDefault);
   // steps 1 and 2: the distinct (image, word) pairs of the new images; df = old + new, idf over N + m, the new offsets
   const int64_t n_postings = index_tables_on_device(c, nx, &ox, s, b, counts, w, total, timed ? ev : nullptr);
   if (n_postings < ox.n_postings || n_postings > ox.n_postings + total) throw HsError(HESAFF_ERR_DEVICE, "hesaff_index_add: the postings do not add up");
   nx.lists.ensure(index_lists_bytes(n_postings));
   // step 3: the old postings to their new places, the old norms under the new idf, the cursors behind them
   if (timed) HIP_TRY(hipEventRecord(ev[3], st));
   hipLaunchKernelGGL(k_index_merge, dim3(tile_grid(std::max<unsigned long long>((unsigned long long)ox.n_postings, (unsigned long long)k))), dim3(256), 0, st,
                      (const uint32_t *)ox.ptr(ox.a.offsets), (const uint32_t *)nx.ptr(nx.a.offsets), k, (uint32_t)ox.n_postings,
                      (const IndexPosting *)ox.lists.as<IndexPosting>(), nx.lists.as<IndexPosting>(), (const uint32_t *)nx.ptr(nx.a.idf), nx.ptr(nx.a.norm2),
                      s.ptr(b.cursor));
   if (timed) HIP_TRY(hipEventRecord(ev[4], st));
   // step 4: the new postings behind them
   scatter_postings(c, nx, &ox, s, b);
   if (timed) HIP_TRY(hipEventRecord(ev[5], st));
   nx.n_postings = n_postings; nx.built = true;
   if (ox.embedded) build_key_lists(c, nx, &ox, s, b, w, total);   // the key lists likewise: lengths = old + new, a scan, the move, the scatter
   finish_stream(c);   // (the scratch goes with this frame)
   for (int q = 0; q < 4; q++) c->index_growth_ms[q] = 0.0f;
   if (timed) {
      const int from[4] = {0, 1, 3, 4};
      for (int q = 0; q < 4; q++) HIP_TRY(hipEventElapsedTime(&c->index_growth_ms[q], ev[from[q]], ev[from[q] + 1]));
   }
   c->index = std::move(nx);
}

// the four add forms: what they refuse before anything is staged (an embedded index takes embedded adds alone, a plain one plain
// adds), the staging, the add (src.n: set here)
int add_from(hesaff_ctx *c, int m, const int32_t *counts, WordSource src)
{
   if (!c || !counts || !c->index.built || c->index.embedded != src.with_sigs || !index_word_stride_ok(src.word_stride)) return HESAFF_ERR_ARG;
   if (m < 1 || m > HS_INDEX_MAX_IMAGES) return HESAFF_ERR_ARG;
   src.n = index_total_keys(counts, m);
   if (src.n < 0 || !index_add_ok(c->index.n_images, m, c->index.n_keys, src.n) || !source_ok(src)) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   DevBuf d, g;   // the staged words and signatures of a host form go with the call
   const DeviceWords w = stage_source(c, src, c->index.k, d, &g);
   add_to_index_on_device(c, m, counts, w, src.n);
   HS_API_END(c)
}

// a host array of the index file's into a new device block
void upload(hipStream_t st, void *dst, const void *src, size_t bytes)
{
   if (bytes) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
}

// the index of a file's arrays (checked by hesaff_read_index_file: the sums of df and of key_count, every df <= n_images)
void load_index_on_device(hesaff_ctx *c, int embedded, int k, int n_images, int64_t n_keys, int64_t n_postings, const uint32_t *df, const uint32_t *postings,
                          const uint32_t *key_count, const uint32_t *key_image, const uint64_t *key_sig)
{
   hesaff_ctx::Index nx;
   StagePlan persistent;
   nx.a = index_arrays(persistent, n_images, k);
   nx.tables.ensure(std::max<size_t>(persistent.bytes(), 256));
   nx.lists.ensure(index_lists_bytes(n_postings));
   TrainArena s;
   const Span<unsigned long long> a_image_tf = s.add<unsigned long long>((size_t)n_images);
   const Span<unsigned long long> a_word_tf = s.add<unsigned long long>(embedded ? (size_t)k : 1);
   const Span<uint32_t> a_key_count = s.add<uint32_t>(embedded ? (size_t)k : 1);
   const Span<unsigned long long> a_total = s.add<unsigned long long>(1);
   const Span<uint32_t> a_flags = s.add<uint32_t>(1);
   const Span<uint32_t> a_block_sums = s.add<uint32_t>(((size_t)k + 4095) / 4096 + 1);
   s.ensure();
   hipStream_t st = c->stream();
   const bool timed = c->profiling >= 1;
   DevEvent ev[2];
   if (timed) for (DevEvent &e : ev) e = DevEvent(hipEventDefault);
   HIP_TRY(hipMemsetAsync(nx.tables.p, 0, persistent.bytes(), st));
   HIP_TRY(hipMemsetAsync(s.buf.p, 0, std::max<size_t>(s.bytes(), 256), st));
   upload(st, nx.ptr(nx.a.df), df, (size_t)k * 4);
   upload(st, nx.lists.p, postings, (size_t)n_postings * 8);
   if (embedded) {
      StagePlan kp;
      nx.ka = key_list_arrays(kp, k, n_keys);
      nx.keys.ensure(std::max<size_t>(kp.bytes(), 256));
      upload(st, s.ptr(a_key_count), key_count, (size_t)k * 4);
      upload(st, nx.kptr(nx.ka.image), key_image, (size_t)n_keys * 4);
      upload(st, nx.kptr(nx.ka.sig), key_sig, (size_t)n_keys * 8);
   }
   HIP_TRY(hipStreamSynchronize(st));   // (the pageable sources have been read)
   if (timed) HIP_TRY(hipEventRecord(ev[0], st));
   hipLaunchKernelGGL(k_index_idf, dim3((uint32_t)((k + 255) / 256)), dim3(256), 0, st, (const uint32_t *)nx.ptr(nx.a.df), k, n_images, nx.ptr(nx.a.idf));
   LoadU32 load;
   load.p = nx.ptr(nx.a.df);
   exclusive_scan(c, load, (long long)k, nx.ptr(nx.a.offsets), nx.ptr(nx.a.offsets) + k, s.ptr(a_block_sums));
   unsigned long long *word_tf = embedded ? s.ptr(a_word_tf) : nullptr;
   if (n_postings > 0)
      hipLaunchKernelGGL(k_index_load_postings, dim3(tile_grid((unsigned long long)n_postings)), dim3(256), 0, st, (const uint32_t *)nx.ptr(nx.a.offsets), k,
                         (uint32_t)n_postings, (const IndexPosting *)nx.lists.as<IndexPosting>(), n_images, (const uint32_t *)nx.ptr(nx.a.idf), nx.ptr(nx.a.norm2),
                         s.ptr(a_image_tf), word_tf, s.ptr(a_flags));
   hipLaunchKernelGGL(k_index_load_sums, dim3((uint32_t)((std::max(n_images, k) + 255) / 256)), dim3(256), 0, st, (const unsigned long long *)s.ptr(a_image_tf), n_images,
                      (const unsigned long long *)word_tf, (const uint32_t *)s.ptr(a_key_count), k, s.ptr(a_total), s.ptr(a_flags));
   if (embedded) {
      if (n_keys > 0)
         hipLaunchKernelGGL(k_index_load_key_images, dim3(grid_for((unsigned long long)n_keys, 4096)), dim3(256), 0, st, (const uint32_t *)nx.kptr(nx.ka.image),
                            (unsigned long long)n_keys, n_images, s.ptr(a_flags));
      load.p = s.ptr(a_key_count);
      uint32_t *offsets = nx.kptr(nx.ka.offsets);
      exclusive_scan(c, load, (long long)k, offsets, offsets + k, s.ptr(a_block_sums));
   }
   if (timed) HIP_TRY(hipEventRecord(ev[1], st));
   struct Sums { unsigned long long total; uint32_t flags, pad; };
   Sums *h = (Sums *)c->h_small_end.ensure_small(sizeof(Sums));
   HIP_TRY(hipMemcpyAsync(&h->total, s.ptr(a_total), 8, hipMemcpyDeviceToHost, st));
   HIP_TRY(hipMemcpyAsync(&h->flags, s.ptr(a_flags), 4, hipMemcpyDeviceToHost, st));
   finish_stream(c);
   uint32_t flags = h->flags;
   if (h->total != (unsigned long long)n_keys) flags |= HS_LOAD_TOTAL;
   if (flags) throw HsError(HESAFF_ERR_ARG, std::string("hesaff_index_load: ") + index_load_rule(flags));
   c->index_growth_ms[4] = 0.0f;
   if (timed) HIP_TRY(hipEventElapsedTime(&c->index_growth_ms[4], ev[0], ev[1]));
   nx.n_images = n_images; nx.k = k; nx.n_keys = n_keys; nx.n_postings = n_postings; nx.built = true; nx.embedded = embedded != 0;
   c->index = std::move(nx);
}

} // namespace

extern "C" {

int hesaff_index_add_device(hesaff_ctx *c, int m_images, const int32_t *counts, const void *d_words, int word_stride)
{
   return add_from(c, m_images, counts, {"hesaff_index_add_device", true, d_words, word_stride, 0, nullptr, false});
}

int hesaff_index_add(hesaff_ctx *c, int m_images, const int32_t *counts, const int32_t *words, int word_stride)
{
   return add_from(c, m_images, counts, {"hesaff_index_add", false, words, word_stride, 0, nullptr, false});
}

int hesaff_index_add_embedded_device(hesaff_ctx *c, int m_images, const int32_t *counts, const void *d_words, int word_stride, const void *d_sigs)
{
   return add_from(c, m_images, counts, {"hesaff_index_add_embedded_device", true, d_words, word_stride, 0, d_sigs, true});
}

int hesaff_index_add_embedded(hesaff_ctx *c, int m_images, const int32_t *counts, const int32_t *words, int word_stride, const uint64_t *sigs)
{
   return add_from(c, m_images, counts, {"hesaff_index_add_embedded", false, words, word_stride, 0, sigs, true});
}

int hesaff_index_get_postings(const hesaff_ctx *c, uint32_t *offsets, uint32_t *images, uint32_t *tf)
{
   if (!c || !c->index.built) return HESAFF_ERR_ARG;
   hesaff_ctx *m = const_cast<hesaff_ctx *>(c);   // (the error string is the context's)
   HS_API_BEGIN
   bind_device(m);
   const hesaff_ctx::Index &ix = c->index;
   const size_t n = (size_t)ix.n_postings;
   if (offsets) HIP_TRY(hipMemcpy(offsets, ix.ptr(ix.a.offsets), ((size_t)ix.k + 1) * 4, hipMemcpyDeviceToHost));
   if ((images || tf) && n) {
      std::vector<IndexPosting> lists(n);
      HIP_TRY(hipMemcpy(lists.data(), ix.lists.p, n * sizeof(IndexPosting), hipMemcpyDeviceToHost));
      for (size_t p = 0; p < n; p++) {
         if (images) images[p] = lists[p].image;
         if (tf) tf[p] = lists[p].tf;
      }
   }
   HS_API_END(m)
}

int hesaff_index_save(hesaff_ctx *c, const char *path)
{
   if (!c || !path || !c->index.built) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   HIP_TRY(hipStreamSynchronize(c->stream()));
   const hesaff_ctx::Index &ix = c->index;
   const size_t k = (size_t)ix.k, n = (size_t)ix.n_postings, t = (size_t)ix.n_keys;
   std::vector<uint32_t> df(k), postings(std::max<size_t>(2 * n, 1)), key_count, key_image;
   std::vector<uint64_t> key_sig;
   HIP_TRY(hipMemcpy(df.data(), ix.ptr(ix.a.df), k * 4, hipMemcpyDeviceToHost));
   if (n) HIP_TRY(hipMemcpy(postings.data(), ix.lists.p, n * 8, hipMemcpyDeviceToHost));   // (image, tf), word-major: the file's layout
   if (ix.embedded) {
      std::vector<uint32_t> off(k + 1);
      key_count.resize(k); key_image.resize(std::max<size_t>(t, 1)); key_sig.resize(std::max<size_t>(t, 1));
      HIP_TRY(hipMemcpy(off.data(), ix.kptr(ix.ka.offsets), (k + 1) * 4, hipMemcpyDeviceToHost));
      for (size_t w = 0; w < k; w++) key_count[w] = off[w + 1] - off[w];
      if (t) {
         HIP_TRY(hipMemcpy(key_image.data(), ix.kptr(ix.ka.image), t * 4, hipMemcpyDeviceToHost));
         HIP_TRY(hipMemcpy(key_sig.data(), ix.kptr(ix.ka.sig), t * 8, hipMemcpyDeviceToHost));
      }
   }
   const int rc = hesaff_write_index_file(path, ix.embedded ? 1 : 0, ix.k, ix.n_images, ix.n_keys, ix.n_postings, df.data(), postings.data(),
                                          ix.embedded ? key_count.data() : nullptr, ix.embedded ? key_image.data() : nullptr, ix.embedded ? key_sig.data() : nullptr);
   if (rc != HESAFF_OK) throw HsError(rc, std::string("hesaff_index_save: cannot write ") + path);
   HS_API_END(c)
}

int hesaff_index_load(hesaff_ctx *c, const char *path)
{
   if (!c || !path) return HESAFF_ERR_ARG;
   int embedded = 0, k = 0, n_images = 0;
   int64_t n_keys = 0, n_postings = 0;
   uint32_t *df = nullptr, *postings = nullptr, *key_count = nullptr, *key_image = nullptr;
   uint64_t *key_sig = nullptr;
   const int rc = hesaff_read_index_file(path, &embedded, &k, &n_images, &n_keys, &n_postings, &df, &postings, &key_count, &key_image, &key_sig);
   struct Blocks { void *p[5]; ~Blocks() { for (void *q : p) hesaff_free(q); } } blocks = {{df, postings, key_count, key_image, key_sig}};
   HS_API_BEGIN
   if (rc != HESAFF_OK) throw HsError(rc, std::string("hesaff_index_load: ") + path + (rc == HESAFF_ERR_NOMEM ? ": out of memory" : " cannot be read or is not a whole index file"));
   bind_device(c);
   load_index_on_device(c, embedded, k, n_images, n_keys, n_postings, df, postings, key_count, key_image, key_sig);
   HS_API_END(c)
}

// of the last add at profiling level >= 1: the hash step, the tables, the merge, the scatter; of the last load: its device pass
int hesaff_get_index_growth_ms(const hesaff_ctx *c, float *insert_ms, float *tables_ms, float *merge_ms, float *scatter_ms, float *load_ms)
{
   if (!c || !insert_ms || !tables_ms || !merge_ms || !scatter_ms || !load_ms) return HESAFF_ERR_ARG;
   *insert_ms = c->index_growth_ms[0]; *tables_ms = c->index_growth_ms[1]; *merge_ms = c->index_growth_ms[2]; *scatter_ms = c->index_growth_ms[3];
   *load_ms = c->index_growth_ms[4];
   return HESAFF_OK;
}

} // extern "C"
