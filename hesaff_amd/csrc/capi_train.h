// capi_train.h -- vocabulary training (hesaff_train_vocabulary*, hesaff_stage_accumulate_words of include/hesaff_amd.h): the loop of
// exact integer Lloyd iterations over k_assign_words (kernels_words.h) and the kernels of kernels_train.h.  Included at the end of
// pipeline.hip, behind capi_stage.h (same translation unit).  A call works in a buffer of its own (TrainArrays, train_plan.h) that it
// releases before it returns: the context's vocabulary, its words and its buffers are neither read nor written, and a context that
// never trains allocates, launches and copies nothing here.  The same loop trains inside the fixed cells of a layer
// (hesaff_train_vocabulary_cells*: capi_cells.h), whose arrays lie in the call's buffer as well.
#pragma once

namespace {

// the arrays of a call in a buffer that lives as long as the call
struct TrainArena : StagePlan {
   DevBuf buf;
   void ensure() { buf.ensure(std::max<size_t>(bytes(), 256)); }   // (HESAFF_ERR_NOMEM: the device cannot hold the working arrays)
   template <class T> T *ptr(const Span<T> &a) const { return buf.at<T>(a.off); }
};

// count and byte sums per word over n keys in device memory: a.counts, a.sums (and stats->distortion from the dist2 of (word, dist2)
// rows, word_stride 2: the caller has zeroed stats).
void accumulate_words(hesaff_ctx *c, const TrainArena &m, const AccumulateArrays &a, const uint8_t *d_desc, long long stride, long long offset,
                      const int32_t *d_words, int word_stride, int n, int k)
{
   hipStream_t st = c->stream();
   HIP_TRY(hipMemsetAsync(m.ptr(a.sums), 0, a.sums.bytes(), st));
   HIP_TRY(hipMemsetAsync(m.ptr(a.sub), 0, a.sub.bytes(), st));
   // (k_word_histogram and k_word_scatter: the same grid, so that a key's wave, and with it its slot, is the same in both)
   const uint32_t key_blocks = (uint32_t)((n + 255) / 256);
   unsigned long long *distortion = word_stride == 2 ? (unsigned long long *)&m.ptr(a.stats)->distortion : nullptr;
   hipLaunchKernelGGL(k_word_histogram, dim3(key_blocks), dim3(256), 0, st, d_words, word_stride, n, m.ptr(a.sub), a.slots, distortion);
   LoadU32 load;
   load.p = m.ptr(a.sub);
   exclusive_scan(c, load, (long long)a.sub.count, m.ptr(a.cursor), m.ptr(a.total), m.ptr(a.block_sums));
   hipLaunchKernelGGL(k_word_scatter, dim3(key_blocks), dim3(256), 0, st, d_words, word_stride, n, m.ptr(a.cursor), a.slots, m.ptr(a.perm));
   hipLaunchKernelGGL(k_word_counts, dim3((uint32_t)((k + 255) / 256)), dim3(256), 0, st, (const uint32_t *)m.ptr(a.cursor), a.slots, k, m.ptr(a.counts));
   const int walk = 8 * HS_ACC_CHUNK * a.chunks;   // positions of a block: four waves, two half-waves each
   hipLaunchKernelGGL(k_accumulate_words, dim3((uint32_t)((n + walk - 1) / walk)), dim3(256), 0, st, d_desc, stride, offset, d_words, word_stride,
                      (const uint32_t *)m.ptr(a.perm), n, a.chunks, m.ptr(a.sums));
}

void update_words(hesaff_ctx *c, const TrainArena &m, const TrainArrays &t, int k)
{
   const int rows_padded = t.n_tiles * HS_WORD_TILE;
   hipLaunchKernelGGL(k_update_words, dim3((uint32_t)((rows_padded + 7) / 8)), dim3(256), 0, c->stream(), (const uint32_t *)m.ptr(t.acc.sums),
                      (const uint32_t *)m.ptr(t.acc.counts), k, rows_padded, m.ptr(t.rows), m.ptr(t.tiles), m.ptr(t.norms), m.ptr(t.acc.stats));
}

// a fixed cell layer for the iterations (hesaff_train_vocabulary_cells: capi_cells.h): cells coarse rows and first[cells + 1], host memory
struct TrainCells {
   int cells;
   const uint8_t *coarse;
   const uint32_t *first;
};

// the iterations of hesaff_train_vocabulary_device on n descriptors in device memory (arguments checked by the caller).  With a layer
// the assignment of every iteration is the cell-restricted one: the coarse step and the grouping once, before the first iteration (a
// key's cell does not change while the coarse rows are fixed), k_assign_words_cells once per iteration.
void train_on_device(hesaff_ctx *c, int n, const uint8_t *d_desc, long long stride, long long offset, int k, const uint8_t *init, int iterations,
                     uint8_t *words_out, int64_t *distortion, int32_t *empty, int *iterations_done, const TrainCells *layer = nullptr)
{
   static_assert(HS_TRAIN_TILE == HS_WORD_TILE, "train_plan.h sizes the tiles k_assign_words reads");
   TrainArena m;
   const TrainArrays t = train_arrays(m, n, k);
   CellLayerArrays la = {};
   CellScratch ls = {};
   if (layer) { la = cell_layer_arrays(m, layer->cells); ls = cell_scratch(m, n, layer->cells); }
   m.ensure();
   hipStream_t st = c->stream();
   const bool timed = c->profiling >= 1;
   DevEvent ev[4];
   if (timed) for (DevEvent &e : ev) e = DevEvent(hipEventDefault);
   c->train_ms[0] = c->train_ms[1] = c->train_ms[2] = 0.0f;
   // V_0: the caller's rows or the sampled keys, then laid out for k_assign_words by the update kernel with every count zero
   HIP_TRY(hipMemsetAsync(m.ptr(t.acc.counts), 0, t.acc.counts.bytes(), st));
   HIP_TRY(hipMemsetAsync(m.ptr(t.acc.stats), 0, sizeof(TrainStats), st));
   if (init) HIP_TRY(hipMemcpyAsync(m.ptr(t.rows), init, (size_t)k * 128, hipMemcpyHostToDevice, st));
   else hipLaunchKernelGGL(k_sample_words, dim3((uint32_t)(((long long)k * 32 + 255) / 256)), dim3(256), 0, st, d_desc, stride, offset, n, k, m.ptr(t.rows));
   update_words(c, m, t, k);
   CellsDevice cd = {};
   if (layer) {
      // the private packed copy of the coarse rows; the pageable copies return once the source has been read
      std::vector<uint8_t> tiles;
      std::vector<int32_t> norms;
      pack_vocabulary(layer->coarse, layer->cells, tiles, norms);
      HIP_TRY(hipMemcpyAsync(m.ptr(la.tiles), tiles.data(), tiles.size(), hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(m.ptr(la.norms), norms.data(), norms.size() * 4, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(m.ptr(la.first), layer->first, la.first.bytes(), hipMemcpyHostToDevice, st));
      HIP_TRY(hipStreamSynchronize(st));
      cd = cells_device(m.buf.p, la, layer->cells, m.buf.p, ls);
      launch_cells_group(c, cd, d_desc, n, stride, offset, nullptr);
   }
   TrainStats *h = (TrainStats *)c->h_small_end.ensure_small(sizeof(TrainStats));
   int done = iterations;
   for (int it = 1; it <= iterations; it++) {
      HIP_TRY(hipMemsetAsync(m.ptr(t.acc.stats), 0, sizeof(TrainStats), st));
      if (timed) HIP_TRY(hipEventRecord(ev[0], st));
      if (layer) launch_cells_fine(st, cd, m.ptr(t.tiles), m.ptr(t.norms), d_desc, n, stride, offset, m.ptr(t.assigned));
      else launch_assign_kernel(st, m.ptr(t.tiles), m.ptr(t.norms), t.n_tiles, d_desc, n, stride, offset, m.ptr(t.assigned));
      if (timed) HIP_TRY(hipEventRecord(ev[1], st));
      accumulate_words(c, m, t.acc, d_desc, stride, offset, m.ptr(t.assigned), 2, n, k);
      if (timed) HIP_TRY(hipEventRecord(ev[2], st));
      update_words(c, m, t, k);
      if (timed) HIP_TRY(hipEventRecord(ev[3], st));
      HIP_TRY(hipMemcpyAsync(h, m.ptr(t.acc.stats), sizeof(TrainStats), hipMemcpyDeviceToHost, st));
      finish_stream(c);
      if (timed)
         for (int q = 0; q < 3; q++) {
            float ms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&ms, ev[q], ev[q + 1]));
            c->train_ms[q] += ms;
         }
      if (distortion) distortion[it - 1] = (int64_t)h->distortion;
      if (empty) empty[it - 1] = (int32_t)h->empty;
      if (h->changed == 0) { done = it; break; }   // V_t == V_{t-1}: a fixed point
   }
   HIP_TRY(hipMemcpyAsync(words_out, m.ptr(t.rows), (size_t)k * 128, hipMemcpyDeviceToHost, st));
   finish_stream(c);
   if (iterations_done) *iterations_done = done;
}

} // namespace

extern "C" {

int hesaff_train_vocabulary_device(hesaff_ctx *c, int64_t n, const void *d_desc, int64_t stride, int64_t offset, int k, const uint8_t *init,
                                   int iterations, uint8_t *words_out, int64_t *distortion, int32_t *empty, int *iterations_done)
{
   if (!c || !d_desc || !words_out || !train_counts_ok(n, k, iterations, init != nullptr)) return HESAFF_ERR_ARG;
   if (!word_source_ok(stride, offset) || (uintptr_t)d_desc % 4 != 0) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   train_on_device(c, (int)n, (const uint8_t *)d_desc, (long long)stride, (long long)offset, k, init, iterations, words_out, distortion, empty, iterations_done);
   HS_API_END(c)
}

int hesaff_train_vocabulary(hesaff_ctx *c, int64_t n, const uint8_t *desc, int k, const uint8_t *init, int iterations, uint8_t *words_out,
                            int64_t *distortion, int32_t *empty, int *iterations_done)
{
   if (!c || !desc || !words_out || !train_counts_ok(n, k, iterations, init != nullptr)) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   DevBuf d;
   d.ensure((size_t)n * 128);
   HIP_TRY(hipMemcpyAsync(d.p, desc, (size_t)n * 128, hipMemcpyHostToDevice, c->stream()));
   train_on_device(c, (int)n, d.as<uint8_t>(), 128, 0, k, init, iterations, words_out, distortion, empty, iterations_done);
   HS_API_END(c)
}

int hesaff_get_training_ms(const hesaff_ctx *c, float *assign_ms, float *accumulate_ms, float *update_ms)
{
   if (!c || !assign_ms || !accumulate_ms || !update_ms) return HESAFF_ERR_ARG;
   *assign_ms = c->train_ms[0]; *accumulate_ms = c->train_ms[1]; *update_ms = c->train_ms[2];
   return HESAFF_OK;
}

// the accumulation of a training iteration alone, on the caller's keys and words
int hesaff_stage_accumulate_words(hesaff_ctx *c, int n, const uint8_t *desc, const int32_t *words, int k, uint32_t *sums_out, uint32_t *counts_out)
{
   if (!c || !desc || !words || !sums_out || !counts_out || !accumulate_counts_ok(n, k)) return HESAFF_ERR_ARG;
   for (int i = 0; i < n; i++)
      if (words[i] < 0 || words[i] >= k) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   TrainArena m;
   const AccumulateArrays a = accumulate_arrays(m, n, k);
   const Span<uint8_t> a_desc = m.add<uint8_t>((size_t)n * 128);
   const Span<int32_t> a_words = m.add<int32_t>((size_t)n);
   m.ensure();
   hipStream_t st = c->stream();
   HIP_TRY(hipMemcpyAsync(m.ptr(a_desc), desc, a_desc.bytes(), hipMemcpyHostToDevice, st));
   HIP_TRY(hipMemcpyAsync(m.ptr(a_words), words, a_words.bytes(), hipMemcpyHostToDevice, st));
   accumulate_words(c, m, a, m.ptr(a_desc), 128, 0, m.ptr(a_words), 1, n, k);
   HIP_TRY(hipMemcpyAsync(sums_out, m.ptr(a.sums), a.sums.bytes(), hipMemcpyDeviceToHost, st));
   HIP_TRY(hipMemcpyAsync(counts_out, m.ptr(a.counts), a.counts.bytes(), hipMemcpyDeviceToHost, st));
   finish_stream(c);
   HS_API_END(c)
}

} // extern "C"
