// capi_cells.h -- vocabulary cells and probes (hesaff_set_vocabulary_cells, hesaff_set_vocabulary_probes, hesaff_stage_probe_cells,
// hesaff_build_vocabulary_cells, hesaff_train_vocabulary_cells* of include/hesaff_amd.h): the entry points over the launchers beside launch_assign_words (pipeline.hip) and the training loop
// (capi_train.h).  Included at the end of pipeline.hip, behind capi_train.h (same translation unit).  A context without a layer
// allocates, launches and copies nothing here.
#pragma once

extern "C" {

int hesaff_set_vocabulary_cells(hesaff_ctx *c, int cells, const uint8_t *coarse, const uint32_t *first)
{
   if (!c || cells < 0 || c->vocab.k == 0 || cells > c->vocab.k) return HESAFF_ERR_ARG;
   if (cells > 0 && (!coarse || !cells_first_ok(first, cells, c->vocab.k))) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   if (cells > 0 && c->neighbours > 1)
      throw HsError(HESAFF_ERR_ARG, "a cell layer and vocabulary neighbours (R > 1) do not combine: set hesaff_set_vocabulary_neighbours to 1 first; no layer is set");
   bind_device(c);
   hesaff_ctx::Cells &cl = c->cells;
   if (cells == 0) {
      HIP_TRY(hipStreamSynchronize(c->stream()));   // nothing still reads the layer that goes
      cl.clear();
      return HESAFF_OK;
   }
   std::vector<uint8_t> tiles;
   std::vector<int32_t> norms;
   pack_vocabulary(coarse, cells, tiles, norms);
   StagePlan p;
   const CellLayerArrays a = cell_layer_arrays(p, cells);
   DevBuf layer;
   layer.ensure(p.bytes());   // (throws HESAFF_ERR_NOMEM with the context's layer untouched)
   HIP_TRY(hipMemcpy(layer.at<uint8_t>(a.tiles.off), tiles.data(), tiles.size(), hipMemcpyHostToDevice));
   HIP_TRY(hipMemcpy(layer.at<int32_t>(a.norms.off), norms.data(), norms.size() * 4, hipMemcpyHostToDevice));
   HIP_TRY(hipMemcpy(layer.at<uint32_t>(a.first.off), first, a.first.bytes(), hipMemcpyHostToDevice));
   HIP_TRY(hipStreamSynchronize(c->stream()));
   cl.layer = std::move(layer);
   cl.a = a;
   cl.c = cells;
   cl.timed_slices = 0;
   c->assign_timed = false;
   HS_API_END(c)
}

int hesaff_get_vocabulary_cells(const hesaff_ctx *c, int *cells)
{
   if (!c || !cells) return HESAFF_ERR_ARG;
   *cells = c->cells.c;
   return HESAFF_OK;
}

int hesaff_set_vocabulary_probes(hesaff_ctx *c, int probes)
{
   if (!c || !cells_probes_ok(probes)) return HESAFF_ERR_ARG;
   c->cells.probes = probes;   // (read by the next assignment through a layer; nothing on the device depends on it until then)
   return HESAFF_OK;
}

int hesaff_get_vocabulary_probes(const hesaff_ctx *c, int *probes)
{
   if (!c || !probes) return HESAFF_ERR_ARG;
   *probes = c->cells.probes;
   return HESAFF_OK;
}

// k_probe_cells alone on caller-supplied descriptors: the context's layer and probe count, P' = min(P, C) cells per key in probe order
int hesaff_stage_probe_cells(hesaff_ctx *c, int n, const uint8_t *desc, int32_t *cells_out, int32_t *dist2_out)
{
   if (!c || n < 0 || (n > 0 && (!desc || !cells_out || !dist2_out)) || c->cells.c == 0) return HESAFF_ERR_ARG;
   const int used = cells_probes_used(c->cells.probes, c->cells.c);
   if (cells_probe_entries(n, used) > HS_CELLS_SLICE_KEYS) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   if (n == 0) return HESAFF_OK;
   const size_t entries = (size_t)cells_probe_entries(n, used);
   StageArena a(c);
   const Span<uint8_t> a_desc = a.add<uint8_t>((size_t)n * 128);
   const Span<int32_t> a_out = a.add<int32_t>(entries * 2);   // (cell, dist2) per entry
   a.ensure();
   a.upload(a_desc, desc);
   CellsDevice d{};
   d.tiles = c->cells.layer.at<uint8_t>(c->cells.a.tiles.off); d.norms = c->cells.layer.at<int32_t>(c->cells.a.norms.off);
   d.n_tiles = c->cells.a.n_tiles; d.c = c->cells.c;
   launch_probe_kernel(c->stream(), d, a.ptr(a_desc), n, 128, 0, used, a.ptr(a_out));
   std::vector<int32_t> rows(entries * 2);
   a.download(rows.data(), a_out);
   finish_stream(c);
   for (size_t e = 0; e < entries; e++) { cells_out[e] = rows[2 * e]; dist2_out[e] = rows[2 * e + 1]; }
   HS_API_END(c)
}

int hesaff_get_assign_cells_ms(const hesaff_ctx *c, float *coarse_ms, float *group_ms, float *fine_ms)
{
   if (!c || !coarse_ms || !group_ms || !fine_ms) return HESAFF_ERR_ARG;
   float sum[3] = {0.0f, 0.0f, 0.0f};
   for (int i = 0; i < c->cells.timed_slices; i++) {
      const DevEvent *ev = &c->cells.ev[(size_t)(4 * i)];
      bool ok = hipEventSynchronize(ev[3]) == hipSuccess;
      for (int q = 0; q < 3 && ok; q++) {
         float ms = 0.0f;
         ok = hipEventElapsedTime(&ms, ev[q], ev[q + 1]) == hipSuccess;
         sum[q] += ms;
      }
      if (!ok) {
         (void)hipGetLastError();
         sum[0] = sum[1] = sum[2] = 0.0f;
         break;
      }
   }
   *coarse_ms = sum[0]; *group_ms = sum[1]; *fine_ms = sum[2];
   return HESAFF_OK;
}

// A layer for any k rows given c coarse rows: every row's nearest coarse row on the device (k_assign_words against a private packed
// copy of the coarse rows), the stable sort by cell on the host (cells_group_rows, cells_plan.h)
int hesaff_build_vocabulary_cells(hesaff_ctx *c, int k, const uint8_t *words, int cells, const uint8_t *coarse, uint8_t *words_out, int32_t *order_out,
                                  uint8_t *coarse_out, uint32_t *first_out, int *cells_out)
{
   if (!c || !words || !coarse || !words_out || !order_out || !coarse_out || !first_out || !cells_out) return HESAFF_ERR_ARG;
   if (k < 1 || k > HS_VOCAB_MAX_ROWS || cells < 1 || cells > k) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   std::vector<uint8_t> tiles;
   std::vector<int32_t> norms;
   pack_vocabulary(coarse, cells, tiles, norms);
   TrainArena m;
   const CellLayerArrays a = cell_layer_arrays(m, cells);
   const Span<uint8_t> a_rows = m.add<uint8_t>((size_t)k * 128);
   const Span<int32_t> a_cell = m.add<int32_t>((size_t)k * 2);
   m.ensure();
   hipStream_t st = c->stream();
   HIP_TRY(hipMemcpyAsync(m.ptr(a.tiles), tiles.data(), tiles.size(), hipMemcpyHostToDevice, st));
   HIP_TRY(hipMemcpyAsync(m.ptr(a.norms), norms.data(), norms.size() * 4, hipMemcpyHostToDevice, st));
   HIP_TRY(hipMemcpyAsync(m.ptr(a_rows), words, a_rows.bytes(), hipMemcpyHostToDevice, st));
   launch_assign_kernel(st, m.ptr(a.tiles), m.ptr(a.norms), a.n_tiles, m.ptr(a_rows), k, 128, 0, m.ptr(a_cell));
   std::vector<int32_t> assigned((size_t)k * 2), cell((size_t)k), kept((size_t)cells);
   HIP_TRY(hipMemcpyAsync(assigned.data(), m.ptr(a_cell), a_cell.bytes(), hipMemcpyDeviceToHost, st));
   finish_stream(c);
   for (int r = 0; r < k; r++) cell[(size_t)r] = assigned[2 * (size_t)r];
   const int n = cells_group_rows(cell.data(), k, cells, order_out, kept.data(), first_out);
   for (int r = 0; r < k; r++) memcpy(words_out + (size_t)r * 128, words + (size_t)order_out[r] * 128, 128);
   for (int j = 0; j < n; j++) memcpy(coarse_out + (size_t)j * 128, coarse + (size_t)kept[(size_t)j] * 128, 128);
   *cells_out = n;
   HS_API_END(c)
}

int hesaff_train_vocabulary_cells_device(hesaff_ctx *c, int64_t n, const void *d_desc, int64_t stride, int64_t offset, int k, const uint8_t *init, int cells,
                                         const uint8_t *coarse, const uint32_t *first, int iterations, uint8_t *words_out, int64_t *distortion, int32_t *empty,
                                         int *iterations_done)
{
   if (!c || !d_desc || !words_out || !init || !coarse || !train_counts_ok(n, k, iterations, true)) return HESAFF_ERR_ARG;
   if (!word_source_ok(stride, offset) || (uintptr_t)d_desc % 4 != 0 || !cells_first_ok(first, cells, k)) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   const TrainCells layer = {cells, coarse, first};
   train_on_device(c, (int)n, (const uint8_t *)d_desc, (long long)stride, (long long)offset, k, init, iterations, words_out, distortion, empty, iterations_done,
                   &layer);
   HS_API_END(c)
}

int hesaff_train_vocabulary_cells(hesaff_ctx *c, int64_t n, const uint8_t *desc, int k, const uint8_t *init, int cells, const uint8_t *coarse,
                                  const uint32_t *first, int iterations, uint8_t *words_out, int64_t *distortion, int32_t *empty, int *iterations_done)
{
   if (!c || !desc || !words_out || !init || !coarse || !train_counts_ok(n, k, iterations, true) || !cells_first_ok(first, cells, k)) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   DevBuf d;
   d.ensure((size_t)n * 128);
   HIP_TRY(hipMemcpyAsync(d.p, desc, (size_t)n * 128, hipMemcpyHostToDevice, c->stream()));
   const TrainCells layer = {cells, coarse, first};
   train_on_device(c, (int)n, d.as<uint8_t>(), 128, 0, k, init, iterations, words_out, distortion, empty, iterations_done, &layer);
   HS_API_END(c)
}

} // extern "C"
