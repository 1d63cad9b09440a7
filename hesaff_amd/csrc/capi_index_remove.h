// capi_index_remove.h -- removing images from the image index (hesaff_index_remove and hesaff_get_index_remove_ms of
// include/hesaff_amd.h) over the kernels of kernels_index_remove.h, with every number from index_remove_plan.h.  Included at the end
// of pipeline.hip, behind capi_index_grow.h (same translation unit).  The add's rule holds: a removal works on a new index and
// installs it when it is whole, so a refused or failed call leaves the context's index byte for byte as it was; a context that never
// calls it allocates, launches and copies nothing here.
#pragma once

namespace {

// the images flagged in gone[N] (m of them, checked) out of the context's index
void remove_from_index_on_device(hesaff_ctx *c, int m, const std::vector<uint32_t> &gone)
{
   const hesaff_ctx::Index &ox = c->index;
   const int k = ox.k, n_old = ox.n_images;
   hesaff_ctx::Index nx;
   nx.n_images = n_old - m; nx.k = k;
   StagePlan persistent;
   nx.a = index_arrays(persistent, nx.n_images, k);
   nx.tables.ensure(std::max<size_t>(persistent.bytes(), 256));   // (HESAFF_ERR_NOMEM: the context's index is untouched)
   TrainArena s;   // the scratch of the call: O(N + K) words
   const IndexRemoveArrays r = index_remove_arrays(s, n_old, k, ox.embedded);
   s.ensure();
   hipStream_t st = c->stream();
   const bool timed = c->profiling >= 1;
   // remap: 0 .. 1, count: 1 .. 2, tables: 2 .. 3 (with the remap's scan), (the host reads the sums and allocates the lists)
   // compact: 4 .. 5, key lists: 5 .. 6
   DevEvent ev[7];
   if (timed) for (DevEvent &e : ev) e = DevEvent(hipEventDefault);
   HIP_TRY(hipMemsetAsync(nx.tables.p, 0, persistent.bytes(), st));   // df, norm2, tfq, dot, score and the head start at zero
   HIP_TRY(hipMemsetAsync(s.buf.p, 0, std::max<size_t>(s.bytes(), 256), st));   // the cursors, the counts and the removed keys
   HIP_TRY(hipMemcpyAsync(s.ptr(r.gone), gone.data(), (size_t)n_old * 4, hipMemcpyHostToDevice, st));
   // step 1: the new number of every image that stays (block sums sized for N)
   if (timed) HIP_TRY(hipEventRecord(ev[0], st));
   LoadKeepU32 keep;
   keep.p = s.ptr(r.gone);
   exclusive_scan(c, keep, (long long)n_old, s.ptr(r.remap), s.ptr(r.kept), s.ptr(r.block_sums));
   hipLaunchKernelGGL(k_remove_mark, dim3((uint32_t)((n_old + 255) / 256)), dim3(256), 0, st, (const uint32_t *)s.ptr(r.gone), n_old, s.ptr(r.remap));
   // step 2: the postings and the keys every word keeps, the keys that go
   if (timed) HIP_TRY(hipEventRecord(ev[1], st));
   const uint32_t *remap = s.ptr(r.remap);
   if (ox.n_postings > 0)
      hipLaunchKernelGGL(k_remove_count, dim3(tile_grid((unsigned long long)ox.n_postings)), dim3(256), 0, st, (const uint32_t *)ox.ptr(ox.a.offsets), k,
                         (uint32_t)ox.n_postings, (const IndexPosting *)ox.lists.as<IndexPosting>(), remap, nx.ptr(nx.a.df), s.ptr(r.removed));
   if (ox.embedded && ox.n_keys > 0)
      hipLaunchKernelGGL(k_remove_count_keys, dim3(tile_grid((unsigned long long)ox.n_keys)), dim3(256), 0, st, (const uint32_t *)ox.kptr(ox.ka.offsets), k,
                         (uint32_t)ox.n_keys, (const uint32_t *)ox.kptr(ox.ka.image), remap, s.ptr(r.key_count));
   // step 3: idf over the images that stay, the new offsets
   if (timed) HIP_TRY(hipEventRecord(ev[2], st));
   hipLaunchKernelGGL(k_index_idf, dim3((uint32_t)((k + 255) / 256)), dim3(256), 0, st, (const uint32_t *)nx.ptr(nx.a.df), k, nx.n_images, nx.ptr(nx.a.idf));
   LoadU32 load;
   load.p = nx.ptr(nx.a.df);
   exclusive_scan(c, load, (long long)k, nx.ptr(nx.a.offsets), nx.ptr(nx.a.offsets) + k, s.ptr(r.block_sums));
   if (ox.embedded) {
      load.p = s.ptr(r.key_count);
      exclusive_scan(c, load, (long long)k, s.ptr(r.key_offsets), s.ptr(r.key_offsets) + k, s.ptr(r.block_sums));
   }
   if (timed) HIP_TRY(hipEventRecord(ev[3], st));
   // the sums in one round trip: the postings and keys that stay, the keys that go, the images that stay
   struct Sums { unsigned long long removed[HS_REMOVE_STRIPES * HS_REMOVE_STRIPE_WORDS]; uint32_t postings, keys, kept, pad; };
   Sums *h = (Sums *)c->h_small_end.ensure_small(sizeof(Sums));
   h->keys = 0u;
   HIP_TRY(hipMemcpyAsync(h->removed, s.ptr(r.removed), r.removed.bytes(), hipMemcpyDeviceToHost, st));
   HIP_TRY(hipMemcpyAsync(&h->postings, nx.ptr(nx.a.offsets) + k, 4, hipMemcpyDeviceToHost, st));
   HIP_TRY(hipMemcpyAsync(&h->kept, s.ptr(r.kept), 4, hipMemcpyDeviceToHost, st));
   if (ox.embedded) HIP_TRY(hipMemcpyAsync(&h->keys, s.ptr(r.key_offsets) + k, 4, hipMemcpyDeviceToHost, st));
   finish_stream(c);
   const int64_t n_postings = (int64_t)h->postings, n_keys = ox.n_keys - (int64_t)index_remove_sum(h->removed);
   if (h->kept != (uint32_t)nx.n_images || n_postings > ox.n_postings || n_keys < n_postings || (ox.embedded && (int64_t)h->keys != n_keys))
      throw HsError(HESAFF_ERR_DEVICE, "hesaff_index_remove: the postings do not add up");
   nx.n_keys = n_keys;
   nx.lists.ensure(index_lists_bytes(n_postings));
   // step 4: the postings that stay to their new lists under their new numbers, the norms under the new idf
   if (timed) HIP_TRY(hipEventRecord(ev[4], st));
   if (ox.n_postings > 0)
      hipLaunchKernelGGL(k_remove_compact, dim3(tile_grid((unsigned long long)ox.n_postings)), dim3(256), 0, st, (const uint32_t *)ox.ptr(ox.a.offsets),
                         (const uint32_t *)nx.ptr(nx.a.offsets), k, (uint32_t)ox.n_postings, (const IndexPosting *)ox.lists.as<IndexPosting>(),
                         nx.lists.as<IndexPosting>(), remap, (const uint32_t *)nx.ptr(nx.a.idf), nx.ptr(nx.a.norm2), s.ptr(r.cursor));
   if (timed) HIP_TRY(hipEventRecord(ev[5], st));
   nx.n_postings = n_postings; nx.built = true;
   // step 5: the key lists likewise
   if (ox.embedded) {
      StagePlan kp;
      nx.ka = key_list_arrays(kp, k, n_keys);
      nx.keys.ensure(std::max<size_t>(kp.bytes(), 256));
      HIP_TRY(hipMemcpyAsync(nx.kptr(nx.ka.offsets), s.ptr(r.key_offsets), ((size_t)k + 1) * 4, hipMemcpyDeviceToDevice, st));
      if (ox.n_keys > 0)
         hipLaunchKernelGGL(k_remove_compact_keys, dim3(tile_grid((unsigned long long)ox.n_keys)), dim3(256), 0, st, (const uint32_t *)ox.kptr(ox.ka.offsets),
                            (const uint32_t *)s.ptr(r.key_offsets), k, (uint32_t)ox.n_keys, (const unsigned long long *)ox.kptr(ox.ka.sig),
                            (const uint32_t *)ox.kptr(ox.ka.image), nx.kptr(nx.ka.sig), nx.kptr(nx.ka.image), remap, s.ptr(r.key_cursor));
      nx.embedded = true;
   }
   if (timed) HIP_TRY(hipEventRecord(ev[6], st));
   finish_stream(c);   // (the scratch goes with this frame)
   for (float &v : c->index_remove_ms) v = 0.0f;
   if (timed) {
      float scan_ms = 0.0f;
      HIP_TRY(hipEventElapsedTime(&scan_ms, ev[0], ev[1]));
      HIP_TRY(hipEventElapsedTime(&c->index_remove_ms[0], ev[1], ev[2]));
      HIP_TRY(hipEventElapsedTime(&c->index_remove_ms[1], ev[2], ev[3]));
      HIP_TRY(hipEventElapsedTime(&c->index_remove_ms[2], ev[4], ev[5]));
      if (ox.embedded) HIP_TRY(hipEventElapsedTime(&c->index_remove_ms[3], ev[5], ev[6]));
      c->index_remove_ms[1] += scan_ms;   // the tables: idf and every scan
   }
   c->index = std::move(nx);   // (the batch scratch goes with the old index, as in an add)
}

} // namespace

extern "C" {

int hesaff_index_remove(hesaff_ctx *c, int m_images, const int32_t *images, int32_t *remap_out)
{
   if (!c || !images || !c->index.built || !index_remove_ok(c->index.n_images, m_images)) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   const int n_old = c->index.n_images;
   std::vector<uint32_t> gone;
   int64_t offender = 0;
   const IndexRemoveFault fault = index_remove_flags(images, m_images, n_old, gone, &offender);
   if (fault == HS_REMOVE_OUTSIDE)
      throw HsError(HESAFF_ERR_ARG, "hesaff_index_remove: image " + std::to_string(offender) + " lies outside 0 .. " + std::to_string(n_old - 1));
   if (fault == HS_REMOVE_TWICE) throw HsError(HESAFF_ERR_ARG, "hesaff_index_remove: image " + std::to_string(offender) + " is given twice");
   bind_device(c);
   remove_from_index_on_device(c, m_images, gone);
   if (remap_out) index_remove_remap(gone.data(), n_old, remap_out);
   HS_API_END(c)
}

// of the last removal at profiling level >= 1: the counting pass, the tables (idf and the scans), the compaction, the key lists
int hesaff_get_index_remove_ms(const hesaff_ctx *c, float *count_ms, float *tables_ms, float *compact_ms, float *keys_ms)
{
   if (!c || !count_ms || !tables_ms || !compact_ms || !keys_ms) return HESAFF_ERR_ARG;
   *count_ms = c->index_remove_ms[0]; *tables_ms = c->index_remove_ms[1]; *compact_ms = c->index_remove_ms[2]; *keys_ms = c->index_remove_ms[3];
   return HESAFF_OK;
}

} // extern "C"
