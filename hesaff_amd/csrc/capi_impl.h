// capi_impl.h -- the extern "C" entry points of include/hesaff_amd.h, the stage operators apart (hesaff_stage_*: capi_stage.h).
// Included at the end of pipeline.hip (same translation unit: needs hesaff_ctx and the
// batch runner).  No exception crosses the ABI: everything is caught and turned into a
// negative return code + hesaff_last_error().
#pragma once

namespace {

int fail(hesaff_ctx *c, const HsError &e)
{
   if (c) c->err = e.msg; else g_create_error = e.msg;
   return e.code;
}

#define HS_API_BEGIN try {
#define HS_API_END(ctx)                                              \
   }                                                                 \
   catch (const HsError &e) { return fail(ctx, e); }                 \
   catch (const std::exception &e) { return fail(ctx, HsError(HESAFF_ERR_NOMEM, e.what())); } \
   return HESAFF_OK;

void bind_device(hesaff_ctx *c) { HIP_TRY(hipSetDevice(c->device)); }

// the end of a stage entry point: everything it enqueued on the main stream has run, and without an error
void finish_stream(hesaff_ctx *c)
{
   HIP_TRY(hipStreamSynchronize(c->stream()));
   HIP_TRY(hipGetLastError());
}

bool finite_f(float v) { return v == v && v - v == 0.0f; }

void validate_params(const hesaff_params &p)
{
   if (!finite_f(p.threshold) || !finite_f(p.edgeEigenValueRatio) || !finite_f(p.initialSigma) || !finite_f(p.convergenceThreshold) ||
       !finite_f(p.mrSize) || !finite_f(p.maxBinValue))
      throw HsError(HESAFF_ERR_ARG, "non-finite parameter");
   if (!(p.initialSigma > 0.0f)) throw HsError(HESAFF_ERR_ARG, "initialSigma must be positive");
   if (!(p.mrSize > 0.0f)) throw HsError(HESAFF_ERR_ARG, "mrSize must be positive");
   if (!(p.edgeEigenValueRatio > 0.0f)) throw HsError(HESAFF_ERR_ARG, "edgeEigenValueRatio must be positive");
   if (p.maxIterations < 1 || p.maxIterations > 1000) throw HsError(HESAFF_ERR_ARG, "maxIterations out of range (1..1000)");
   if (p.fast == 1)
      throw HsError(HESAFF_ERR_ARG, "hesaff_params.fast = 1 was withdrawn in ABI version 4 (it bought 1.02x); use 0 (parity mode) or 2");
   if (p.fast != 0 && p.fast != 2) throw HsError(HESAFF_ERR_ARG, "fast must be 0 (parity mode) or 2");
}

// What the two device-resident entry points share: the device and the batch size first, then (detect_device) the plan for a full
// batch, the batch itself and the counts read back.  check_source runs between plan and batch: the float planes' value check fires
// after the plan's own refusals.
void begin_device_batch(hesaff_ctx *c, int n)
{
   bind_device(c);
   if (n > c->par.max_batch) throw HsError(HESAFF_ERR_ARG, "n exceeds hesaff_params.max_batch for the device-resident entry point");
}

// hesaff_set_next_masks*: what is armed leaves the context with the call that meets it, whatever that call then returns
ArmedMasks take_masks(hesaff_ctx *c)
{
   ArmedMasks am;
   if (c) std::swap(am, c->next_masks);
   return am;
}

// a call that takes no masks met armed ones
void refuse_masks(const ArmedMasks &am, const char *why)
{
   if (am.kind != ArmedMasks::NONE) throw HsError(HESAFF_ERR_ARG, std::string("detection masks are armed (hesaff_set_next_masks), but ") + why + "; the masks are cleared");
}

// the masks of a device-resident call: n planes of height x width bytes in device memory
SelMasks device_masks(const ArmedMasks &am, int n, int height, int width)
{
   SelMasks mk;
   if (am.kind == ArmedMasks::NONE) return mk;
   if (am.kind != ArmedMasks::DEVICE) throw HsError(HESAFF_ERR_ARG, "masks armed with hesaff_set_next_masks (host memory) met a device-resident call; the masks are cleared");
   char msg[160];
   if (am.n != n) {
      snprintf(msg, sizeof msg, "%d masks armed for a call with %d images; the masks are cleared", am.n, n);
      throw HsError(HESAFF_ERR_ARG, msg);
   }
   const long long rs = am.row_stride ? am.row_stride : width;
   const long long is = am.img_stride ? (long long)am.img_stride : rs * height;
   if (rs < width) throw HsError(HESAFF_ERR_ARG, "row stride of the device masks smaller than the width; the masks are cleared");
   if (n > 1 && is < rs * (height - 1) + width) throw HsError(HESAFF_ERR_ARG, "image stride of the device masks does not keep the planes apart; the masks are cleared");
   mk.base = (const uint8_t *)am.d_masks; mk.img_stride = is; mk.row_stride = (int)rs; mk.W = width; mk.H = height;
   return mk;
}

template <class CHECK>
void detect_device(hesaff_ctx *c, int n, const SrcImages &src, int height, int width, int32_t *count_hessian, int32_t *count_desc,
                   const void **d_keys_out, int64_t *total_out, CHECK check_source, const ArmedMasks &am)
{
   const SelMasks mk = device_masks(am, n, height, width);
   plan(c, c->par.max_batch, height, width);
   check_source();
   c->word_spans.clear();
   c->sig_spans.clear();
   c->words_device_total = -1;
   c->sigs_device_total = -1;
   c->neigh_spans.clear();
   c->neigh_device_total = -1;
   const BatchResult r = run_batch(c, src, n, height, width, mk);
   const int32_t *hs = r.hessian_starts, *ds = r.desc_starts;
   if (c->vocab.k) { finish_stream(c); c->words_device_total = ds[n]; }   // the words of the batch are in b_words when the call returns
   if (c->vocab.k && c->neighbours > 1) { c->neigh_device_total = ds[n]; c->neigh_device_r = c->neighbours; }   // ... the neighbours in b_neigh
   if (c->embed.set) c->sigs_device_total = ds[n];                        // ... and the signatures in b_sigs
   for (int b = 0; b < n; b++) {
      if (count_hessian) count_hessian[b] = hs[b + 1] - hs[b];
      if (count_desc) count_desc[b] = ds[b + 1] - ds[b];
   }
   if (d_keys_out) *d_keys_out = c->geo.b_out.p;
   if (total_out) *total_out = ds[n];
}

} // namespace

extern "C" {

const char *hesaff_version(void)
{
#ifdef HESAFF_TUNING
   return "hesaff_amd 0.3 (gfx950, tuning build)";
#else
   return "hesaff_amd 0.3 (gfx950)";
#endif
}

int hesaff_abi_version(void) { return HESAFF_ABI_VERSION; }
size_t hesaff_sizeof_params(void) { return sizeof(hesaff_params); }
size_t hesaff_sizeof_timings(void) { return sizeof(hesaff_timings); }
size_t hesaff_sizeof_region(void) { return sizeof(hesaff_region); }

int hesaff_device_count(void)
{
   int n = 0;
   if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
   return n;
}

int hesaff_shard_range(int n, int rank, int world, int *lo, int *hi)
{
   if (n < 0 || world < 1 || rank < 0 || rank >= world || !lo || !hi) return HESAFF_ERR_ARG;
   *lo = (int)(((long long)n * rank + world - 1) / world);
   *hi = (int)(((long long)n * (rank + 1) + world - 1) / world);
   return HESAFF_OK;
}

int hesaff_default_params(hesaff_params *p)
{
   if (!p) return HESAFF_ERR_ARG;
   p->threshold = 16.0f / 3.0f;
   p->edgeEigenValueRatio = 10.0f;
   p->initialSigma = 1.6f;
   p->maxIterations = 16;
   p->convergenceThreshold = 0.05f;
   p->mrSize = 3.0f * sqrtf(3.0f);
   p->maxBinValue = 0.2f;
   p->upscaleInputImage = 0;
   p->max_batch = 64;
   p->max_kpts_per_mpx = 40000;
   p->fast = 0;
   return HESAFF_OK;
}

int hesaff_create(hesaff_ctx **out, const hesaff_params *p, int device)
{
   if (!out) return HESAFF_ERR_ARG;
   *out = nullptr;
   hesaff_ctx *c = nullptr;
   try {
      int ndev = 0;
      if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
         throw HsError(HESAFF_ERR_DEVICE, "no HIP device visible: libhesaff_amd has no CPU fallback");
      if (device < 0 || device >= ndev) throw HsError(HESAFF_ERR_ARG, "device ordinal out of range");
      c = new hesaff_ctx();
      if (p) c->par = *p; else hesaff_default_params(&c->par);
      if (c->par.max_batch < 1) c->par.max_batch = 1;
      if (c->par.max_kpts_per_mpx < 1000) c->par.max_kpts_per_mpx = 1000;
      validate_params(c->par);
      c->device = device;
      c->fast_pyramid = c->par.fast == 2;
#ifdef HESAFF_TUNING
      if (const char *fm = getenv("HESAFF_FAST")) c->fast_pyramid = atoi(fm) == 2;   // profile the fast mode under bench.py
#endif
      bind_device(c);
      hipDeviceProp_t prop;
      HIP_TRY(hipGetDeviceProperties(&prop, device));
      if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
         std::string m = std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only";
         throw HsError(HESAFF_ERR_DEVICE, m);
      }
      // The HIP streams of a context outlive it: the next context on this device takes the same ones, whole (take_stream_set).  A stream
      // created later lands on whichever hardware queue has the fewest users at that moment, so the second and third context of
      // a process used to get another - often worse - sharing of queues than the first (the chunks of bench.py's file leg, third
      // context of its process: 110-135 ms each against 107-110 in a process of their own).  New streams are created in the order
      // of their groups (0, 1, 2, 3; StreamSet has the pairing).
      if (!take_stream_set(device, c->sset))
         for (hipStream_t &st : c->sset.comp) HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
      for (int i = 0; i < HS_NSIDE; i++) c->ev_join[i] = DevEvent(hipEventDisableTiming);
      c->ev_fork = DevEvent(hipEventDisableTiming);
      // (the four compute streams stay on the default priority: every other assignment measured 1.5-6 % slower, profiles/r04_notes.md)
      c->ev_detect_done = DevEvent(hipEventDisableTiming | hipEventBlockingSync);
      c->ev_batch_done = DevEvent(hipEventDisableTiming | hipEventBlockingSync);
      for (int i = 0; i < HS_NSLOT; i++) {
         c->ev_extract_done[i] = DevEvent(hipEventDisableTiming);
         c->ev_sift_done[i] = DevEvent(hipEventDisableTiming);
      }
      set_kernel_attrs(c);
      {
         const ContextTables t = build_context_tables(c->par);
         c->tables.upload(t);
         c->ct = t;   // (the scalars; the vectors end here)
      }
      memset(&c->tm, 0, sizeof c->tm);
#ifdef HESAFF_TUNING
      // what makes the schedule observable (libhesaff_amd_tuning.so only); neither changes a result
      if (const char *ov = getenv("HESAFF_OVERLAP")) c->no_overlap = atoi(ov) == 0;
      c->debug = getenv("HESAFF_DEBUG") != nullptr;
      if (const char *sf = getenv("HESAFF_SIFT_INSIDE")) c->sift_inside = atoi(sf) == 1;
#endif
   } catch (const HsError &e) {
      hesaff_destroy(c);
      return fail(nullptr, e);
   } catch (const std::exception &e) {
      hesaff_destroy(c);
      return fail(nullptr, HsError(HESAFF_ERR_NOMEM, e.what()));
   }
   *out = c;
   return HESAFF_OK;
}

void hesaff_destroy(hesaff_ctx *c)
{
   if (!c) return;
   const int device = c->device;
   (void)hipSetDevice(device);
   // Every HIP stream of the context is idle before anything goes back: no kernel still uses a buffer, no copy engine a page-locked
   // block.  The members then free themselves; the streams outlive the context and serve the next one on this device.
   const StreamSet set = c->sset;
   for (hipStream_t st : {set.comp[0], set.comp[1], set.comp[2], set.comp[3], set.h2d, set.d2h})
      if (st) (void)hipStreamSynchronize(st);
   delete c;
   if (set.comp[3]) give_stream_set(device, set);   // (a context whose creation failed before its streams were complete has no set)
}

const char *hesaff_last_error(const hesaff_ctx *c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int hesaff_set_profiling(hesaff_ctx *c, int level)
{
   if (!c) return HESAFF_ERR_ARG;
   c->profiling = level;
   return HESAFF_OK;
}

int hesaff_get_timings(const hesaff_ctx *c, hesaff_timings *t)
{
   if (!c || !t) return HESAFF_ERR_ARG;
   *t = c->tm;
   return HESAFF_OK;
}

int hesaff_detect_batch_device(hesaff_ctx *c, int n, const void *d_gray, int width, int height, int32_t *count_hessian,
                               int32_t *count_desc, const void **d_keys_out, int64_t *total_out)
{
   const ArmedMasks am = take_masks(c);
   if (!c || n < 1 || !d_gray) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   begin_device_batch(c, n);
   detect_device(c, n, SrcImages::u8(d_gray, 1, (long long)width * height, width), height, width, count_hessian, count_desc, d_keys_out, total_out, [] {}, am);
   HS_API_END(c)
}

// ------------------------------------------------------------------------------------------------------------------
// Chunk engine: the device side of every entry point that takes host images or files (hesaff_detect_batch, _cb, _regions,
// hesaff_describe_regions, hesaff_process_files).  The loop - which thread does what, in which order, and what happens
// to a chunk that is refused - is run_chunk_loop (chunk_engine.h); ChunkDevice is what that loop drives: every HIP call
// of a chunk, on the stream and the thread the loop's order puts it.
// ------------------------------------------------------------------------------------------------------------------
} // extern "C"

namespace {
using namespace hesaff_engine;

// the refusal of a float image with a pixel outside the domain (include/hesaff_amd.h): the caller's image index and the first such pixel
[[noreturn]] void throw_bad_f32(int index, const uint8_t *img, int H, int W, size_t stride)
{
   int row = 0, col = 0;
   float v = 0.0f;
   char msg[256];
   if (first_bad_f32(img, H, W, stride, &row, &col, &v))
      snprintf(msg, sizeof msg, "image %d: pixel (row %d, column %d) is %.9g; float input must be finite with |v| <= 2^20", index, row, col, (double)v);
   else
      snprintf(msg, sizeof msg, "image %d: a pixel is not finite or exceeds 2^20 in magnitude", index);
   throw HsError(HESAFF_ERR_ARG, msg);
}

// hesaff_describe_regions: why a caller's record is refused (include/hesaff_amd.h lists the rules), nullptr when it is accepted.
// n_oct: the octaves of this image's pyramid.  Runs on the staging thread while the records are copied into pinned memory, so no
// refused value reaches a kernel.
const char *describe_bad_record(const hesaff_region &r, int from, int n_oct)
{
   const float lim = 1048576.0f;   // 2^20
   if (r.type < 0 || r.type > 2) return "type is not 0, 1 or 2";
   if (!finite_f(r.x) || !finite_f(r.y) || !finite_f(r.s) || !finite_f(r.response)) return "x, y, s or response is not finite";
   if (fabsf(r.x) > lim || fabsf(r.y) > lim) return "|x| or |y| exceeds 2^20";
   if (!(r.s > 0.0f && r.s <= lim)) return "s is not in (0, 2^20]";
   if (from == HESAFF_FROM_POINTS) {
      if (r.octave < 0 || r.octave >= n_oct) return "octave is outside this image's pyramid";
      if (r.level < 0 || r.level >= HS_NSCALES) return "level is not one the detector finds keypoints on (0..2)";
      return nullptr;
   }
   const float a[4] = {r.a11, r.a12, r.a21, r.a22};
   for (float v : a) {
      if (!finite_f(v)) return "a11..a22 is not finite";
      if (fabsf(v) > lim) return "|a_ij| exceeds 2^20";
   }
   // rectifyAffineTransformationUpIsUp divides by both (helpers.cpp:90-97), in double
   if ((double)r.a11 * (double)r.a22 - (double)r.a12 * (double)r.a21 == 0.0) return "a11 * a22 - a12 * a21 is zero";
   if ((double)r.a11 * (double)r.a11 + (double)r.a12 * (double)r.a12 == 0.0) return "a11^2 + a12^2 is zero";
   return nullptr;
}

void ensure_copy_streams(hesaff_ctx *c)
{
   if (c->slot[1].ev_exp[3]) return;   // (the last thing made below)
   // The copy streams get a priority of their own: the runtime multiplexes the streams of one priority onto a few hardware queues
   // (four by default; this context has four compute streams), and a copy command holds its queue until the copy engine is done -
   // 23 ms for the 1.3 GB of text of a chunk, during which the patch kernels of whatever stream shared that queue did not start
   // (measured: +19 ms on the patch stage of every chunk, profiles/r04_notes.md).  Streams of another priority live on other queues.
   int prio_least = 0, prio_greatest = 0;
   HIP_TRY(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
   if (!(c->sset.h2d && c->sset.d2h)) {   // (else: the copy streams of the context that had this set before)
      HIP_TRY(hipStreamCreateWithPriority(&c->sset.h2d, hipStreamNonBlocking, prio_greatest));
      HIP_TRY(hipStreamCreateWithPriority(&c->sset.d2h, hipStreamNonBlocking, prio_greatest));
   }
   for (hesaff_ctx::ChunkSlot &sl : c->slot) {
      sl.ev_h2d = DevEvent(hipEventDisableTiming);
      sl.ev_h2d_blk = DevEvent(hipEventDisableTiming | hipEventBlockingSync);
      sl.ev_in_free = DevEvent(hipEventDisableTiming | hipEventBlockingSync);
      sl.ev_out_ready = DevEvent(hipEventDisableTiming);
      sl.ev_d2h = DevEvent(hipEventDisableTiming | hipEventBlockingSync);
      for (DevEvent &e : sl.ev_exp) e = DevEvent(hipEventDefault);
   }
}

// The device of run_chunk_loop (chunk_engine.h) for one call.  stage runs on the staging thread, everything else on the caller's.
struct ChunkDevice {
   using State = ChunkState;
   using Slot = hesaff_ctx::ChunkSlot;
   using Clock = std::chrono::steady_clock;
   hesaff_ctx *c;
   const int wants, ring;
   std::vector<std::future<void>> presize;   // ring blocks being pinned on a helper thread
   bool presized = false;
   // the tuning build's per-chunk lines (HESAFF_DEBUG): when the caller's thread began to wait for the chunk, got it, had run its
   // batch and had laid out its block, and the thread's CPU time at the first three
   Clock::time_point dbg_t0, dbg_t1, dbg_t2, dbg_t3;
   double dbg_c0 = 0.0, dbg_c1 = 0.0, dbg_c2 = 0.0;

   ChunkDevice(hesaff_ctx *c_, int wants_, int ring_) : c(c_), wants(wants_), ring(ring_), presize((size_t)std::max(ring_, 0))
   {
      bind_device(c);
      ensure_copy_streams(c);
      if (ring > 0 && (int)c->pin_out.size() < ring) c->pin_out.resize((size_t)ring);
      dbg_next_chunk();
   }
   ~ChunkDevice() { for (auto &x : presize) if (x.valid()) x.wait(); }   // no helper outlives the call
   void dbg_next_chunk() { dbg_t0 = Clock::now(); dbg_c0 = c->debug ? thread_cpu_ms() : 0.0; }
   bool times_export(const State &s) const { return c->profiling && (wants & (WANT_TEXT | WANT_BIN)) && s.total > 0; }

   // chunk -> pinned buffer -> the slot's device input buffer on the H2D stream; runs while the chunk before computes
   void stage(State &s)
   {
      HIP_TRY(hipSetDevice(c->device));
      const HostChunk &q = s.q;
      Slot &sl = c->slot[s.no & 1];
      const size_t row_bytes = (size_t)q.W * q.bpp(), img_bytes = row_bytes * q.H;
      // what travels per image: its pixels, or - a JPEG file - its coefficient blob (the pixels are then made in b_in2 by the device)
      const size_t unit = q.blob_bytes ? q.blob_bytes : img_bytes, total = unit * q.data.size();
      hs_wait_event(sl.ev_in_free);   // the chunk two before no longer reads this input buffer (never recorded: returns at once)
      s.largest = std::max<int>((int)q.data.size(), std::min(s.largest, c->par.max_batch));
      sl.b_in2.ensure(img_bytes * (size_t)s.largest);
      if (q.blob_bytes) sl.b_jcoef.ensure(unit * (size_t)s.largest);
      if (q.pinned) {
         // the readers filled page-locked buffers of this context (PinHooks): every image goes to the device from where it is, and its
         // buffer is given back to the readers (ChunkIO::staged) when the copy engine has read it (this thread sleeps on a blocking
         // event meanwhile)
         uint8_t *dst = (uint8_t *)(q.blob_bytes ? sl.b_jcoef.p : sl.b_in2.p);
         for (size_t b = 0; b < q.data.size(); b++)
            HIP_TRY(hipMemcpyAsync(dst + unit * b, q.data[b], unit, hipMemcpyHostToDevice, c->sset.h2d));
         HIP_TRY(hipEventRecord(sl.ev_h2d, c->sset.h2d));
         HIP_TRY(hipEventRecord(sl.ev_h2d_blk, c->sset.h2d));
         hs_wait_event(sl.ev_h2d_blk);
         return;
      }
      sl.pin_in.ensure(unit * (size_t)s.largest);   // sized once, for the large chunks that follow a small first one
      // pixels into the pinned buffer: a chunk of 64 UHD images is 0.5 GB (2.1 GB as float planes) - on four threads when it is worth
      // it (the first chunk's copy is the pipeline's fill: nothing runs on the device meanwhile).  Float planes are checked in the same
      // pass (copy_row_f32): the first image of a share with a pixel outside the domain stops that share and is reported below.
      const size_t nimg = q.data.size();
      std::vector<size_t> bad_img(nimg + 1, nimg);   // per share: the first refused image (nimg: none)
      auto copy_images = [&](size_t b0, size_t b1) {
         for (size_t b = b0; b < b1; b++) {
            uint8_t *dst = (uint8_t *)sl.pin_in.p + unit * b;
            if (q.blob_bytes) { memcpy(dst, q.data[b], unit); continue; }
            const size_t stride = q.stride[b];
            if (q.f32) {
               for (int y = 0; y < q.H; y++)
                  if (!copy_row_f32(dst + row_bytes * y, q.data[b] + stride * y, q.W)) { bad_img[b0] = b; return; }
               continue;
            }
            if (stride == row_bytes) memcpy(dst, q.data[b], img_bytes);
            else for (int y = 0; y < q.H; y++) memcpy(dst + row_bytes * y, q.data[b] + stride * y, row_bytes);
         }
      };
      const size_t nthr = (total >= ((size_t)32 << 20) && nimg >= 4) ? (size_t)std::max(1, std::min(4, c->stage_threads)) : 1;
      {
         std::vector<std::thread> th;
         size_t t = 1;
         try {
            for (; t < nthr; t++) th.emplace_back(copy_images, nimg * t / nthr, nimg * (t + 1) / nthr);
         } catch (...) {   // a thread that cannot be started: its share (and the rest) is copied right here
         }
         copy_images(0, nimg / nthr);
         if (t < nthr) copy_images(nimg * t / nthr, nimg);
         for (auto &x : th) x.join();
      }
      if (q.f32) {
         const size_t b = *std::min_element(bad_img.begin(), bad_img.end());
         if (b < nimg) throw_bad_f32(q.index[b], q.data[b], q.H, q.W, q.stride[b]);
      }
      if (q.from) {
         // the chunk's records travel with it: [B + 1 starts][records] into pinned memory, each record checked on the way, one copy in
         const int n_oct = (int)pyramid_geometry(q.H, q.W, c->ct.up).oct.size();
         unsigned long long n_rec = 0;
         for (int cnt : q.region_count) n_rec += (unsigned long long)cnt;
         if (n_rec > 0x7fffffffull) throw HsError(HESAFF_ERR_CAPACITY, "more records in a chunk than 32-bit indices hold");
         const size_t rec_at = describe_records_offset((int)nimg), bytes = rec_at + (size_t)n_rec * sizeof(hesaff_region);
         sl.pin_reg.ensure_grow(bytes);
         sl.b_reg.ensure_grow(bytes);
         int32_t *starts = (int32_t *)sl.pin_reg.p;
         hesaff_region *dst = (hesaff_region *)((char *)sl.pin_reg.p + rec_at);
         size_t at = 0;
         for (size_t b = 0; b < nimg; b++) {
            starts[b] = (int32_t)at;
            const hesaff_region *src = q.regions[b];
            for (int i = 0; i < q.region_count[b]; i++) {
               if (const char *why = describe_bad_record(src[i], q.from, n_oct)) {
                  char msg[256];
                  snprintf(msg, sizeof msg, "image %d: record %d: %s", q.index[b], i, why);
                  throw HsError(HESAFF_ERR_ARG, msg);
               }
               dst[at + (size_t)i] = src[i];
            }
            at += (size_t)q.region_count[b];
         }
         starts[nimg] = (int32_t)at;
         s.n_rec = (uint32_t)at;
         HIP_TRY(hipMemcpyAsync(sl.b_reg.p, sl.pin_reg.p, bytes, hipMemcpyHostToDevice, c->sset.h2d));
      }
      if (!q.masks.empty()) {
         // the chunk's masks travel with it: [present bytes][tight planes] into pinned memory, one copy in beside the pixels
         const size_t bytes = mask_block_bytes((int)nimg, q.H, q.W);
         sl.pin_mask.ensure_grow(bytes);
         sl.b_mask.ensure_grow(bytes);
         fill_mask_block((uint8_t *)sl.pin_mask.p, mask_planes_offset((int)nimg), q);
         HIP_TRY(hipMemcpyAsync(sl.b_mask.p, sl.pin_mask.p, bytes, hipMemcpyHostToDevice, c->sset.h2d));
      }
      HIP_TRY(hipMemcpyAsync(q.blob_bytes ? sl.b_jcoef.p : sl.b_in2.p, sl.pin_in.p, total, hipMemcpyHostToDevice, c->sset.h2d));
      HIP_TRY(hipEventRecord(sl.ev_h2d, c->sset.h2d));
   }

   // the chunk's batch, its per-image counts and the layout of its result block.  ev_in_free of the slot is recorded when the batch has
   // run and when the chunk is refused (HESAFF_ERR_ARG, HESAFF_ERR_CAPACITY: both are thrown with the main stream idle), not on other errors
   void compute(State &s)
   {
      dbg_t1 = Clock::now();
      dbg_c1 = c->debug ? thread_cpu_ms() : 0.0;
      const HostChunk &q = s.q;
      Slot &sl = c->slot[s.no & 1];
      const int B = (int)q.data.size();
      const size_t row_bytes = (size_t)q.W * q.bpp(), img_bytes = row_bytes * q.H;
      HIP_TRY(hipStreamWaitEvent(c->stream(), sl.ev_h2d, 0));
      BatchResult res = {};
      try {
         plan(c, std::max(std::min<int>(c->par.max_batch, B), s.largest), q.H, q.W);
         // a chunk of JPEG files: inverse DCT, up-sampling and colour conversion of all its images (kernels_jpeg.h) into the input slot
         if (q.blob_bytes) jpeg_pixels(c, sl.b_jcoef.as<uint8_t>(), make_jpeg_geom(q.jpeg), B, (uint8_t *)sl.b_in2.p, img_bytes, c->stream());
         const SrcImages src = q.f32 ? SrcImages::f32(sl.b_in2.p, (long long)img_bytes, (int)row_bytes)
                                     : SrcImages::u8(sl.b_in2.p, q.ch, (long long)img_bytes, (int)row_bytes);
         SelMasks mk;
         if (!q.masks.empty()) {
            mk.present = (const uint8_t *)sl.b_mask.p; mk.base = mk.present + mask_planes_offset(B);
            mk.img_stride = (long long)q.H * q.W; mk.row_stride = q.W; mk.W = q.W; mk.H = q.H;
         }
         res = q.from ? run_describe(c, src, B, q.H, q.W, (const uint8_t *)sl.b_reg.p, s.n_rec, q.from) : run_batch(c, src, B, q.H, q.W, mk);
      } catch (const HsError &e) {
         if (e.code == HESAFF_ERR_ARG || e.code == HESAFF_ERR_CAPACITY) {
            HIP_TRY(hipEventRecord(sl.ev_in_free, c->stream()));
            dbg_next_chunk();
         }
         throw;
      }
      HIP_TRY(hipEventRecord(sl.ev_in_free, c->stream()));
      dbg_t2 = Clock::now();
      dbg_c2 = c->debug ? thread_cpu_ms() : 0.0;
      const int32_t *hs = res.hessian_starts, *ds = res.desc_starts;
      s.total = ds[B];
      s.n_hess = (size_t)hs[B];
      s.nh.resize((size_t)B); s.nd.resize((size_t)B); s.off.resize((size_t)B);
      for (int b = 0; b < B; b++) {
         s.nh[(size_t)b] = hs[b + 1] - hs[b];
         s.nd[(size_t)b] = ds[b + 1] - ds[b];
         s.off[(size_t)b] = (size_t)ds[b];
      }
      const size_t n_rows = (size_t)s.total;
      size_t at = 0;
      auto place = [&at](size_t bytes) { const size_t o = at; at = (at + bytes + 255) & ~(size_t)255; return o; };
      if (wants & WANT_KEYS) s.keys_at = place(n_rows * sizeof(hesaff_keypoint));
      if (wants & WANT_WORDS) s.words_at = place(n_rows * 8);
      if (wants & WANT_REGIONS) s.regions_at = place(s.n_hess * sizeof(hesaff_region));
      if (times_export(s)) HIP_TRY(hipEventRecord(sl.ev_exp[0], c->stream()));
      if (wants & WANT_TEXT) {   // row lengths and offsets first: the host needs the byte count (a short wait on the main stream)
         const unsigned long long text_bytes = export_text_prepare(c, c->geo.b_out.as<KeyRec>(), (uint32_t)n_rows, res.d_desc_starts, B, s.toff);
         s.text_at = place((size_t)text_bytes);
      }
      if (wants & WANT_BIN) s.bin_at = place(n_rows * EX_BIN_ROW);
      if (wants & WANT_SIGS) s.sigs_at = place(n_rows * 8);
      if (wants & WANT_NEIGH) s.neigh_at = place(n_rows * 8 * (size_t)c->neighbours);
      if (wants & WANT_NSIGS) {   // the signatures of the ranks above 0 that every key has, a plane per rank (rank 0 is b_sigs)
         s.nsigs_at = place(n_rows * 8 * (size_t)(c->neighbours - 1));
         embed_batch_ranks(c, (long long)n_rows);
      }
      if (times_export(s)) HIP_TRY(hipEventRecord(sl.ev_exp[1], c->stream()));
      s.bytes = at;
      dbg_t3 = Clock::now();
   }

   // s.block is chosen: the block is sized, then the device copy / formatting into the staging slot (frees b_out for the next chunk)
   // and the D2H beside the next chunk
   void copy_out(State &s)
   {
      Slot &sl = c->slot[s.no & 1];
      const int B = (int)s.q.data.size();
      const size_t bytes = s.bytes, n_rows = (size_t)s.total;
      if (ring > 0) {
         // A list that starts with small chunks (a long one): every block of the ring is sized for a FULL chunk of this density the
         // first time one is needed, the other blocks on a helper thread beside the next chunk's kernels: pinning 1.5 GB takes
         // 150 ms, and a block that is sized - or grown - when its chunk is already waiting leaves the device idle for that long.
         const int follow = std::max(s.largest, B);   // images of the largest chunk that is known to follow (ChunkIO::largest_chunk)
         const size_t full = (bytes * (size_t)follow + (size_t)B - 1) / (size_t)B;
         if (presize[(size_t)s.block].valid()) presize[(size_t)s.block].get();
         PinBuf &pb = c->pin_out[(size_t)s.block];
         if (bytes > pb.bytes) pb.ensure_grow(std::max<size_t>(full, 16));
         if (!presized && follow > B) {   // a list that starts small is a long one: its other blocks will be needed
            presized = true;
            for (int r = 0; r < ring; r++)
               if (r != s.block && c->pin_out[(size_t)r].bytes == 0)
                  presize[(size_t)r] = std::async(std::launch::async, [c = c, r, full] {
                     if (hipSetDevice(c->device) != hipSuccess) return;
                     try { c->pin_out[(size_t)r].ensure_grow(std::max<size_t>(full, 16)); } catch (const HsError &) {}   // asked for again, and reported, when the block is needed
                  });
         }
      } else {   // a block per chunk, kept until the next call
         if ((int)c->pin_out.size() <= s.block) c->pin_out.resize((size_t)s.block + 1);
         c->pin_out[(size_t)s.block].ensure(std::max<size_t>(bytes, 16));
      }
      s.copied = s.total > 0 || ((wants & WANT_REGIONS) && s.n_hess > 0);
      if (s.copied) {
         const KeyRec *d_keys = c->geo.b_out.as<KeyRec>();
         HIP_TRY(hipStreamWaitEvent(c->stream(), sl.ev_d2h, 0));      // the D2H of the chunk two before has left this staging slot
         if (bytes > sl.b_outstage.bytes) sl.b_outstage.ensure(bytes + bytes / 4);
         char *stg = (char *)sl.b_outstage.p;
         if ((wants & WANT_KEYS) && n_rows > 0)
            HIP_TRY(hipMemcpyAsync(stg + s.keys_at, c->geo.b_out.p, n_rows * sizeof(hesaff_keypoint), hipMemcpyDeviceToDevice, c->stream()));
         if ((wants & WANT_WORDS) && n_rows > 0)   // (b_words: written by k_assign_words behind the pack stage, on this stream)
            HIP_TRY(hipMemcpyAsync(stg + s.words_at, c->b_words.p, n_rows * 8, hipMemcpyDeviceToDevice, c->stream()));
         if ((wants & WANT_SIGS) && n_rows > 0)    // (b_sigs: written by k_embed_keys behind b_words, on this stream)
            HIP_TRY(hipMemcpyAsync(stg + s.sigs_at, c->b_sigs.p, n_rows * 8, hipMemcpyDeviceToDevice, c->stream()));
         if ((wants & WANT_NEIGH) && n_rows > 0)   // (b_neigh: written by k_assign_neighbours with b_words, on this stream)
            HIP_TRY(hipMemcpyAsync(stg + s.neigh_at, c->b_neigh.p, n_rows * 8 * (size_t)c->neighbours, hipMemcpyDeviceToDevice, c->stream()));
         if ((wants & WANT_NSIGS) && n_rows > 0)   // (b_nsigs: written by embed_batch_ranks in compute(), on this stream)
            HIP_TRY(hipMemcpyAsync(stg + s.nsigs_at, c->b_nsigs.p, n_rows * 8 * (size_t)(c->neighbours - 1), hipMemcpyDeviceToDevice, c->stream()));
         if (wants & WANT_REGIONS) pack_regions(c, (uint32_t)s.n_hess, B, (hesaff_region *)(stg + s.regions_at));
         if (times_export(s)) HIP_TRY(hipEventRecord(sl.ev_exp[2], c->stream()));
         if (wants & WANT_TEXT) export_text_write(c, d_keys, (uint32_t)n_rows, stg + s.text_at);
         if (wants & WANT_BIN) export_bin_rows(c, d_keys, (uint32_t)n_rows, stg + s.bin_at);
         if (times_export(s)) HIP_TRY(hipEventRecord(sl.ev_exp[3], c->stream()));
         HIP_TRY(hipEventRecord(sl.ev_out_ready, c->stream()));
         HIP_TRY(hipStreamWaitEvent(c->sset.d2h, sl.ev_out_ready, 0));
         HIP_TRY(hipMemcpyAsync(c->pin_out[(size_t)s.block].p, stg, bytes, hipMemcpyDeviceToHost, c->sset.d2h));
         HIP_TRY(hipEventRecord(sl.ev_d2h, c->sset.d2h));
      }
      if (c->debug) {
         auto ms = [](Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
         const auto dbg_t5 = Clock::now();
         fprintf(stderr, "[hesaff] chunk %d: caller's CPU: wait staged %.1f run_batch %.1f rest %.1f ms\n", s.no, dbg_c1 - dbg_c0, dbg_c2 - dbg_c1, thread_cpu_ms() - dbg_c2);
         fprintf(stderr, "[hesaff] chunk %d: wait staged %.1f  run_batch %.1f  export prepare %.1f  deliver prev %.1f  acquire+enqueue %.1f ms | device: pyramid %.1f detect %.1f affine %.1f patch %.1f sift %.1f pack %.1f total %.1f\n", s.no, ms(dbg_t0, dbg_t1),
                 ms(dbg_t1, dbg_t2), ms(dbg_t2, dbg_t3), ms(dbg_t3, s.delivered), ms(s.delivered, dbg_t5), c->tm.pyramid_ms, c->tm.detect_ms, c->tm.affine_ms, c->tm.patch_ms, c->tm.sift_ms, c->tm.pack_ms, c->tm.total_ms);
      }
      dbg_next_chunk();
   }

   // the chunk's copy out has landed: the base of its result block (and, when profiling, what its export passes took)
   const char *wait_out(State &s)
   {
      Slot &sl = c->slot[s.no & 1];
      if (s.copied) hs_wait_event(sl.ev_d2h);
      if (times_export(s)) {
         float ms = 0.0f;   // length pass (with the host's short wait for the byte counts) + write pass
         float ms2 = 0.0f;
         if (hipEventElapsedTime(&ms, sl.ev_exp[0], sl.ev_exp[1]) == hipSuccess && hipEventElapsedTime(&ms2, sl.ev_exp[2], sl.ev_exp[3]) == hipSuccess) {
            ms += ms2; c->export_ms = ms; c->export_rows = s.total; c->tm.export_ms = ms; c->tm.export_rows = s.total; }
         else (void)hipGetLastError();
      }
      return (const char *)c->pin_out[(size_t)s.block].p;
   }

   void drain()
   {
      (void)hipStreamSynchronize(c->sset.h2d);
      (void)hipStreamSynchronize(c->sset.d2h);
      (void)hipStreamSynchronize(c->stream());
   }
   void finish()
   {
      HIP_TRY(hipStreamSynchronize(c->sset.d2h));
      HIP_TRY(hipStreamSynchronize(c->stream()));
   }
};

void run_chunks(hesaff_ctx *c, ChunkIO &io, int ring)
{
   ChunkDevice dev(c, io.wants(), ring);
   run_chunk_loop(io, c->ring, ring, dev);
}

// what ArrayIO (chunk_engine.h) takes for granted
void validate_image_list(int n, const uint8_t *const *images, const int *widths, const int *heights, const int *strides, const int *channels)
{
   for (int j = 0; j < n; j++) {
      const int W = widths[j], H = heights[j], ch = channels ? channels[j] : 1;
      if (ch != 1 && ch != 3) throw HsError(HESAFF_ERR_ARG, "channels must be 1 or 3");
      if (!images[j] || W < 1 || H < 1) throw HsError(HESAFF_ERR_ARG, "bad image");
      if (strides && (long long)strides[j] < (long long)W * ch) throw HsError(HESAFF_ERR_ARG, "row stride smaller than width * channels");
   }
}

// the same for the float entry points (include/hesaff_amd.h: input layout); -> the image pointers as ArrayIO holds them
std::vector<const uint8_t *> validate_f32_list(int n, const float *const *images, const int *widths, const int *heights, const int *strides)
{
   std::vector<const uint8_t *> bytes((size_t)n);
   for (int j = 0; j < n; j++) {
      const int W = widths[j], H = heights[j];
      if (!images[j] || W < 1 || H < 1) throw HsError(HESAFF_ERR_ARG, "bad image");
      if ((uintptr_t)images[j] % 4 != 0) throw HsError(HESAFF_ERR_ARG, "float image pointer not 4-byte aligned");
      if (strides && ((long long)strides[j] < 4LL * W || strides[j] % 4 != 0))
         throw HsError(HESAFF_ERR_ARG, "row stride of a float image must be at least 4 * width bytes and a multiple of 4");
      bytes[(size_t)j] = reinterpret_cast<const uint8_t *>(images[j]);
   }
   return bytes;
}

// hesaff_detect_batch_device_f32's check of n planes in device memory (capi_stage.h: its flags are an array of the stage buffer)
void check_device_f32(hesaff_ctx *c, int n, const uint8_t *d, long long img_stride, int row_stride, int H, int W);

// The body of the six host-image entry points: the list is validated, cut into chunks (ArrayIO), given its consumer - set_consumer
// fills in `results`, `region_results` or `sink` + `user` - and run through the chunk engine with `ring` result blocks.
// images: n pointers to 8-bit images (const uint8_t *const *, with `channels`) or, f32, to float planes (const float *const *).
struct DescribeInput { const hesaff_region *const *regions = nullptr; const int *counts = nullptr; int from = 0; };

// the armed masks against the images of the host call that takes them -> what ArrayIO deals out with the images
MaskInput host_masks(const ArmedMasks &am, int n, const int *widths)
{
   MaskInput mi;
   if (am.kind == ArmedMasks::NONE) return mi;
   if (am.kind != ArmedMasks::HOST) throw HsError(HESAFF_ERR_ARG, "masks armed with hesaff_set_next_masks_device met a host-image call; the masks are cleared");
   char msg[160];
   if (am.n != n) {
      snprintf(msg, sizeof msg, "%d masks armed for a call with %d images; the masks are cleared", am.n, n);
      throw HsError(HESAFF_ERR_ARG, msg);
   }
   if (!am.strides.empty())
      for (int j = 0; j < n; j++)
         if (am.masks[(size_t)j] && am.strides[(size_t)j] < widths[j]) {
            snprintf(msg, sizeof msg, "image %d: row stride of its mask (%d) smaller than the width (%d); the masks are cleared", j, am.strides[(size_t)j], widths[j]);
            throw HsError(HESAFF_ERR_ARG, msg);
         }
   mi.masks = am.masks.data();
   mi.strides = am.strides.empty() ? nullptr : am.strides.data();
   return mi;
}

template <class CONSUMER>
void detect_images(hesaff_ctx *c, int n, const void *images, bool f32, const int *widths, const int *heights, const int *strides, const int *channels,
                   int ring, CONSUMER set_consumer, const ArmedMasks &am, const DescribeInput &di = DescribeInput())
{
   std::vector<const uint8_t *> planes;
   if (f32) planes = validate_f32_list(n, (const float *const *)images, widths, heights, strides);
   else validate_image_list(n, (const uint8_t *const *)images, widths, heights, strides, channels);
   const MaskInput mi = host_masks(am, n, widths);
   ArrayIO io(&c->ring, c->par.max_batch, n, f32 ? planes.data() : (const uint8_t *const *)images, widths, heights, strides, channels, f32,
              di.regions, di.counts, di.from, mi);
   c->words_device_total = -1;
   c->word_spans.clear();
   c->sig_spans.clear();
   c->sigs_device_total = -1;
   c->neigh_spans.clear();
   c->neigh_device_total = -1;
   if (c->vocab.k) {   // the words travel beside the keys (WANT_WORDS); hesaff_get_words finds them by the caller's image index
      c->word_spans.assign((size_t)n, WordSpan());
      io.word_spans = &c->word_spans;
      if (c->neighbours > 1) {   // ... and so do the neighbours (WANT_NEIGH; hesaff_get_neighbours)
         c->neigh_spans.assign((size_t)n, NeighSpan());
         c->neigh_spans_r = c->neighbours;
         io.neigh_spans = &c->neigh_spans;
         io.neigh_r = c->neighbours;
      }
      if (c->embed.set) {   // ... and so do the signatures (WANT_SIGS; hesaff_get_signatures)
         c->sig_spans.assign((size_t)n, SigSpan());
         io.sig_spans = &c->sig_spans;
      }
   }
   set_consumer(io);
   run_chunks(c, io, ring);
   c->neigh_device_total = -1;   // (b_neigh holds the last chunk's rows only)
   if (io.sink_rc.load() != 0) throw HsError(HESAFF_ERR_IO, "the result sink reported an error");
}

} // namespace

extern "C" {

int hesaff_detect_batch(hesaff_ctx *c, int n, const uint8_t *const *images, const int *widths, const int *heights,
                        const int *strides, const int *channels, hesaff_result *results)
{
   const ArmedMasks am = take_masks(c);
   if (!c || n < 0 || (n > 0 && (!images || !widths || !heights || !results))) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   detect_images(c, n, images, false, widths, heights, strides, channels, 0, [&](ArrayIO &io) { io.results = results; }, am);
   HS_API_END(c)
}

int hesaff_detect_batch_cb(hesaff_ctx *c, int n, const uint8_t *const *images, const int *widths, const int *heights,
                           const int *strides, const int *channels, hesaff_chunk_sink sink, void *user)
{
   const ArmedMasks am = take_masks(c);
   if (!c || n < 0 || !sink || (n > 0 && (!images || !widths || !heights))) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   detect_images(c, n, images, false, widths, heights, strides, channels, 3, [&](ArrayIO &io) { io.sink = sink; io.user = user; }, am);
   HS_API_END(c)
}

// the chunks of hesaff_detect_batch, each with a block of hesaff_region records beside its keys (k_pack_regions, launched in ChunkDevice's
// copy_out into the staging slot: the records leave on the chunk's one copy out)
int hesaff_detect_regions(hesaff_ctx *c, int n, const uint8_t *const *images, const int *widths, const int *heights,
                          const int *strides, const int *channels, hesaff_region_result *results)
{
   const ArmedMasks am = take_masks(c);
   if (!c || n < 0 || (n > 0 && (!images || !widths || !heights || !results))) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   detect_images(c, n, images, false, widths, heights, strides, channels, 0, [&](ArrayIO &io) { io.region_results = results; }, am);
   HS_API_END(c)
}

// ---- float grey planes (CV_32FC1, pyramid.h:73): the same paths with the float source format ----
int hesaff_detect_batch_f32(hesaff_ctx *c, int n, const float *const *images, const int *widths, const int *heights, const int *strides,
                            hesaff_result *results)
{
   const ArmedMasks am = take_masks(c);
   if (!c || n < 0 || (n > 0 && (!images || !widths || !heights || !results))) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   detect_images(c, n, images, true, widths, heights, strides, nullptr, 0, [&](ArrayIO &io) { io.results = results; }, am);
   HS_API_END(c)
}

int hesaff_detect_batch_cb_f32(hesaff_ctx *c, int n, const float *const *images, const int *widths, const int *heights, const int *strides,
                               hesaff_chunk_sink sink, void *user)
{
   const ArmedMasks am = take_masks(c);
   if (!c || n < 0 || !sink || (n > 0 && (!images || !widths || !heights))) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   detect_images(c, n, images, true, widths, heights, strides, nullptr, 3, [&](ArrayIO &io) { io.sink = sink; io.user = user; }, am);
   HS_API_END(c)
}

int hesaff_detect_regions_f32(hesaff_ctx *c, int n, const float *const *images, const int *widths, const int *heights, const int *strides,
                              hesaff_region_result *results)
{
   const ArmedMasks am = take_masks(c);
   if (!c || n < 0 || (n > 0 && (!images || !widths || !heights || !results))) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   detect_images(c, n, images, true, widths, heights, strides, nullptr, 0, [&](ArrayIO &io) { io.region_results = results; }, am);
   HS_API_END(c)
}

// ---- hesaff_describe_regions: the chunks of hesaff_detect_regions with the caller's records in the place of detection's ----
} // extern "C"
namespace {
DescribeInput describe_input(int n, const hesaff_region *const *regions, const int *counts, int from)
{
   if (from != HESAFF_FROM_POINTS && from != HESAFF_FROM_SHAPES) throw HsError(HESAFF_ERR_ARG, "from must be HESAFF_FROM_POINTS (1) or HESAFF_FROM_SHAPES (2)");
   for (int j = 0; j < n; j++) {
      char msg[128];
      if (counts[j] < 0) { snprintf(msg, sizeof msg, "image %d: negative record count", j); throw HsError(HESAFF_ERR_ARG, msg); }
      if (counts[j] > 0 && !regions[j]) { snprintf(msg, sizeof msg, "image %d: %d records but no record pointer", j, counts[j]); throw HsError(HESAFF_ERR_ARG, msg); }
   }
   DescribeInput di;
   di.regions = regions; di.counts = counts; di.from = from;
   return di;
}
} // namespace
extern "C" {

int hesaff_describe_regions(hesaff_ctx *c, int n, const uint8_t *const *images, const int *widths, const int *heights, const int *strides,
                            const int *channels, const hesaff_region *const *regions, const int *counts, int from, hesaff_region_result *results)
{
   const ArmedMasks am = take_masks(c);
   if (!c || n < 0 || (n > 0 && (!images || !widths || !heights || !regions || !counts || !results))) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   refuse_masks(am, "hesaff_describe_regions takes none: its records are the caller's");
   const DescribeInput di = describe_input(n, regions, counts, from);
   detect_images(c, n, images, false, widths, heights, strides, channels, 0, [&](ArrayIO &io) { io.region_results = results; }, am, di);
   HS_API_END(c)
}

int hesaff_describe_regions_f32(hesaff_ctx *c, int n, const float *const *images, const int *widths, const int *heights, const int *strides,
                                const hesaff_region *const *regions, const int *counts, int from, hesaff_region_result *results)
{
   const ArmedMasks am = take_masks(c);
   if (!c || n < 0 || (n > 0 && (!images || !widths || !heights || !regions || !counts || !results))) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   refuse_masks(am, "hesaff_describe_regions takes none: its records are the caller's");
   const DescribeInput di = describe_input(n, regions, counts, from);
   detect_images(c, n, images, true, widths, heights, strides, nullptr, 0, [&](ArrayIO &io) { io.region_results = results; }, am, di);
   HS_API_END(c)
}

int hesaff_detect_batch_device_f32(hesaff_ctx *c, int n, const void *d_planes, int width, int height, int row_stride, int64_t img_stride,
                                   int32_t *count_hessian, int32_t *count_desc, const void **d_keys_out, int64_t *total_out)
{
   const ArmedMasks am = take_masks(c);
   if (!c || n < 1 || !d_planes || width < 1 || height < 1 || row_stride < 0 || img_stride < 0) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   begin_device_batch(c, n);
   const long long rs = row_stride ? row_stride : 4LL * width;
   const long long is = img_stride ? (long long)img_stride : rs * height;
   if ((uintptr_t)d_planes % 4 != 0) throw HsError(HESAFF_ERR_ARG, "float planes not 4-byte aligned");
   if (rs < 4LL * width || rs % 4 != 0 || rs > 0x7fffffffLL)
      throw HsError(HESAFF_ERR_ARG, "row stride of a float plane must be at least 4 * width bytes and a multiple of 4");
   if (is % 4 != 0 || (n > 1 && is < rs * (height - 1) + 4LL * width))
      throw HsError(HESAFF_ERR_ARG, "image stride of the float planes must be a multiple of 4 and keep the images apart");
   detect_device(c, n, SrcImages::f32(d_planes, is, (int)rs), height, width, count_hessian, count_desc, d_keys_out, total_out,
                 [&] { check_device_f32(c, n, (const uint8_t *)d_planes, is, (int)rs, height, width); }, am);
   HS_API_END(c)
}

int hesaff_set_output_format(hesaff_ctx *c, int format)
{
   if (!c || (format & ~(HESAFF_OUT_TEXT | HESAFF_OUT_BIN | HESAFF_OUT_WORDS)) != 0 || format == 0) return HESAFF_ERR_ARG;
   c->out_format = format;
   return HESAFF_OK;
}

int hesaff_set_resume(hesaff_ctx *c, int on)
{
   if (!c || on < 0 || on > 2) return HESAFF_ERR_ARG;
   c->resume = on;
   return HESAFF_OK;
}

int hesaff_set_pinned_read_budget(hesaff_ctx *c, size_t max_bytes, size_t keep_bytes)
{
   if (!c) return HESAFF_ERR_ARG;
   {
      std::lock_guard<std::mutex> lk(c->pin_read.mu);
      c->pin_read.max_bytes = max_bytes;
      c->pin_read.keep_bytes = std::min(keep_bytes, max_bytes);
   }
   c->pin_read.trim(c->pin_read.keep_bytes);
   return HESAFF_OK;
}

int hesaff_set_pool_priority(hesaff_ctx *c, int mode)
{
   if (!c || mode < -1 || mode > 1) return HESAFF_ERR_ARG;
   c->pool_priority = mode;
   return HESAFF_OK;
}

int hesaff_set_keypoint_limit(hesaff_ctx *c, int n)
{
   if (!c || n < 0) return HESAFF_ERR_ARG;
   if (n > 0 && n < c->grid_rows * c->grid_cols) return HESAFF_ERR_ARG;   // a quota of 0 per cell
   c->keypoint_limit = n;
   return HESAFF_OK;
}

int hesaff_get_keypoint_limit(const hesaff_ctx *c, int *n)
{
   if (!c || !n) return HESAFF_ERR_ARG;
   *n = c->keypoint_limit;
   return HESAFF_OK;
}

int hesaff_set_keypoint_grid(hesaff_ctx *c, int rows, int cols)
{
   if (!c || rows < 1 || cols < 1 || rows > HS_GRID_MAX_CELLS || cols > HS_GRID_MAX_CELLS || rows * cols > HS_GRID_MAX_CELLS) return HESAFF_ERR_ARG;
   if (c->keypoint_limit > 0 && c->keypoint_limit < rows * cols) return HESAFF_ERR_ARG;   // a quota of 0 per cell
   c->grid_rows = rows;
   c->grid_cols = cols;
   return HESAFF_OK;
}

int hesaff_get_keypoint_grid(const hesaff_ctx *c, int *rows, int *cols)
{
   if (!c || !rows || !cols) return HESAFF_ERR_ARG;
   *rows = c->grid_rows;
   *cols = c->grid_cols;
   return HESAFF_OK;
}

int hesaff_set_orientation(hesaff_ctx *c, int mode)
{
   if (!c || (mode != HESAFF_ORI_UP && mode != HESAFF_ORI_DOMINANT)) return HESAFF_ERR_ARG;
   c->orientation = mode;
   return HESAFF_OK;
}

int hesaff_set_orientation_count(hesaff_ctx *c, int k)
{
   if (!c || k < 1 || k > HS_ORI_MAX_COUNT) return HESAFF_ERR_ARG;
   c->orientation_count = k;
   return HESAFF_OK;
}

int hesaff_get_orientation_count(const hesaff_ctx *c, int *k)
{
   if (!c || !k) return HESAFF_ERR_ARG;
   *k = c->orientation_count;
   return HESAFF_OK;
}

int hesaff_get_orientation(const hesaff_ctx *c, int *mode)
{
   if (!c || !mode) return HESAFF_ERR_ARG;
   *mode = c->orientation;
   return HESAFF_OK;
}

int hesaff_set_descriptor(hesaff_ctx *c, int mode)
{
   if (!c || (mode != HESAFF_DESC_SIFT && mode != HESAFF_DESC_ROOTSIFT)) return HESAFF_ERR_ARG;
   c->descriptor = mode;
   return HESAFF_OK;
}

int hesaff_get_descriptor(const hesaff_ctx *c, int *mode)
{
   if (!c || !mode) return HESAFF_ERR_ARG;
   *mode = c->descriptor;
   return HESAFF_OK;
}

int hesaff_set_next_masks(hesaff_ctx *c, int n, const uint8_t *const *masks, const int *strides)
{
   if (!c || n < 0 || (n > 0 && !masks)) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   ArmedMasks am;
   if (n > 0 && masks) {
      am.kind = ArmedMasks::HOST; am.n = n;
      am.masks.assign(masks, masks + n);
      if (strides) am.strides.assign(strides, strides + n);
   }
   c->next_masks = std::move(am);
   HS_API_END(c)
}

int hesaff_set_next_masks_device(hesaff_ctx *c, int n, const void *d_masks, int row_stride, int64_t img_stride)
{
   if (!c || n < 0 || (n > 0 && !d_masks) || row_stride < 0 || img_stride < 0) return HESAFF_ERR_ARG;
   ArmedMasks am;
   if (n > 0) { am.kind = ArmedMasks::DEVICE; am.n = n; am.d_masks = d_masks; am.row_stride = row_stride; am.img_stride = img_stride; }
   c->next_masks = am;
   return HESAFF_OK;
}

int hesaff_process_files(hesaff_ctx *c, int n, const char *const *paths, const char *const *out_paths, int decode_threads,
                         int write_threads, hesaff_file_status *status)
{
   const ArmedMasks am = take_masks(c);
   if (!c || n < 0 || (n > 0 && (!paths || !status))) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   refuse_masks(am, "hesaff_process_files takes none: no masks travel with a file list");
   if ((c->out_format & HESAFF_OUT_WORDS) && c->vocab.k == 0) throw HsError(HESAFF_ERR_ARG, "HESAFF_OUT_WORDS is selected but no vocabulary is set (hesaff_set_vocabulary)");
   c->words_device_total = -1;
   c->word_spans.clear();
   c->sig_spans.clear();
   c->sigs_device_total = -1;
   c->neigh_spans.clear();
   c->neigh_device_total = -1;
   for (int i = 0; i < n; i++) { status[i].rc = HESAFF_ERR_IO; status[i].stage = HESAFF_FILE_PENDING; status[i].count_hessian = 0; status[i].count_desc = 0; }
   hesaff_host_plan hp;
   (void)hesaff_host_plan_for(1, &hp);   // "0 = auto": this context has the host to itself (callers that share it pass the counts of their own plan)
   const int dt = std::max(1, std::min(decode_threads > 0 ? decode_threads : hp.decode_threads, 64));
   const int wt = std::max(1, std::min(write_threads > 0 ? write_threads : hp.write_threads, 256));
   // the rows are formatted on the device (kernels_export.h): the writer threads only write()
   const bool device_jpeg = true;   // JPEG files: entropy decoding on the pool's threads, the pixels made on the device
   PinHooks pin;   // the readers fill page-locked buffers of this context: no malloc'ed image, no staging copy
   c->pin_read.device = c->device;
   pin.alloc = [](size_t bytes, void *user) -> void * { return ((hesaff_ctx *)user)->pin_read.take(bytes); };
   pin.release = [](void *p, size_t bytes, void *user) { ((hesaff_ctx *)user)->pin_read.give(p, bytes); };
   pin.user = c;
   // the pool's threads step down (nice 10) only where they would otherwise crowd out the caller's thread: a CPU-starved plan
   const bool nice_pool = c->pool_priority == 1 || (c->pool_priority < 0 && hesaff_host_threads() <= dt + wt + 1);
   FileIO io(&c->ring, c->par.max_batch, c->par.mrSize, c->out_format, n, paths, out_paths, status, dt, wt, true, c->resume, device_jpeg, pin, nice_pool, c->embed.set);
   io.vocabulary_size = c->vocab.k;
   io.neighbours = c->vocab.k ? c->neighbours : 1;   // (R > 1: a row per key and present rank in the words and signatures files)
   c->stage_threads = hesaff_stage_threads_for_pool(dt + wt);
   try {
      run_chunks(c, io, 3);
      io.wait_writers();
   } catch (...) {
      io.shutdown();
      c->pin_read.trim(c->pin_read.keep_bytes);
      throw;
   }
   io.shutdown();
   c->neigh_device_total = -1;   // (b_neigh holds the last chunk's rows only)
   c->pin_read.trim(c->pin_read.keep_bytes);   // a long-lived context does not keep the peak of its largest list pinned
   HS_API_END(c)
}

// ---------------------------------- visual words (kernels_words.h) ----------------------------------
} // extern "C"
namespace {
// The vocabulary as k_assign_words reads it: XORed with 0x80, padded to whole tiles of HS_WORD_TILE rows, in lane order - tile t, step
// s, lane l: bytes [32 s + 16 (l >> 5), + 16) of row t * 32 + (l & 31) at ((t * 4 + s) * 64 + l) * 16 - and |w'|^2 per row (pad rows:
// all zero, HS_WORD_PAD_NORM).
void pack_vocabulary(const uint8_t *words, int k, std::vector<uint8_t> &tiles, std::vector<int32_t> &norms)
{
   const size_t n_tiles = ((size_t)k + HS_WORD_TILE - 1) / HS_WORD_TILE;
   tiles.assign(n_tiles * HS_WORD_TILE_BYTES, 0);
   norms.assign(n_tiles * HS_WORD_TILE, HS_WORD_PAD_NORM);
   for (size_t row = 0; row < (size_t)k; row++) {
      const uint8_t *w = words + row * 128;
      const size_t t = row / HS_WORD_TILE, r = row % HS_WORD_TILE;
      int32_t sq = 0;
      for (int j = 0; j < 128; j++) {
         const int v = (int)w[j] - 128;
         sq += v * v;
         const size_t s = (size_t)j / 32, h = ((size_t)j % 32) / 16, lane = r + 32 * h;
         tiles[((t * 4 + s) * 64 + lane) * 16 + (size_t)j % 16] = (uint8_t)(w[j] ^ 0x80u);
      }
      norms[row] = sq;
   }
}

void need_vocabulary(const hesaff_ctx *c)
{
   if (c->vocab.k == 0) throw HsError(HESAFF_ERR_ARG, "no vocabulary is set (hesaff_set_vocabulary)");
}
} // namespace
extern "C" {

int hesaff_set_vocabulary(hesaff_ctx *c, int k, const uint8_t *words)
{
   if (!c || k < 0 || k > (1 << 20) || (k > 0 && !words)) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   bind_device(c);
   hesaff_ctx::Vocabulary v;
   if (k > 0) {
      std::vector<uint8_t> tiles;
      std::vector<int32_t> norms;
      pack_vocabulary(words, k, tiles, norms);
      v.tiles.ensure(tiles.size());   // (throws HESAFF_ERR_NOMEM with the context's vocabulary untouched)
      v.norms.ensure(norms.size() * 4);
      HIP_TRY(hipMemcpy(v.tiles.p, tiles.data(), tiles.size(), hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(v.norms.p, norms.data(), norms.size() * 4, hipMemcpyHostToDevice));
      v.k = k;
      v.n_tiles = (int)(norms.size() / HS_WORD_TILE);
   }
   HIP_TRY(hipStreamSynchronize(c->stream()));   // nothing still reads the vocabulary that goes
   c->vocab = std::move(v);
   c->cells.clear();   // (hesaff_set_vocabulary_cells: first[C] = K describes the vocabulary that went)
   c->embed.clear();   // (hesaff_set_embedding: tau has the rows of the vocabulary that went)
   c->b_sigs.release();
   if (k == 0) c->b_words.release();
   c->word_spans.clear();
   c->sig_spans.clear();
   c->sigs_device_total = -1;
   c->embed_timed = false;
   c->words_device_total = -1;
   c->assign_timed = false;
   if (k == 0) { c->b_neigh.release(); c->b_nsigs.release(); }
   c->neigh_spans.clear();   // (the neighbour count itself is a setting and stays)
   c->neigh_device_total = -1;
   HS_API_END(c)
}

int hesaff_get_vocabulary_size(const hesaff_ctx *c, int *k)
{
   if (!c || !k) return HESAFF_ERR_ARG;
   *k = c->vocab.k;
   return HESAFF_OK;
}

int hesaff_get_words(const hesaff_ctx *c, int image, const int32_t **words, int *count)
{
   if (!c || !words || !count || c->vocab.k == 0) return HESAFF_ERR_ARG;
   if (image < 0 || (size_t)image >= c->word_spans.size() || c->word_spans[(size_t)image].n < 0) return HESAFF_ERR_ARG;
   *words = c->word_spans[(size_t)image].p;
   *count = c->word_spans[(size_t)image].n;
   return HESAFF_OK;
}

int hesaff_get_words_device(const hesaff_ctx *c, const void **d_words, int64_t *total)
{
   if (!c || !d_words || !total || c->vocab.k == 0 || c->words_device_total < 0) return HESAFF_ERR_ARG;
   *d_words = c->words_device_total > 0 ? c->b_words.p : nullptr;
   *total = c->words_device_total;
   return HESAFF_OK;
}

int hesaff_assign_words_device(hesaff_ctx *c, int64_t n, const void *d_desc, int64_t stride, int64_t offset, void *d_words_out)
{
   if (!c || n < 0 || (n > 0 && (!d_desc || !d_words_out))) return HESAFF_ERR_ARG;
   if (stride < 128 || offset < 0 || offset + 128 > stride || stride % 4 != 0 || offset % 4 != 0) return HESAFF_ERR_ARG;
   if ((uintptr_t)d_desc % 4 != 0 || (uintptr_t)d_words_out % 4 != 0 || n > ((int64_t)1 << 38)) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   need_vocabulary(c);
   bind_device(c);
   launch_assign_words(c, d_desc, (long long)n, (long long)stride, (long long)offset, d_words_out);
   finish_stream(c);
   HS_API_END(c)
}

// ---- vocabulary neighbours (kernels_neighbours.h) ----

int hesaff_set_vocabulary_neighbours(hesaff_ctx *c, int neighbours)
{
   if (!c || neighbours < 1 || neighbours > HS_NEIGH_MAX) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   if (neighbours > 1 && c->cells.c > 0)
      throw HsError(HESAFF_ERR_ARG, "vocabulary neighbours (R > 1) and a cell layer do not combine: remove the layer (hesaff_set_vocabulary_cells with 0 cells) first; the neighbour count is unchanged");
   if (neighbours == c->neighbours) return HESAFF_OK;
   bind_device(c);
   HIP_TRY(hipStreamSynchronize(c->stream()));
   c->neighbours = neighbours;
   // the rows the former count left are not this count's: the getters serve the next call's (R = 1: the words, which stay)
   c->neigh_spans.clear();
   c->neigh_device_total = -1;
   if (neighbours == 1) { c->b_neigh.release(); c->b_nsigs.release(); }
   HS_API_END(c)
}

int hesaff_get_vocabulary_neighbours(const hesaff_ctx *c, int *neighbours)
{
   if (!c || !neighbours) return HESAFF_ERR_ARG;
   *neighbours = c->neighbours;
   return HESAFF_OK;
}

int hesaff_get_neighbours(const hesaff_ctx *c, int image, const int32_t **neighbours, int *count, int *r)
{
   if (!c || !neighbours || !count || !r || c->vocab.k == 0) return HESAFF_ERR_ARG;
   if (c->neighbours == 1) {   // [n][1][2] is the (word, dist2) array itself
      const int rc = hesaff_get_words(c, image, neighbours, count);
      if (rc == HESAFF_OK) *r = 1;
      return rc;
   }
   if (image < 0 || (size_t)image >= c->neigh_spans.size() || c->neigh_spans[(size_t)image].n < 0) return HESAFF_ERR_ARG;
   *neighbours = c->neigh_spans[(size_t)image].p;
   *count = c->neigh_spans[(size_t)image].n;
   *r = c->neigh_spans_r;
   return HESAFF_OK;
}

int hesaff_get_neighbours_device(const hesaff_ctx *c, const void **d_neighbours, int64_t *total, int *r)
{
   if (!c || !d_neighbours || !total || !r || c->vocab.k == 0) return HESAFF_ERR_ARG;
   if (c->neighbours == 1) {
      const int rc = hesaff_get_words_device(c, d_neighbours, total);
      if (rc == HESAFF_OK) *r = 1;
      return rc;
   }
   if (c->neigh_device_total < 0) return HESAFF_ERR_ARG;
   *d_neighbours = c->neigh_device_total > 0 ? c->b_neigh.p : nullptr;
   *total = c->neigh_device_total;
   *r = c->neigh_device_r;
   return HESAFF_OK;
}

int hesaff_assign_neighbours_device(hesaff_ctx *c, int64_t n, const void *d_desc, int64_t stride, int64_t offset, void *d_neighbours_out)
{
   if (!c || n < 0 || (n > 0 && (!d_desc || !d_neighbours_out))) return HESAFF_ERR_ARG;
   if (stride < 128 || offset < 0 || offset + 128 > stride || stride % 4 != 0 || offset % 4 != 0) return HESAFF_ERR_ARG;
   if ((uintptr_t)d_desc % 4 != 0 || (uintptr_t)d_neighbours_out % 4 != 0 || n > ((int64_t)1 << 38)) return HESAFF_ERR_ARG;
   HS_API_BEGIN
   need_vocabulary(c);
   bind_device(c);
   launch_assign_neighbours(c, d_desc, (long long)n, (long long)stride, (long long)offset, d_neighbours_out);
   finish_stream(c);
   HS_API_END(c)
}

int hesaff_get_assign_ms(const hesaff_ctx *c, float *ms)
{
   if (!c || !ms) return HESAFF_ERR_ARG;
   *ms = 0.0f;
   if (!c->assign_timed) return HESAFF_OK;
   if (hipEventSynchronize(c->ev_assign[1]) != hipSuccess || hipEventElapsedTime(ms, c->ev_assign[0], c->ev_assign[1]) != hipSuccess) {
      (void)hipGetLastError();
      *ms = 0.0f;
   }
   return HESAFF_OK;
}

// ---------------------------------- host tables ----------------------------------

int hesaff_table_gauss_mask(int size, float *mask)
{
   if (size < 1 || !(size & 1) || !mask) return HESAFF_ERR_ARG;
   hesaff::gauss_mask(size, mask);
   return HESAFF_OK;
}
int hesaff_table_circ_gauss_mask(int size, float *mask)
{
   if (size < 1 || !(size & 1) || !mask) return HESAFF_ERR_ARG;
   hesaff::circ_gauss_mask(size, mask);
   return HESAFF_OK;
}
int hesaff_table_sift_bins(int32_t *bin0, int32_t *bin1, float *w0, float *w1)
{
   if (!bin0 || !bin1 || !w0 || !w1) return HESAFF_ERR_ARG;
   hesaff::sift_bins(bin0, bin1, w0, w1);
   return HESAFF_OK;
}
int hesaff_table_gauss_kernel(float sigma, int cap, float *taps, int *ksize)
{
   if (!ksize) return HESAFF_ERR_ARG;
   const int K = hesaff::gauss_ksize(sigma);
   *ksize = K;
   if (taps) {
      if (cap < K) return HESAFF_ERR_ARG;
      hesaff::blur_taps(K, sigma, taps);
   }
   return HESAFF_OK;
}

} // extern "C"
