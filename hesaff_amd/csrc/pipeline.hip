// pipeline.hip -- host side of libhesaff_amd.so: context, HBM buffer plan, kernel
// orchestration of one batch, and the C ABI of include/hesaff_amd.h.
//
// The reference chains its stages depth-first through virtual callbacks, one keypoint at
// a time (hesaff.cpp:66-105).  Here a batch of B equally sized images runs breadth-first:
//   pyramid (per octave: R0, 4x blur+response, decimate)  ->  extrema + localise per octave
//   -> order by bitmask rank -> affine iteration -> rectify/bin -> patch -> SIFT -> pack.
// The reference's output order (octave, level, raster of the initial extremum) is
// reproduced by ranking survivors through a bitmask laid out in exactly that order.
//
// Nothing here reads the environment unless the library is built with -DHESAFF_TUNING
// (`make tuning`, a second .so that makes the one schedule observable: HESAFF_OVERLAP=0 runs every
// kernel alone, HESAFF_DEBUG logs the chunks and batches, HESAFF_FAST selects fast mode): a drop-in
// library must not change its schedule, let alone its results, because of an environment variable.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <condition_variable>
#include <deque>
#include <future>
#include <map>
#include <memory>
#include <mutex>
#include <thread>

#include "../../include/hesaff_amd.h"
#include "host_tables.h"
#include "kernels_keypoint.h"
#include "kernels_select.h"
#include "kernels_patch.h"
#include "kernels_sift.h"
#include "kernels_orient.h"
#include "kernels_pyramid.h"
#include "kernels_export.h"
#include "kernels_jpeg.h"
#include "kernels_words.h"
#include "kernels_neighbours.h"
#include "kernels_train.h"
#include "kernels_cells.h"
#include "kernels_index.h"
#include "kernels_verify.h"
#include "kernels_expand.h"
#include "kernels_embed.h"
#include "kernels_index_grow.h"
#include "kernels_index_remove.h"
#include "kernels_index_batch.h"
#include "chunk_engine.h"
#include "batch_plan.h"
#include "buffer_layouts.h"
#include "context_tables.h"
#include "group_schedule.h"
#include "train_plan.h"
#include "cells_plan.h"
#include "index_plan.h"
#include "verify_plan.h"
#include "expand_plan.h"
#include "embed_plan.h"

static thread_local std::string g_create_error;

#define HIP_TRY(expr)                                                                         \
   do {                                                                                       \
      hipError_t e_ = (expr);                                                                 \
      if (e_ != hipSuccess) {                                                                 \
         char buf_[512];                                                                      \
         snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
         throw HsError(HESAFF_ERR_DEVICE, buf_);                                              \
      }                                                                                       \
   } while (0)

using hesaff_engine::HsError;
using hesaff_engine::ArmedMasks;
using namespace hesaff_plan;   // batch_plan.h, context_tables.h: the layouts, the launch arithmetic and the tables of a batch
namespace sched = hesaff_sched;   // group_schedule.h: the stream / event order of the keypoint stages

// Host wait for a HIP event WITHOUT a spinning core.  hipEventSynchronize spins in this runtime even on events created with
// hipEventBlockingSync (measured in round 5 with CLOCK_THREAD_CPUTIME_ID around the call: 96 ms of CPU for a 96 ms wait, one busy core per
// context while a chunk's kernels run - half the CPU quota of an 8-GPU node).  Poll hipEventQuery instead: a few immediate queries for
// waits of microseconds, then sleeps of 20 .. 200 us.
static void hs_wait_event(hipEvent_t ev)
{
   timespec t0;
   clock_gettime(CLOCK_MONOTONIC, &t0);
   for (int tries = 0;; tries++) {
      const hipError_t e = hipEventQuery(ev);
      if (e == hipSuccess) return;
      if (e != hipErrorNotReady) throw HsError(HESAFF_ERR_DEVICE, std::string("hipEventQuery: ") + hipGetErrorString(e));
      (void)hipGetLastError();   // hipErrorNotReady is not an error
      if (tries < 16) continue;
      // sleep an eighth of what has been waited so far, 20 .. 200 us: the wake-up is late by at most ~6 % of a short wait, 0.2 ms of a long one
      timespec now;
      clock_gettime(CLOCK_MONOTONIC, &now);
      const long long waited = (long long)(now.tv_sec - t0.tv_sec) * 1000000000ll + (now.tv_nsec - t0.tv_nsec);
      const timespec nap = {0, (long)std::min<long long>(std::max<long long>(waited / 8, 20000), 200000)};
      nanosleep(&nap, nullptr);
   }
}

static double thread_cpu_ms()   // CPU time of the calling thread (debug lines: does the caller sleep while the device works?)
{
   timespec ts;
   clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts);
   return (double)ts.tv_sec * 1e3 + (double)ts.tv_nsec * 1e-6;
}

// A device buffer that only grows.  ensure() never leaves a dangling pointer behind: the new block
// is allocated before the old one is released (when the device cannot hold both, the old block
// is released first and the allocation retried); on failure the buffer is empty (p == nullptr,
// bytes == 0) and HESAFF_ERR_NOMEM is thrown.  The buffer owns its block: move-only, released with it.
struct DevBuf {
   void *p = nullptr;
   size_t bytes = 0;
   DevBuf() = default;
   DevBuf(const DevBuf &) = delete;
   DevBuf &operator=(const DevBuf &) = delete;
   DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
   DevBuf &operator=(DevBuf &&o) noexcept
   {
      if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
      return *this;
   }
   ~DevBuf() { release(); }
   void ensure(size_t need)
   {
      if (need <= bytes) return;
      void *q = nullptr;
      hipError_t e = hipMalloc(&q, need);
      if (e != hipSuccess && p) {
         (void)hipGetLastError();
         (void)hipFree(p);
         p = nullptr; bytes = 0;
         e = hipMalloc(&q, need);
      }
      if (e != hipSuccess) {
         (void)hipGetLastError();
         if (p) (void)hipFree(p);
         p = nullptr; bytes = 0;
         char buf[256];
         snprintf(buf, sizeof buf, "hipMalloc(%zu bytes) failed: %s", need, hipGetErrorString(e));
         throw HsError(HESAFF_ERR_NOMEM, buf);
      }
      if (p) (void)hipFree(p);
      p = q;
      bytes = need;
   }
   // for buffers whose size follows the data (keypoints of a group, rows of a chunk): a new maximum is allocated with head-room, so
   // that hipFree + hipMalloc - tens of ms for the group buffers, with the device idle - become rare instead of "every denser chunk"
   void ensure_grow(size_t need)
   {
      if (need <= bytes) return;
      try { ensure(need + need / 8); }
      catch (const HsError &) { ensure(need); }
   }
   void release()
   {
      if (p) (void)hipFree(p);
      p = nullptr;
      bytes = 0;
   }
   template <class T> T *as() const { return (T *)p; }
   template <class T> T *at(size_t off) const { return (T *)((char *)p + off); }   // an array of a layout (buffer_layouts.h)
};

// A page-locked host block that only grows, owned like a DevBuf.  The three ways to ask differ in what a block that has to be
// replaced is sized to - pinning costs 0.1 ms per MB and synchronises the device, so that is part of the schedule.
struct PinBuf {
   void *p = nullptr;
   size_t bytes = 0;
   PinBuf() = default;
   PinBuf(const PinBuf &) = delete;
   PinBuf &operator=(const PinBuf &) = delete;
   PinBuf(PinBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
   PinBuf &operator=(PinBuf &&o) noexcept
   {
      if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
      return *this;
   }
   ~PinBuf() { release(); }
   void release() { if (p) (void)hipHostFree(p); p = nullptr; bytes = 0; }
   hipError_t replace(size_t cap)   // the old block goes first; on failure the block is empty
   {
      release();
      const hipError_t e = hipHostMalloc(&p, cap, hipHostMallocDefault);
      if (e != hipSuccess) p = nullptr; else bytes = cap;
      return e;
   }
   // exactly `need` bytes
   void ensure(size_t need)
   {
      if (need <= bytes) return;
      const hipError_t e = replace(need);
      if (e != hipSuccess) throw HsError(HESAFF_ERR_NOMEM, std::string("hipHostMalloc failed: ") + hipGetErrorString(e));
   }
   // a block that is asked for a little more every other chunk (result blocks: the chunks' keypoint counts differ) grows with
   // head-room, so that hipHostFree + hipHostMalloc (hundreds of MB, device-synchronising) stop after the first chunks
   void ensure_grow(size_t need)
   {
      if (need <= bytes) return;
      ensure((need + need / 4 + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1));
   }
   // Small results the host reads every batch (per-image counts, counters, byte offsets of the text rows) arrive in PAGE-LOCKED memory:
   // a hipMemcpyAsync into pageable memory is not asynchronous - the calling thread waits inside the runtime, spinning, until everything
   // before it in the stream has run (a whole batch of kernels: one busy core per context, measured in round 5) - whereas a copy into
   // pinned memory is enqueued and the host sleeps on a blocking-sync event.  Twice the need, 4 KB at least.
   void *ensure_small(size_t need)
   {
      if (need > bytes && replace(std::max<size_t>(need * 2, 4096)) != hipSuccess)
         throw HsError(HESAFF_ERR_NOMEM, "hipHostMalloc failed (small result block)");
      return p;
   }
};

// A HIP event, created with its flags and destroyed with its owner (move-only); passes for the hipEvent_t wherever HIP wants one.
struct DevEvent {
   hipEvent_t e = nullptr;
   DevEvent() = default;
   explicit DevEvent(unsigned flags) { HIP_TRY(hipEventCreateWithFlags(&e, flags)); }
   DevEvent(const DevEvent &) = delete;
   DevEvent &operator=(const DevEvent &) = delete;
   DevEvent(DevEvent &&o) noexcept : e(o.e) { o.e = nullptr; }
   DevEvent &operator=(DevEvent &&o) noexcept
   {
      if (this != &o) { reset(); e = o.e; o.e = nullptr; }
      return *this;
   }
   ~DevEvent() { reset(); }
   void reset() { if (e) (void)hipEventDestroy(e); e = nullptr; }
   operator hipEvent_t() const { return e; }
};

#define HS_AFF_BLOCKS_PER_CU 8   // persistent k_affine blocks per CU (19 KB of LDS each: 8 resident).  Alone on the device 64 / 128 blocks per CU
                                 // are 4 % faster (20.7 / 20.6 vs 21.6 ms), beside the other stages' kernels they make the step 3.5 % slower
                                 // (453 vs 438 ms at B = 128): the queued blocks take every slot that frees up
// grids of the grid-stride list kernels (blocks of 256 threads)
#define HS_GRID_LOC 1024
#define HS_GRID_DED 512
#define HS_GRID_SCAT 1024
#define HS_GRID_PACK 3584   // 14 blocks per CU: what k_pack's 10.7 KB of LDS per block lets a CU hold
#define HS_MID_CAP 6   // blocks per CU of the two row-streamed bins (at most; the occupancy query may say fewer)
#define HS_BIG_CAP 4
#define HS_OVERSUB 128u   // oversubscription of the statically strided persistent grids (step at B = 128: x 1 / 32 / 128 / 256 / 2048: 443 / 438 / 433 / 434 / 447 ms)
// The HIP streams a context runs on (four compute streams, two copy streams).  They are created once per device and handed from a
// destroyed context to the next one (capi_impl.h): which hardware queues a NEW stream shares depends on everything the process has
// created before, so only reuse keeps the queue pairing of the first context.  Contexts alive at the same time get sets of their own.
//
// The HIP runtime runs the streams of one priority on FOUR hardware queues, and kernels of streams that share a queue do not
// overlap.  Which of a context's seven logical streams (main, patch bins 0-3, descriptor, affine) end up together moves the step
// by up to 8 %, and with seven HIP streams it depends on what else the process has created.  So the pairing is made explicit:
// four HIP streams, each serving the logical streams that measured best together
// (profiles/r04_notes.md):   main + bin 3 | bin 0 + bin 1 | bin 2 + affine | descriptor.
struct StreamSet {
   hipStream_t comp[4] = {nullptr, nullptr, nullptr, nullptr};
   hipStream_t h2d = nullptr, d2h = nullptr;   // made when the first chunk needs them (ensure_copy_streams, capi_impl.h)
   static constexpr int group[7] = {0, 1, 1, 2, 0, 3, 2};   // logical stream -> HIP stream: 0 main, 1-4 patch bins 0-3, 5 descriptor, 6 affine
   hipStream_t of(int logical) const { return comp[group[logical]]; }   // (the numbers are sched::Stream's, group_schedule.h)
   hipStream_t main() const { return of(0); }
   hipStream_t bin(int i) const { return of(1 + i); }   // side stream of the patch stage's window-size bin i (0..3)
   hipStream_t sift() const { return of(5); }           // descriptor kernels of every image group
   hipStream_t affine() const { return of(6); }         // affine shape of image group g+1 runs beside the patch extraction of group g
};
static std::mutex g_sets_mu;
static std::map<int, std::vector<StreamSet>> g_idle_sets;   // per device: the sets no context is using
static bool take_stream_set(int device, StreamSet &out)
{
   std::lock_guard<std::mutex> lk(g_sets_mu);
   std::vector<StreamSet> &v = g_idle_sets[device];
   if (v.empty()) return false;
   out = v.back();
   v.pop_back();
   return true;
}
static void give_stream_set(int device, const StreamSet &s)
{
   std::lock_guard<std::mutex> lk(g_sets_mu);
   g_idle_sets[device].push_back(s);
}

// The tables of a context on the device (context_tables.h makes them), and the view of them the kernels take.  Either method
// leaves the view current.
struct DeviceTables {
   DevBuf smm, sift_mask, bin0, bin1, w0, w1, mask_idx, sgrad_nb, sgrad_om, vo_rows, vo_src, pyr_taps, patch_taps, patch_off, patch_k;
   KpTables view = {};   // (view.max_p0: the patch tap table covers odd P0 <= max_p0)
   template <class T> static const T *put(DevBuf &b, const std::vector<T> &v)
   {
      b.ensure(std::max<size_t>(v.size() * sizeof(T), 16));
      HIP_TRY(hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
      return b.as<T>();
   }
   void upload(const ContextTables &t)
   {
      view.smm_mask = put(smm, t.smm); view.sift_mask = put(sift_mask, t.sift_mask);
      view.mask_idx = put(mask_idx, t.mask_idx); view.n_masked = t.n_masked;
      view.sgrad_nb = (const int4 *)put(sgrad_nb, t.sgrad_nb); view.sgrad_om = (const int2 *)put(sgrad_om, t.sgrad_om);
      view.vo_rows = (const int4 *)put(vo_rows, t.vo_rows); view.vo_src = put(vo_src, t.vo_src);
      view.bin0 = put(bin0, t.bin0); view.bin1 = put(bin1, t.bin1); view.w0 = put(w0, t.w0); view.w1 = put(w1, t.w1);
      put(pyr_taps, t.pyr_taps);
   }
   void grow_patch_taps(int max_p0)
   {
      if (max_p0 <= view.max_p0) return;
      const PatchTaps t = build_patch_taps(max_p0);
      view.patch_taps = put(patch_taps, t.taps); view.patch_tap_off = put(patch_off, t.off); view.patch_tap_k = put(patch_k, t.k);
      view.max_p0 = t.max_p0;
   }
};

struct hesaff_ctx {
   hesaff_params par;
   int device = 0;
   StreamSet sset;   // every HIP stream of the context
   hipStream_t stream() const { return sset.main(); }
   std::string err;
   ContextScalars ct;     // the schedule, DConsts and the pyramid blurs' tap counts (build_context_tables)
   DeviceTables tables;
   int batch_max_p = 0;   // largest window side P of the current batch's huge windows (known after detection)

   // geometry of the current buffer plan (H x W: the images; the pyramid starts at (H << ct.up) x (W << ct.up))
   int B = 0, H = 0, W = 0;
   std::vector<OctGeom> oct;
   long long words_per_image = 0;
   uint32_t cap = 0;      // keypoint capacity of a batch
   uint32_t cand_cap = 0; // candidate slots of one octave (k_extrema_march -> k_localize)
   OrderMapEpochs map_epochs;   // of b_map (batch_plan.h)

   // the buffers whose size follows the plan's geometry (B x H x W and the keypoint capacity): a plan the device cannot hold gives
   // all of them back at once (plan())
   struct GeomBufs {
      DevBuf b_gray, b_up, b_L, b_L3, b_R, b_map, b_bitmask, b_prefix, b_blocksums;   // planes
      DevBuf b_cand, b_rec_f, b_rec_i, b_rec_w, b_hess_f, b_hess_i, b_aff, b_pw, b_bins, b_rank, b_desc, b_out, b_starts;   // lists
   } geo;
   DevBuf b_generic;
   std::vector<DPlane> L;   // [octave*3 + level]
   DPlane gray, upimg, L3, R[5];
   // lists
   DevBuf b_counters;       // one CounterBlock (batch_plan.h)
   DevBuf b_patches, b_stage;
   DevBuf b_input;          // staging for host images (stage API)
   // The host entry points: chunks of max_batch images are pipelined -- pinned staging + H2D of chunk k+1 and D2H of chunk k-1 run
   // beside the kernels of chunk k (chunk_engine.h: run_chunk_loop).  Chunk k has slot k & 1: what it is copied into, computed from and
   // copied out of on the device, and the events between those steps (made by ensure_copy_streams, capi_impl.h).
   struct ChunkSlot {
      PinBuf pin_in;        // the chunk's pixels (or JPEG coefficient blobs) on their way in, unless the readers filled pinned memory ...
      DevBuf b_in2;         // ... and on the device: the input of run_batch
      DevBuf b_jcoef;       // JPEG chunks: the images' coefficient blobs (kernels_jpeg.h makes the pixels in b_in2)
      PinBuf pin_reg;       // hesaff_describe_regions: the chunk's record starts + records ...
      DevBuf b_reg;         // ... and on the device (run_describe's d_block)
      PinBuf pin_mask;      // hesaff_set_next_masks: the chunk's "present" bytes + mask planes (batch_plan.h: mask_planes_offset) ...
      DevBuf b_mask;        // ... and on the device (run_batch's SelMasks); neither exists before a mask was armed
      DevBuf b_outstage;    // what leaves for the host, in the layout of the result block
      DevEvent ev_h2d;      // the copy in has landed
      DevEvent ev_h2d_blk;  // blocking-sync: the staging thread sleeps until a chunk's direct copies have left the readers' buffers
      DevEvent ev_in_free;  // the kernels have read the input: the slot may be refilled
      DevEvent ev_out_ready, ev_d2h;   // b_outstage is complete; the copy out has left it
      DevEvent ev_exp[4];   // profiling: brackets of the chunk's length pass and of its write pass (the host's waits between them - a free pinned block - are not the export's)
   } slot[2];
   // Page-locked buffers the readers of hesaff_process_files fill directly (chunk_engine.h: PinHooks): handed out by size, taken back
   // when their image is on the device, kept pinned from one list to the next (pinning costs 0.1 ms per MB), released with the context.
   // At most kPinReadBytes are out or parked; a request beyond that gets nullptr (the image then takes the staging copy).
   struct PinReadCache {
      static constexpr size_t kLargest = (size_t)64 << 20;
      size_t max_bytes = (size_t)4 << 30;    // out + parked never exceed this (hesaff_set_pinned_read_budget)
      size_t keep_bytes = (size_t)1 << 30;   // parked buffers kept from one hesaff_process_files call to the next
      std::mutex mu;
      std::vector<std::pair<void *, size_t>> parked;
      size_t bytes_total = 0;   // out + parked
      int device = 0;
      // (hipHostFree / hipHostMalloc are device-synchronising and slow: never under `mu`, which FileIO reaches with its own lock held)
      void *take(size_t bytes)
      {
         if (bytes == 0 || bytes > kLargest) return nullptr;
         std::vector<std::pair<void *, size_t>> evicted;
         bool room = false;
         {
            std::lock_guard<std::mutex> lk(mu);
            for (size_t k = 0; k < parked.size(); k++)
               if (parked[k].second == bytes) { void *q = parked[k].first; parked[k] = parked.back(); parked.pop_back(); return q; }
            // no room: parked buffers of other sizes (an earlier list's images) make way
            while (bytes_total + bytes > max_bytes && !parked.empty()) {
               evicted.push_back(parked.back());
               bytes_total -= parked.back().second;
               parked.pop_back();
            }
            room = bytes_total + bytes <= max_bytes;
            if (room) bytes_total += bytes;
         }
         for (auto &b : evicted) (void)hipHostFree(b.first);
         if (!room) return nullptr;
         void *q = nullptr;
         if (hipSetDevice(device) != hipSuccess || hipHostMalloc(&q, bytes, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            std::lock_guard<std::mutex> lk(mu);
            bytes_total -= bytes;
            return nullptr;
         }
         return q;
      }
      void give(void *q, size_t bytes)
      {
         std::lock_guard<std::mutex> lk(mu);
         parked.emplace_back(q, bytes);
      }
      // the end of a hesaff_process_files call: what is parked beyond `keep` goes back to the system
      void trim(size_t keep)
      {
         std::vector<std::pair<void *, size_t>> out;
         {
            std::lock_guard<std::mutex> lk(mu);
            size_t held = 0;
            for (auto &b : parked) held += b.second;
            while (held > keep && !parked.empty()) {
               out.push_back(parked.back());
               held -= parked.back().second; bytes_total -= parked.back().second;
               parked.pop_back();
            }
         }
         for (auto &b : out) (void)hipHostFree(b.first);
      }
      ~PinReadCache() { trim(0); }
   } pin_read;
   std::vector<PinBuf> pin_out;       // result blocks: one per chunk of the current call (hesaff_detect_batch), or a ring of three
   hesaff_engine::BlockRing ring;     // (hesaff_detect_batch_cb, hesaff_process_files: a block returns to the ring when its consumer is done with it)
   float export_ms = 0.0f; int32_t export_rows = 0;
   PinBuf h_small_end, h_small_mid, h_small_exp;   // small results the host reads every batch (PinBuf::ensure_small)
   DevBuf b_rowprefix, b_trows, b_trows2, b_trows3;
   DevBuf b_jplane;   // JPEG chunks: the component planes after the inverse DCT (kernels_jpeg.h)
   DevBuf b_ex_len, b_ex_sums, b_ex_off, b_ex_imgoff, b_ex_starts;   // device export (kernels_export.h): row lengths, sums / offsets per 64 rows, offsets per image
   size_t rows_lds_set = 0;            // dynamic LDS opt-in of k_patch_large_rows on THIS device
   // persistent grids of the LDS-window kernels: exactly as many blocks as the device holds at once (CUs x resident
   // blocks per CU), so that every block takes the same share of a bin's list; queried per device at hesaff_create
   int n_cu = 256;
   uint32_t g_small0 = 256 * 6, g_small1 = 256 * 4, g_mid = HS_MID_BLOCKS, g_big = HS_BIG_BLOCKS, g_lfin = 256 * 4, g_shist = 256 * 32;
   uint32_t sgrad_grid = 256 * 32;     // persistent grid of k_sift_grad: 32 blocks per CU (set_kernel_attrs)
   uint32_t trows_rows = 4u << 20;     // rows of T' (82 floats each) the large-window buffer holds at least: 1.3 GB

   hesaff_timings tm;
   int profiling = 0;
   int out_format = HESAFF_OUT_TEXT;   // hesaff_set_output_format
   int resume = 0;                     // hesaff_set_resume: 0 off, 1 skip complete outputs (O(1) test), 2 strict (rows counted)
   int pool_priority = -1;             // hesaff_set_pool_priority: -1 lower the pool's priority when the plan is CPU-starved, 0 never, 1 always
   int keypoint_limit = 0;             // hesaff_set_keypoint_limit: 0 no limit, N >= 1 the N strongest Hessian keypoints of every image (run_batch)
   int grid_rows = 1, grid_cols = 1;   // hesaff_set_keypoint_grid: with a limit N and more than one cell, the N / cells strongest of every cell
   int descriptor = HESAFF_DESC_SIFT;  // hesaff_set_descriptor: which instantiation of k_sift_hist the pipeline's launch_sift takes
   int orientation = HESAFF_ORI_UP;    // hesaff_set_orientation: HESAFF_ORI_DOMINANT runs the oriented order of group_schedule.h (run_keypoint_stages)
   int orientation_count = 1;          // hesaff_set_orientation_count: keys per region at most (read in HESAFF_ORI_DOMINANT only: ori_count)
   DevBuf b_ori_ranks;                 // the rank arrays of an orientation count K > 1 (OrientRanks, device_lists.h): allocated by the first such call
   // hesaff_set_vocabulary: the vocabulary as k_assign_words reads it (kernels_words.h: XORed, padded to whole tiles, in lane order,
   // with |w'|^2 per row); k = 0: none, and nothing below is allocated, launched or copied
   struct Vocabulary { DevBuf tiles, norms; int k = 0, n_tiles = 0; } vocab;
   DevBuf b_words;                     // (word, dist2) per record of b_out, written behind the pack stage of every batch
   int64_t words_device_total = -1;    // hesaff_get_words_device: the rows of b_words after a device-resident call (-1: no such call was the last)
   std::vector<hesaff_engine::WordSpan> word_spans;   // hesaff_get_words: per image of the last host call, its rows in the call's result blocks
   // hesaff_set_vocabulary_neighbours: R = 1 (the default) is the plain assignment, and nothing of the four below is allocated,
   // launched or copied; R > 1: k_assign_neighbours (kernels_neighbours.h) takes k_assign_words' place and leaves int32[rows][R][2]
   // in b_neigh beside the (word, dist2) array, which is its rank 0
   int neighbours = 1;
   DevBuf b_neigh;
   DevBuf b_nsigs;                     // hesaff_process_files with an embedding and R > 1: the signatures of the ranks 1 .. R - 1 of a chunk, a plane per rank
   int64_t neigh_device_total = -1;    // hesaff_get_neighbours_device: the rows of b_neigh the last assignment left (-1: none, or a host call since)
   int neigh_device_r = 1;             // ... and the R they were written with
   std::vector<hesaff_engine::NeighSpan> neigh_spans;   // hesaff_get_neighbours: per image of the last host call (R > 1), as word_spans
   int neigh_spans_r = 1;
   DevEvent ev_assign[2];              // profiling: brackets of the last k_assign_words (R > 1: k_assign_neighbours) launch
   bool assign_timed = false;          // ev_assign holds a launch of the last batch
   float train_ms[3] = {0.0f, 0.0f, 0.0f};   // hesaff_get_training_ms: assignment, accumulation, update of the last training call (profiling >= 1)
   // hesaff_set_vocabulary_cells: a cell layer over the vocabulary (cells_plan.h: CellLayerArrays in `layer`, CellScratch for `cap` keys
   // in `scratch`, which is allocated by the first assignment through the layer and only grows); c = 0: none, nothing here is
   // allocated, launched or copied and the assignment is k_assign_words over the whole vocabulary
   struct Cells {
      DevBuf layer, scratch;
      CellLayerArrays a;
      int c = 0;
      int64_t cap = 0;                 // keys the scratch is laid out for
      std::vector<DevEvent> ev;        // profiling: four per slice of the last assignment (start, coarse, grouped, fine)
      int timed_slices = 0;            // slices of the last assignment that ev brackets
      int probes = 1;                  // hesaff_set_vocabulary_probes: a context setting, kept by clear(); read with a layer set only
      void clear() { layer.release(); scratch.release(); c = 0; cap = 0; timed_slices = 0; }
   } cells;
   // hesaff_index_build: the inverted file over visual words (index_plan.h: IndexArrays in `tables`, the posting lists in `lists`);
   // not built: nothing here is allocated, launched or copied
   struct Index {
      DevBuf tables, lists, qwords;    // qwords: the staged words of a host query
      IndexArrays a;
      // hesaff_index_build_embedded: word-major key lists of (image, signature) beside the postings (embed_plan.h: KeyListArrays in
      // `keys`); a plain build leaves them empty
      DevBuf keys, qsigs;              // qsigs: the staged signatures of a host query
      KeyListArrays ka;
      bool embedded = false;
      template <class T> T *kptr(const Span<T> &s) const { return keys.at<T>(s.off); }
      int n_images = 0, k = 0;
      int64_t n_keys = 0, n_postings = 0;
      bool built = false;
      template <class T> T *ptr(const Span<T> &s) const { return tables.at<T>(s.off); }
      // hesaff_index_query_batch*: the scratch of a chunk (index_batch_plan.h: IndexBatchArrays), the chunks' query starts, the staged
      // words and signatures of a host batch, and the pinned block a chunk's ranked rows arrive in.  They grow to what the batches so
      // far needed and go with the index; no batch call: nothing here is allocated, launched or copied
      DevBuf batch_scratch, batch_starts, batch_words, batch_sigs;
      PinBuf batch_ranked;
      void release_batch() { batch_scratch.release(); batch_starts.release(); batch_words.release(); batch_sigs.release(); batch_ranked.release(); }
   } index;
   size_t index_batch_budget = 0;      // hesaff_index_set_batch_budget: a context setting, kept by clear, build and load (0: the plan's default)
   float index_batch_ms[3] = {0.0f, 0.0f, 0.0f};   // hesaff_get_index_batch_ms: grouping, scoring, finish and selection, summed over the last batch's chunks
   int index_batch_chunks = 0;         // hesaff_index_get_batch_chunks: the chunks of the last batch
   // hesaff_set_embedding: the projection as k_embed_keys reads it and the thresholds of every word (embed_plan.h: EmbedArrays in `buf`);
   // not set: nothing here is allocated, launched or copied, and the assignment stops at the words
   struct Embedding {
      DevBuf buf;
      EmbedArrays a;
      int k = 0;                       // the rows of tau: the vocabulary's
      bool set = false;
      std::vector<int8_t> P;           // hesaff_get_embedding: P as the caller gave it
      template <class T> T *ptr(const Span<T> &s) const { return buf.at<T>(s.off); }
      void clear() { buf.release(); k = 0; set = false; P.clear(); P.shrink_to_fit(); }
   } embed;
   DevBuf b_sigs;                      // a signature per record of b_out, written behind b_words of every batch
   int64_t sigs_device_total = -1;     // hesaff_get_signatures_device: the rows of b_sigs after a device-resident call (-1: as words_device_total)
   std::vector<hesaff_engine::SigSpan> sig_spans;   // hesaff_get_signatures: per image of the last host call, its rows in the call's result blocks
   DevEvent ev_embed[2];               // profiling: brackets of the last k_embed_keys launch
   bool embed_timed = false;
   float embed_train_ms[3] = {0.0f, 0.0f, 0.0f};   // hesaff_get_embedding_ms: projection, grouping, medians of the last threshold training
   float index_ms[3] = {0.0f, 0.0f, 0.0f};   // hesaff_get_index_ms: the last build's hash step and list steps, the last query (profiling >= 1)
   float index_growth_ms[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};   // hesaff_get_index_growth_ms: the last add's insert, tables, merge, scatter; the last load's device pass
   float index_remove_ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};   // hesaff_get_index_remove_ms: the last removal's counting pass, tables, compaction, key lists
   // hesaff_verify_matches: the result of the last call (verify_plan.h: VerifyResultArrays in `result`); no call: nothing here is
   // allocated, launched or copied
   struct Verify {
      DevBuf result;
      VerifyResultArrays a;
      int n_candidates = 0;
      uint32_t query_inert = 0;
      bool done = false;
      std::vector<uint32_t> used;      // M_r of the last call: hesaff_verify_get_pairs' counts
      std::vector<int32_t> h_pairs;    // hesaff_verify_get_pairs: the pairs of the candidate asked for last
      template <class T> T *ptr(const Span<T> &s) const { return result.at<T>(s.off); }
   } verify;
   float verify_ms[2] = {0.0f, 0.0f};        // hesaff_get_verify_ms: the pair steps and the hypothesis steps of the last call (profiling >= 1)
   float expand_ms[2] = {0.0f, 0.0f};        // hesaff_get_expand_ms: the flags pass with its scan, and the scatter, of the last call (profiling >= 1)
   ArmedMasks next_masks;              // hesaff_set_next_masks / _device: the masks of the next detecting call (taken, so cleared, by take_masks)
   int stage_threads = 4;              // host threads that copy a chunk's pixels into pinned memory (hesaff_process_files: within its thread budget)
   DevEvent ev_detect_done, ev_batch_done;   // blocking-sync events: the host sleeps instead of spinning
   std::vector<DevEvent> ev_aff;             // one per image group, grown on demand (GroupDevice)
   DevEvent ev_extract_done[HS_NSLOT], ev_sift_done[HS_NSLOT];
   DevBuf b_patches2[HS_NSLOT];
   DevBuf b_meanvar2, b_siftvo2;   // the descriptor stage's intermediates: one copy (ensure_group_buffers)
   DevEvent ev_fork, ev_join[HS_NSIDE];
   bool fast_pyramid = false;      // hesaff_params.fast == 2: windows beyond bin 0 sampled from the scale-space level with the matching blur (not bit-exact)
   // off in the product build; the tuning build (-DHESAFF_TUNING) reads them from the environment, and HESAFF_FAST for fast_pyramid
   bool no_overlap = false;        // HESAFF_OVERLAP=0: every kernel alone on the device (per-kernel profiling)
   bool debug = false;             // HESAFF_DEBUG=1: launch geometry on stderr
   bool sift_inside = false;       // HESAFF_SIFT_INSIDE=1: a group's descriptor kernels submitted inside the next group's patch stage (group_schedule.h)

   std::vector<DevEvent> ev_pool;   // timing events of the stage timers (get_event)
   size_t ev_used = 0;
};

namespace {

struct EvPair { hipEvent_t a, b; int kind; double bytes; };

hipEvent_t get_event(hesaff_ctx *c)
{
   if (c->ev_used == c->ev_pool.size()) c->ev_pool.emplace_back(hipEventDefault);
   return c->ev_pool[c->ev_used++];
}

DPlane make_plane(float *p, int rows, int cols, int pitch)
{
   DPlane d;
   d.p = p; d.rows = rows; d.cols = cols; d.pitch = pitch; d.img_stride = (long long)rows * pitch;
   return d;
}

template <class KERNEL> void set_dyn_lds(KERNEL kern, size_t lds)
{
   HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
}

size_t small_extract_lds_bytes(int bin) { return (size_t)(bin == 0 ? SmallGeom<0>::FLOATS : SmallGeom<1>::FLOATS) * 4; }
size_t mid_lds_bytes() { return (size_t)MidGeom<HS_MID_PMAX>::FLOATS * 4; }
size_t big_lds_bytes() { return (size_t)MidGeom<HS_BIN3_PMAX>::FLOATS * 4; }

// Dynamic-LDS opt-ins are per device: applied when a context is created on its device (hesaff_create) and, for the
// large-window kernel whose need depends on the image size, in plan().
template <class KERNEL> uint32_t resident_grid(hesaff_ctx *c, KERNEL kern, int threads, size_t dyn_lds, uint32_t fallback_per_cu)
{
   int nb = 0;
   if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)kern, threads, dyn_lds) != hipSuccess || nb < 1) {
      (void)hipGetLastError();
      nb = (int)fallback_per_cu;
   }
   return (uint32_t)c->n_cu * (uint32_t)nb;
}

void set_kernel_attrs(hesaff_ctx *c)
{
   set_dyn_lds(k_patch_extract_small<0>, small_extract_lds_bytes(0));
   set_dyn_lds(k_patch_extract_small<1>, small_extract_lds_bytes(1));
   set_dyn_lds(k_patch_mid<HS_MID_PMAX>, mid_lds_bytes());
   set_dyn_lds(k_patch_mid<HS_BIN3_PMAX>, big_lds_bytes());
   hipDeviceProp_t prop;
   HIP_TRY(hipGetDeviceProperties(&prop, c->device));
   c->n_cu = std::max(1, prop.multiProcessorCount);
   c->g_small0 = resident_grid(c, k_patch_extract_small<0>, 256, small_extract_lds_bytes(0), 6);
   c->g_small1 = resident_grid(c, k_patch_extract_small<1>, 256, small_extract_lds_bytes(1), 4);
   // the row-streamed bins claim their items dynamically: any grid that fills the device works; one T' slot per block
   c->g_mid = std::min<uint32_t>(resident_grid(c, k_patch_mid<HS_MID_PMAX>, 256, mid_lds_bytes(), HS_MID_CAP), HS_MID_BLOCKS);
   c->g_big = std::min<uint32_t>(resident_grid(c, k_patch_mid<HS_BIN3_PMAX>, 256, big_lds_bytes(), HS_BIG_CAP), HS_BIG_BLOCKS);
   c->g_lfin = resident_grid(c, k_patch_large_finish, 256, 0, 4);
   c->g_shist = resident_grid(c, k_sift_hist<HESAFF_DESC_SIFT>, 64, 0, 32);   // (the RootSIFT instantiation strides over the same grid)
   // k_sift_grad: a block keeps its per-pixel tables and requests the next patch while it works on the current one; well
   // over the resident count so that the tail of a launch is short (measured: one block per keypoint 18.5 ms per 32 UHD
   // images, 6 / 16 / 32 / 64 blocks per CU 15.2 / 13.8 / 13.3 / 13.4)
   c->sgrad_grid = (uint32_t)c->n_cu * 32u;
   // The statically strided grids are launched HS_OVERSUB x oversubscribed: an item's cost varies several-fold, blocks beyond the
   // resident count start as others finish, and the hardware's block scheduler evens out what a fixed stride cannot
   // (a claim per item on an atomic counter serialises in L2 instead).  Measured per 32 UHD images, x 1 / 8 / 32:
   // k_patch_extract_small<0> 13.8 / 13.3 / 12.9 ms, <1> 6.1 / - / 5.9, k_sift_hist 13.4 / 12.0 / 11.7.
   c->g_small0 *= HS_OVERSUB; c->g_small1 *= HS_OVERSUB; c->g_shist *= HS_OVERSUB;
}

// Buffer plan for a batch of B images of H x W.
void plan_buffers(hesaff_ctx *c, int B, int H, int W);
void plan(hesaff_ctx *c, int B, int H, int W)
{
   try {
      plan_buffers(c, B, H, W);
   } catch (const HsError &e) {
      if (e.code == HESAFF_ERR_NOMEM) {
         // a plan the device cannot hold must not keep what it managed to allocate on the way (hundreds of GB for an absurd
         // capacity request): every geometry-sized buffer goes back, the next plan starts from nothing
         (void)hipStreamSynchronize(c->stream());
         c->geo = hesaff_ctx::GeomBufs();
         c->map_epochs.invalidate();
      }
      throw;
   }
}

void plan_buffers(hesaff_ctx *c, int B, int H, int W)
{
   if (B <= c->B && H == c->H && W == c->W) return;
   if (H < 1 || W < 1 || (H << c->ct.up) > 65535 || (W << c->ct.up) > 65535) throw HsError(HESAFF_ERR_ARG, "image size out of range (1..65535 at the first pyramid level)");
   const int PH = H << c->ct.up, PW = W << c->ct.up;   // first pyramid level
   // the cached geometry describes buffers that are about to be replaced: a failure below must not leave it valid
   c->B = c->H = c->W = 0;
   c->L.clear();
   {
      PyramidGeom pg = pyramid_geometry(H, W, c->ct.up);
      c->oct = std::move(pg.oct);
      c->words_per_image = pg.words_per_image;
   }
   const long long words = c->words_per_image;
   size_t L_floats = 0;
   for (const OctGeom &g : c->oct) L_floats += (size_t)3 * B * g.rows * g.pitch;
   const int pitch0 = round_up(W, 64);
   const size_t plane0 = (size_t)B * H * pitch0;
   c->geo.b_gray.ensure(plane0 * 4);
   c->gray = make_plane(c->geo.b_gray.as<float>(), H, W, pitch0);
   c->geo.b_L.ensure(std::max<size_t>(L_floats * 4, 16));
   {
      float *p = c->geo.b_L.as<float>();
      for (const OctGeom &g : c->oct)
         for (int l = 0; l < 3; l++) {
            c->L.push_back(make_plane(p, g.rows, g.cols, g.pitch));
            p += (size_t)B * g.rows * g.pitch;
         }
   }
   const int ppitch0 = round_up(PW, 64);
   const size_t pplane0 = (size_t)B * PH * ppitch0;
   if (c->ct.up) {
      c->geo.b_up.ensure(pplane0 * 4);
      c->upimg = make_plane(c->geo.b_up.as<float>(), PH, PW, ppitch0);
   }
   c->geo.b_L3.ensure(pplane0 * 4);
   c->geo.b_R.ensure(pplane0 * 4 * 5);
   {
      const void *before = c->geo.b_map.p;
      const size_t before_bytes = c->geo.b_map.bytes;
      c->geo.b_map.ensure(std::max<size_t>((size_t)B * PH * PW * 4, 16));
      // a new block is filled once before its first use (run_detection).  Pointer AND size: ensure()'s out-of-memory path frees the old
      // block first, and the larger one may come back at the same address with a tail that was never filled
      if (c->geo.b_map.p != before || c->geo.b_map.bytes != before_bytes) c->map_epochs.invalidate();
      c->map_epochs.set_key_bits(order_key_bits(PH, PW));
   }
   const long long total_words = (long long)B * words;
   c->geo.b_bitmask.ensure(std::max<size_t>((size_t)total_words * 8, 16));
   c->geo.b_prefix.ensure(std::max<size_t>((size_t)(total_words + 1) * 4, 16));
   c->cap = keypoint_capacity(B, PH, PW, (double)c->par.max_kpts_per_mpx);
   const size_t cap = c->cap;
   const long long scan_items = std::max<long long>(total_words, (long long)cap);
   c->geo.b_blocksums.ensure((size_t)((scan_items + SCAN_BLOCK - 1) / SCAN_BLOCK + 1) * 4);
   c->b_counters.ensure(sizeof(CounterBlock));
   c->cand_cap = candidate_capacity(c->cap, B, PH, PW);
   c->geo.b_cand.ensure((size_t)c->cand_cap * sizeof(CandRec));
   // the lists: sized here, cut into their arrays by make_lists - both from the layouts of buffer_layouts.h
   const RecLayout rec = rec_layout(cap);
   c->geo.b_rec_f.ensure(rec.f_bytes);
   c->geo.b_rec_i.ensure(rec.i_bytes);
   c->geo.b_rec_w.ensure(rec.w_bytes);
   const HessLayout hess = hess_layout(cap);
   c->geo.b_hess_f.ensure(hess.f_bytes);
   c->geo.b_hess_i.ensure(hess.i_bytes);
   c->geo.b_aff.ensure(affine_layout(cap).bytes);
   const PatchLayout patch = patch_layout(cap);
   c->geo.b_pw.ensure(patch.pw_bytes);
   c->geo.b_bins.ensure(patch.bins_bytes);
   c->geo.b_rank.ensure((cap + 1) * 4);
   c->geo.b_desc.ensure(cap * 128);
   c->geo.b_out.ensure(cap * sizeof(KeyRec));
   c->geo.b_starts.ensure(starts_block((int32_t *)nullptr, B).words_allocated() * 4);   // StartsBlock, batch_plan.h
   // patch taps: P <= sqrt(W*H) + small (the det-1 window must fit)
   const int max_p0 = (int)std::floor(std::sqrt((double)W * (double)H)) + 3;
   c->tables.grow_patch_taps(max_p0);
   // per-block T' slots of the row-streamed bins (persistent grids of fixed size)
   c->b_trows2.ensure((size_t)HS_MID_BLOCKS * (HS_MID_PMAX + 2 * HS_MID_RPAD) * HS_NEED * 4);
   c->b_trows3.ensure((size_t)HS_BIG_BLOCKS * (HS_BIN3_PMAX + 2 * HS_BIG_RPAD) * HS_NEED * 4);
   const size_t want = large_rows_lds_optin(c->tables.view.max_p0);   // (refuses an image whose largest window row does not fit the LDS)
   if (want > c->rows_lds_set) {
      set_dyn_lds(k_patch_large_rows, want);
      c->rows_lds_set = want;
   }
   c->B = B; c->H = H; c->W = W;
}

template <class LOAD> void exclusive_scan(hesaff_ctx *c, LOAD load, long long n, uint32_t *out, uint32_t *total, uint32_t *block_sums = nullptr)
{
   // out[0..n) exclusive prefix, *total = sum (device pointers); block_sums: one word per SCAN_BLOCK items (default: the plan's)
   if (n <= 0) { HIP_TRY(hipMemsetAsync(total, 0, 4, c->stream())); return; }
   const int nb = (int)((n + SCAN_BLOCK - 1) / SCAN_BLOCK);
   uint32_t *bs = block_sums ? block_sums : c->geo.b_blocksums.as<uint32_t>();
   hipLaunchKernelGGL(k_scan_reduce<LOAD>, dim3(nb), dim3(256), 0, c->stream(), load, n, bs);
   hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(256), 0, c->stream(), bs, nb, total);
   hipLaunchKernelGGL(k_scan_down<LOAD>, dim3(nb), dim3(256), 0, c->stream(), load, n, bs, out);
}

// Stage timers: one HIP event pair per bracket, recorded on the stream the bracketed work is launched on.
struct StageTimer {
   hesaff_ctx *c;
   std::vector<EvPair> pairs;
   std::vector<hipStream_t> streams;
   explicit StageTimer(hesaff_ctx *ctx) : c(ctx) {}
   int begin(int kind, double bytes = 0, hipStream_t st = nullptr)
   {
      if (!c->profiling) return -1;
      if (kind >= 100 && c->profiling < 2) return -1;
      if (!st) st = c->stream();
      EvPair p; p.a = get_event(c); p.b = get_event(c); p.kind = kind; p.bytes = bytes;
      (void)hipEventRecord(p.a, st);
      pairs.push_back(p);
      streams.push_back(st);
      return (int)pairs.size() - 1;
   }
   void end(int id) { if (id >= 0) (void)hipEventRecord(pairs[id].b, streams[id]); }
};

enum { T_PYR = 0, T_DET = 1, T_AFF = 2, T_PATCH = 3, T_SIFT = 4, T_TOTAL = 5, T_PACK = 6, T_BLURHESS = 100, T_EXTREMA = 101 };

// Band height of k_blur_hess_march: march_bands (batch_plan.h).
template <int K, bool WL, bool WR, bool WH, bool WR0 = false, int SRC = SRC_PLANE>
void launch_march(hesaff_ctx *c, const DPlane &in, const DPlane &outL, const DPlane &outR, const DPlane &outHalf, const float *taps,
                  float norm2, int B, const DPlane &outR0 = DPlane(), float norm2_in = 0.0f, const GraySrc &gs = GraySrc(), const DPlane &outGray = DPlane())
{
   const MarchBands mb = march_bands(in.rows, in.cols, B);
   const int band = mb.band;
   if (c->debug) fprintf(stderr, "[hesaff] march K=%d %dx%d B=%d bands=%d band=%d blocks=%lld\n", K, in.cols, in.rows, B, mb.bands, band, (long long)mb.strip_blocks * B * mb.bands);
   const dim3 grid(mb.strip_blocks, (in.rows + band - 1) / band, B);
   hipLaunchKernelGGL((k_blur_hess_march<K, WL, WR, WH, WR0, SRC>), grid, dim3(256), 0, c->stream(), in, outL, outR, outHalf, taps, norm2, band, outR0, norm2_in, gs, outGray);
}

template <bool WL, bool WR, bool WH>
void launch_blur_hess(hesaff_ctx *c, const DPlane &in, const DPlane &outL, const DPlane &outR, const DPlane &outHalf, const float *taps, int K,
                      float norm2, int B)
{
   switch (K) {
      case 9: launch_march<9, WL, WR, WH>(c, in, outL, outR, outHalf, taps, norm2, B); return;
      case 11: launch_march<11, WL, WR, WH>(c, in, outL, outR, outHalf, taps, norm2, B); return;
      case 13: launch_march<13, WL, WR, WH>(c, in, outL, outR, outHalf, taps, norm2, B); return;
      case 15: launch_march<15, WL, WR, WH>(c, in, outL, outR, outHalf, taps, norm2, B); return;
      default: break;   // non-default initialSigma
   }
   if (K <= 2 * BH_RMAX + 1) {
      // LDS-tile kernel: any tap count up to 15
      const dim3 grid((in.cols + BH_TW - 1) / BH_TW, (in.rows + BH_TH - 1) / BH_TH, B);
      hipLaunchKernelGGL((k_blur_hess_tile<WL, WR, WH>), grid, dim3(256), 0, c->stream(), in, outL, outR, outHalf, taps, K, norm2);
      return;
   }
   // any larger tap count (initialSigma above ~1.9): plain two-pass blur + stand-alone response / decimation kernels
   const size_t planeF = (size_t)B * in.rows * in.pitch;
   c->b_generic.ensure(planeF * 4 * 2);
   const DPlane tmp = make_plane(c->b_generic.as<float>(), in.rows, in.cols, in.pitch);
   const DPlane blurred = WL ? outL : make_plane(c->b_generic.as<float>() + planeF, in.rows, in.cols, in.pitch);
   const dim3 grid((in.cols + 255) / 256, in.rows, B);
   hipLaunchKernelGGL(k_blur_rows_generic, grid, dim3(256), 0, c->stream(), in, tmp, taps, K);
   hipLaunchKernelGGL(k_blur_cols_generic, grid, dim3(256), 0, c->stream(), tmp, blurred, taps, K);
   if (WR) hipLaunchKernelGGL(k_hess, grid, dim3(256), 0, c->stream(), blurred, outR, norm2);
   if (WH) hipLaunchKernelGGL(k_half, dim3((outHalf.cols + 255) / 256, outHalf.rows, B), dim3(256), 0, c->stream(), blurred, outHalf);
}

// The source images of a batch in device memory: B images img_stride bytes apart, rows row_stride bytes apart, in one of three
// formats - 8-bit grey, 8-bit with three interleaved channels (hesaff.cpp:138-148 converts both), or float planes, the
// CV_32FC1 image detectPyramidKeypoints takes (pyramid.h:73; row_stride a multiple of 4).
enum SrcFormat { HS_SRC_U8C1 = 0, HS_SRC_U8C3 = 1, HS_SRC_F32 = 2 };
struct SrcImages {
   const uint8_t *p;
   int format;
   long long img_stride;
   int row_stride;
   int channels() const { return format == HS_SRC_U8C3 ? 3 : 1; }
   static SrcImages u8(const void *p, int channels, long long img_stride, int row_stride)
   {
      return SrcImages{(const uint8_t *)p, channels == 3 ? HS_SRC_U8C3 : HS_SRC_U8C1, img_stride, row_stride};
   }
   static SrcImages f32(const void *p, long long img_stride, int row_stride) { return SrcImages{(const uint8_t *)p, HS_SRC_F32, img_stride, row_stride}; }
};

struct Lists {
   CandList cl;
   RecList rl;
   HessList hl;
   AffineOut ao;
   PatchWork pw;
   CounterBlock *counters;
};

Lists make_lists(hesaff_ctx *c)
{
   Lists s;
   CounterBlock *cnt = c->b_counters.as<CounterBlock>();
   const hesaff_ctx::GeomBufs &g = c->geo;
   s.counters = cnt;
   s.cl.count = &cnt->head.cand; s.cl.items = g.b_cand.as<CandRec>(); s.cl.cap = c->cand_cap; s.cl.overflow = &cnt->head.overflow;
   const RecLayout rec = rec_layout(c->cap);
   s.rl.count = &cnt->head.rec; s.rl.cap = c->cap;
   s.rl.x = g.b_rec_f.at<float>(rec.x); s.rl.y = g.b_rec_f.at<float>(rec.y); s.rl.s = g.b_rec_f.at<float>(rec.s); s.rl.response = g.b_rec_f.at<float>(rec.response);
   s.rl.meta = g.b_rec_i.at<int32_t>(rec.meta); s.rl.cell = g.b_rec_i.at<uint32_t>(rec.cell); s.rl.key = g.b_rec_i.at<uint32_t>(rec.key);
   s.rl.bit = g.b_rec_i.at<uint32_t>(rec.bit); s.rl.word = g.b_rec_w.at<long long>(rec.word);
   const HessLayout hess = hess_layout(c->cap);
   s.hl.x = g.b_hess_f.at<float>(hess.x); s.hl.y = g.b_hess_f.at<float>(hess.y); s.hl.s = g.b_hess_f.at<float>(hess.s); s.hl.response = g.b_hess_f.at<float>(hess.response);
   s.hl.meta = g.b_hess_i.at<int32_t>(hess.meta); s.hl.r0c0 = g.b_hess_i.at<int32_t>(hess.r0c0); s.hl.cap = c->cap;
   const AffineLayout aff = affine_layout(c->cap);
   s.ao.converged = g.b_aff.at<int32_t>(aff.converged); s.ao.iters = g.b_aff.at<int32_t>(aff.iters); s.ao.U = g.b_aff.at<float>(aff.U);
   const PatchLayout patch = patch_layout(c->cap);
   s.pw.P0 = g.b_pw.at<int32_t>(patch.P0); s.pw.alive = g.b_pw.at<int32_t>(patch.alive); s.pw.A = g.b_pw.at<float>(patch.A);
   s.pw.bin_count = cnt->bin_count; s.pw.bin_work = cnt->bin_work; s.pw.bin_items = g.b_bins.at<uint32_t>(patch.bin_items); s.pw.cap = c->cap;
   return s;
}

// group_schedule.h's wait / record on a context: the logical streams through the pairing table, the events by name.  Every
// hipStreamWaitEvent and hipEventRecord of the keypoint stages is issued here (the stage timers' and the host round trips' apart).
struct ScheduleDevice {
   hesaff_ctx *c;
   hipStream_t stream(sched::Stream s) const { return c->sset.of(s); }
   hipEvent_t event(const sched::Event &e) const
   {
      switch (e.kind) {
         case sched::Event::DETECT_DONE: return c->ev_detect_done;
         case sched::Event::AFFINE_DONE: return c->ev_aff[e.index];
         case sched::Event::EXTRACT_DONE: return c->ev_extract_done[e.index];
         case sched::Event::SIFT_DONE: return c->ev_sift_done[e.index];
         case sched::Event::FORK: return c->ev_fork;
         case sched::Event::JOIN: return c->ev_join[e.index];
      }
      return nullptr;
   }
   void wait(sched::Stream s, const sched::Event &e) { HIP_TRY(hipStreamWaitEvent(stream(s), event(e), 0)); }
   void record(const sched::Event &e, sched::Stream s) { HIP_TRY(hipEventRecord(event(e), stream(s))); }
};

// normalizeAffine for every keypoint k_prepare_patch left alive and binned.  Every launch is a persistent grid of
// fixed size that reads its work-list length from the device-side bin counters: the host never waits for them.
// large_rows_bound: upper bound of the large bin's T' rows in this group (from k_image_large_rows).
// n_side: the side streams the caller has forked (fork_side_streams / join_side_streams, group_schedule.h; patch_side_streams says
// how many a context uses); bin i's kernel runs on patch_stream(i, n_side).
int patch_side_streams(const hesaff_ctx *c, const PlaneTab *pt) { return c->no_overlap ? 0 : (c->fast_pyramid && pt) ? 1 : HS_NSIDE; }

void launch_patch_kernels(hesaff_ctx *c, const Lists &s, const DPlane &image, float *patches_out, uint32_t h_base, uint32_t large_rows_bound,
                          const PlaneTab *pt, int n_side)
{
   hipStream_t st = c->stream();
   PatchIO io;
   memset(&io, 0, sizeof io);
   io.image = image;
   io.patches = patches_out;
   io.h_base = h_base;
   // The bins are independent (disjoint keypoints) and each kernel leaves CU resources idle
   // (LDS- or latency-bound), so they run concurrently on side streams.
   hipStream_t sb[HS_NSIDE];
   for (int i = 0; i < HS_NSIDE; i++) sb[i] = c->sset.of(sched::patch_stream(i, n_side));
   if (c->fast_pyramid && pt) {
      // hesaff_params.fast = 2: bin 0 (P <= 41) on the parity kernel, every larger window from the pyramid (k_patch_pyramid)
      hipLaunchKernelGGL(k_patch_extract_small<0>, dim3(c->g_small0), dim3(256), small_extract_lds_bytes(0), sb[0], s.hl, s.pw, io, c->tables.view);
      hipLaunchKernelGGL(k_patch_pyramid, dim3((uint32_t)c->n_cu * 32u), dim3(256), 0, st, s.hl, s.pw, io, *pt, (int)c->oct.size(), c->ct.consts.pd0, 1);
      return;
   }
   {
      PatchIO io2 = io;
      io2.trows = c->b_trows2.as<float>();
      PatchIO io3 = io;
      io3.trows = c->b_trows3.as<float>();
      hipLaunchKernelGGL(k_patch_extract_small<0>, dim3(c->g_small0), dim3(256), small_extract_lds_bytes(0), sb[0], s.hl, s.pw, io, c->tables.view);
      hipLaunchKernelGGL(k_patch_extract_small<1>, dim3(c->g_small1), dim3(256), small_extract_lds_bytes(1), sb[1], s.hl, s.pw, io, c->tables.view);
      hipLaunchKernelGGL(k_patch_mid<HS_MID_PMAX>, dim3(c->g_mid), dim3(256), mid_lds_bytes(), sb[2], s.hl, s.pw, io2, c->tables.view);
      hipLaunchKernelGGL(k_patch_mid<HS_BIN3_PMAX>, dim3(c->g_big), dim3(256), big_lds_bytes(), sb[3], s.hl, s.pw, io3, c->tables.view);
   }
   // the rare huge windows (P > 512): row tasks over all of them, then one block per keypoint, on the main stream, which shares its HIP
   // stream (= hardware queue) with bin 3.  That queue is the stage's longest on photographs (8.1 + 8.8 + 1.9 ms per 32 photograph mosaics
   // against 5.3 for the queue of bins 0 and 1), but the kernels behind bins 0 and 1 instead measured slower: photographs 397.2 / 394.9 ->
   // 407.5 / 406.3 ms per step (profiles/r06_notes.md).  k_prepare_patch orders them after the bin counts.
   if (large_rows_bound > 0) {
      const uint32_t rows_cap = std::max(large_rows_bound, c->trows_rows);
      c->b_trows.ensure((size_t)rows_cap * HS_NEED * 4);
      c->b_rowprefix.ensure(((size_t)c->cap + 1) * 4);
      io.trows = c->b_trows.as<float>();
      io.row_prefix = c->b_rowprefix.as<uint32_t>();
      io.trows_cap = rows_cap;
      io.overflow = &s.counters->head.row_overflow;
      hipLaunchKernelGGL(k_large_prefix, dim3(1), dim3(256), 0, st, s.pw, c->b_rowprefix.as<uint32_t>());
      // one launch, or two when the batch's largest window is far above the common ones (large_rows_split, large_rows_launch: batch_plan.h)
      const LargeSplit sp = large_rows_split(c->tables.view.max_p0, c->batch_max_p);
      for (int i = 0; i < sp.n; i++) {
         const LargeLaunch ll = large_rows_launch(sp.p_hi[i], c->tables.view.max_p0, large_rows_bound);
         hipLaunchKernelGGL(k_patch_large_rows, dim3(ll.grid_blocks), dim3(64 * ll.wavefronts), ll.lds_bytes, st, s.hl, s.pw, io, c->tables.view, ll.srow_stride,
                            ll.tap_stride, ll.nrow, sp.p_lo[i], std::min(sp.p_hi[i], 0x7ffffff0));
      }
      hipLaunchKernelGGL(k_patch_large_finish, dim3(c->g_lfin), dim3(256), 0, st, s.pw, io, c->tables.view);
   }
}

// the patch stage on its own (hesaff_stage_normalize_affine): no plane table, so never fast mode 2's kernels
void run_patch_stage(hesaff_ctx *c, const Lists &s, const DPlane &image, float *patches_out, uint32_t h_base, uint32_t large_rows_bound)
{
   ScheduleDevice dev{c};
   const int n_side = patch_side_streams(c, nullptr);
   sched::fork_side_streams(dev, 0, n_side);
   launch_patch_kernels(c, s, image, patches_out, h_base, large_rows_bound, nullptr, n_side);
   sched::join_side_streams(dev, 0, n_side);
}

// k_orientation's grid over n keypoints: one wavefront each, at most the 8 blocks per CU its 19536 B (19.1 KiB) of LDS admit
uint32_t orientation_grid(const hesaff_ctx *c, uint32_t n) { return std::max<uint32_t>(1u, std::min<uint32_t>(n, (uint32_t)c->n_cu * 8u)); }

// The orientation count in force: hesaff_set_orientation_count's K in HESAFF_ORI_DOMINANT, 1 - the feature inert - in HESAFF_ORI_UP.
int ori_count(const hesaff_ctx *c) { return c->orientation == HESAFF_ORI_DOMINANT ? c->orientation_count : 1; }

// The rank arrays of K > 1 over the current keypoint capacity: frames, window sides, flags and descriptor rows of the ranks 1 .. K - 1
// (rank_layout, buffer_layouts.h).  ensure_rank_arrays allocates them (HESAFF_ERR_NOMEM when the device cannot hold them).
OrientRanks rank_arrays(const hesaff_ctx *c, int K)
{
   OrientRanks r;
   memset(&r, 0, sizeof r);
   const RankLayout L = rank_layout(K, c->cap);
   const DevBuf &b = c->b_ori_ranks;
   r.K = K; r.cap = c->cap;
   r.A = b.at<float>(L.A); r.P0 = b.at<int32_t>(L.P0); r.alive = b.at<int32_t>(L.alive); r.desc = b.at<uint8_t>(L.desc);
   return r;
}
void ensure_rank_arrays(hesaff_ctx *c, int K) { c->b_ori_ranks.ensure(std::max<size_t>(rank_layout(K, c->cap).bytes, 16)); }

// per image: upper bound of the T' rows its huge windows (P > 512) need, known from the scales alone
void launch_image_large_rows(hesaff_ctx *c, const Lists &s, int B)
{
   const StartsBlock<uint32_t> sb = starts_block(c->geo.b_starts.as<uint32_t>(), B);
   HIP_TRY(hipMemsetAsync(sb.large_rows(), 0, sb.words_to_clear() * 4, c->stream()));
   hipLaunchKernelGGL(k_image_large_rows, dim3(512), dim3(256), 0, c->stream(), s.hl, (const uint32_t *)&s.counters->head.hess_total, c->ct.consts.mrSize,
                      sb.large_rows(), B, c->tables.view.max_p0);
}

// The three steps of detection that follow the response planes.  run_detection calls them on the planes it has just made,
// hesaff_stage_detect_planes (capi_stage.h) on the planes of its caller: one set of launches for both.
// begin_detection: the counters, the bitmask and the order-key map before the first octave of a batch
void begin_detection(hesaff_ctx *c, const Lists &s, int B)
{
   hipStream_t st = c->stream();
   HIP_TRY(hipMemsetAsync(s.counters, 0, sizeof(CounterBlock), st));
   HIP_TRY(hipMemsetAsync(c->geo.b_bitmask.p, 0, std::max<size_t>((size_t)B * c->words_per_image * 8, 8), st));
   // octaveMap (pyramid.cpp:226: zeroed per octave): the order-key map is filled with "free" when it is new; every pass over an octave then bids
   // with keys of a fresh, smaller epoch (OctaveCtx::map_epoch), so what earlier passes left behind never wins - no fill and no reset per octave
   if (c->map_epochs.begin_batch()) HIP_TRY(hipMemsetAsync(c->geo.b_map.p, 0xFF, c->geo.b_map.bytes, st));
}

// detect_octave: extrema scan, localisation and the octaveMap rule on octave o, whose blur planes are Lo[0..3] and response planes Ro[0..4].
// band_override: the band height of k_extrema_march (0: extrema_band's choice; only the stage entry point passes anything else).
void detect_octave(hesaff_ctx *c, const Lists &s, StageTimer &tm, int B, size_t o, const DPlane *Lo, const DPlane *Ro, int band_override = 0)
{
   const hesaff::OctaveSchedule &sc = c->ct.sched;
   hipStream_t st = c->stream();
   CounterBlock *cnt = s.counters;
   const OctGeom &g = c->oct[o];
   const int t = tm.begin(T_DET);
   HIP_TRY(hipMemsetAsync(&cnt->head.cand, 0, 4, st));
   HIP_TRY(hipMemcpyAsync(&cnt->oct_rec_start[o], &cnt->head.rec, 4, hipMemcpyDeviceToDevice, st));
   OctaveCtx oc;
   for (int l = 0; l < 5; l++) { oc.R[l] = Ro[l]; oc.L[l] = Lo[l]; oc.sigma[l] = sc.level_sigma[l]; }
   oc.pixelDistance = c->ct.consts.pd0 * (float)(1 << o);   // pyramid.cpp:288: doubles per octave
   oc.octave = (int)o;
   oc.map = c->geo.b_map.as<uint32_t>();
   // a fresh epoch for this pass (counting down; the all-ones epoch is the fill value): refill when they have run out
   const OrderMapEpochs::Pass pass = c->map_epochs.next_pass();
   if (pass.refill_first) HIP_TRY(hipMemsetAsync(c->geo.b_map.p, 0xFF, c->geo.b_map.bytes, st));
   oc.map_epoch = pass.epoch_bits;
   oc.word_base = g.word_base;
   oc.words_per_image = c->words_per_image;
   oc.words_per_row = g.words_per_row;
   if (g.rows > 2 * HS_BORDER && g.cols > 2 * HS_BORDER) {
      FivePlanes fp;
      for (int l = 0; l < 5; l++) fp.R[l] = Ro[l];
      const int strips = (g.cols + EXM_STRIP - 1) / EXM_STRIP;
      const int band = band_override > 0 ? band_override : extrema_band(g.rows, g.cols, B);
      const dim3 grid(strips, (g.rows + band - 1) / band, B);
      const int te = tm.begin(T_EXTREMA, 20.0 * (double)B * g.rows * g.cols);
      hipLaunchKernelGGL(k_extrema_march, grid, dim3(64), 0, st, fp, c->ct.consts.positiveThreshold, c->ct.consts.negativeThreshold, s.cl, band);
      tm.end(te);
      hipLaunchKernelGGL(k_localize, dim3(HS_GRID_LOC), dim3(256), 0, st, oc, s.cl, s.rl, c->ct.consts);
      hipLaunchKernelGGL(k_dedupe, dim3(HS_GRID_DED), dim3(256), 0, st, oc, s.rl, (const uint32_t *)&cnt->oct_rec_start[o],
                         c->geo.b_bitmask.as<unsigned long long>());
   }
   tm.end(t);
}

// order_hessian_list: the surviving records of all octaves at their ranks in the reference's detection order, and the per-image starts
void order_hessian_list(hesaff_ctx *c, const Lists &s, StageTimer &tm, int B)
{
   hipStream_t st = c->stream();
   CounterBlock *cnt = s.counters;
   const int t = tm.begin(T_DET);
   const long long total_words = (long long)B * c->words_per_image;
   LoadPopc lp; lp.p = c->geo.b_bitmask.as<unsigned long long>();
   exclusive_scan(c, lp, total_words, c->geo.b_prefix.as<uint32_t>(), &cnt->head.hess_total);
   // the records at their ranks as 32-byte items (in the candidate buffer: its last reader, the last octave's k_localize, is done), then dealt out
   HessItem *items = reinterpret_cast<HessItem *>(c->geo.b_cand.p);
   static_assert(sizeof(HessItem) == 32 && sizeof(CandRec) >= sizeof(HessItem), "the items fit the candidate slots (cand_cap >= cap)");
   hipLaunchKernelGGL(k_scatter_ordered, dim3(HS_GRID_SCAT), dim3(256), 0, st, s.rl, (const unsigned long long *)c->geo.b_bitmask.p,
                      (const uint32_t *)c->geo.b_prefix.p, items, s.hl.cap);
   hipLaunchKernelGGL(k_hess_deal, dim3(HS_GRID_SCAT), dim3(256), 0, st, (const HessItem *)items, (const uint32_t *)&cnt->head.hess_total, s.hl);
   hipLaunchKernelGGL(k_image_counts, dim3((B + 1 + 63) / 64), dim3(64), 0, st, (const uint32_t *)c->geo.b_prefix.p,
                      c->words_per_image, B, (const uint32_t *)&cnt->head.hess_total, c->geo.b_starts.as<int32_t>());
   launch_image_large_rows(c, s, B);
   tm.end(t);
}

// ---- the pyramid builder: the first level, then octave by octave the launches of batch_plan.h's step table ----
void launch_gray_plane(hesaff_ctx *c, const SrcImages &src, int B)
{
   const dim3 grid((c->W + 1023) / 1024, c->H, B);
   if (src.format == HS_SRC_F32) hipLaunchKernelGGL(k_gray_plane<2>, grid, dim3(256), 0, c->stream(), src.p, src.img_stride, src.row_stride, c->gray);
   else if (src.format == HS_SRC_U8C3) hipLaunchKernelGGL(k_gray_plane<1>, grid, dim3(256), 0, c->stream(), src.p, src.img_stride, src.row_stride, c->gray);
   else hipLaunchKernelGGL(k_gray_plane<0>, grid, dim3(256), 0, c->stream(), src.p, src.img_stride, src.row_stride, c->gray);
}

// The planes of octave o of a batch of B images: L[0..2] the kept levels, L[3] and R[0..4] one octave's worth of b_L3 / b_R, which every
// octave overwrites.  L[4] is empty: detection never reads it (getHessianPointType reads L1..L3); who wants it supplies a plane.
struct OctavePlanes { DPlane L[5], R[5]; };
OctavePlanes octave_planes(hesaff_ctx *c, size_t o, int B)
{
   const OctGeom &g = c->oct[o];
   const size_t planeF = (size_t)B * g.rows * g.pitch;
   OctavePlanes P;
   for (int l = 0; l < 3; l++) P.L[l] = c->L[o * 3 + l];
   P.L[3] = make_plane(c->geo.b_L3.as<float>(), g.rows, g.cols, g.pitch);
   P.L[4] = make_plane(nullptr, 0, 0, 0);
   for (int l = 0; l < 5; l++) P.R[l] = make_plane(c->geo.b_R.as<float>() + l * planeF, g.rows, g.cols, g.pitch);
   return P;
}

// The grey plane (normalizeAffine's input) and the first level L0 of octave 0, of the B device images src (SrcImages: 8-bit with 1 or
// 3 interleaved channels, or float planes).
void build_first_level(hesaff_ctx *c, const SrcImages &src, int B, StageTimer &tm)
{
   hipStream_t st = c->stream();
   const float *taps = c->tables.pyr_taps.as<float>() + c->ct.pyr_tap_off[0];
   const int t = tm.begin(T_PYR);
   const DPlane none = make_plane(nullptr, 0, 0, 0);
   // Default parameters: grey conversion (hesaff.cpp:138-148) fused into the initial blur 0.5 -> 1.6 (pyramid.cpp:276-280,
   // K = 11): the source images are read once, the float grey plane and L0 are written.
   // 8-bit images: 9 B/px (read 1, write 4 + 4); float planes: 12 B/px (read 4, write 4 + 4).
   const bool fused_gray = !c->oct.empty() && c->ct.pyr_K[0] == 11 && !c->ct.up;
   if (fused_gray) {
      GraySrc gs;
      gs.p = src.p; gs.channels = src.channels(); gs.img_stride = src.img_stride; gs.row_stride = src.row_stride;
      const int tb = tm.begin(T_BLURHESS, 0);   // not one of the 58 B/px launches (bytes 0)
      if (src.format == HS_SRC_F32)
         launch_march<11, true, false, false, false, SRC_F32>(c, c->gray, c->L[0], none, none, taps, 0.0f, B, DPlane(), 0.0f, gs, c->gray);
      else
         launch_march<11, true, false, false, false, SRC_U8>(c, c->gray, c->L[0], none, none, taps, 0.0f, B, DPlane(), 0.0f, gs, c->gray);
      tm.end(tb);
   } else {
      // grey conversion; without an initial blur (initialSigma <= the input's own blur) it is the first level directly
      launch_gray_plane(c, src, B);
      if (c->ct.up) {
         // pyramid.cpp:267-271: the first level is the 2x up-sampled image (doubleImage, helpers.cpp:297-329)
         const dim3 g2((c->upimg.cols + 255) / 256, c->upimg.rows, B);
         hipLaunchKernelGGL(k_double, g2, dim3(256), 0, st, c->gray, c->upimg);
      }
      const DPlane &first = c->ct.up ? c->upimg : c->gray;
      if (c->ct.pyr_K[0] == 0 && !c->oct.empty()) HIP_TRY(hipMemcpyAsync(c->L[0].p, first.p, (size_t)B * first.img_stride * 4, hipMemcpyDeviceToDevice, st));
      if (!c->oct.empty() && c->ct.pyr_K[0] > 0) {
         // pyramid.cpp:276-280 initial blur 0.5 -> initialSigma
         const int tb = tm.begin(T_BLURHESS, 0);   // initial blur: not counted in the 12N launches (bytes 0)
         launch_blur_hess<true, false, false>(c, first, c->L[0], none, none, taps, c->ct.pyr_K[0], 0.0f, B);
         tm.end(tb);
      }
   }
   tm.end(t);
}

// What `want` asks of octave o, whose first level P.L[0] exists: octave_steps (batch_plan.h) says which blur launches that takes and what
// each writes.  DetectKeepL4: P.L[4] is the caller's plane.  BlursOnly touches the blur planes and nothing else.
void build_octave(hesaff_ctx *c, size_t o, int B, const OctavePlanes &P, OctaveWant want, StageTimer &tm)
{
   const hesaff::OctaveSchedule &sc = c->ct.sched;
   const OctGeom &g = c->oct[o];
   const OctaveSteps steps = octave_steps(want, o + 1 < c->oct.size(), c->ct.pyr_march);
   const DPlane none = make_plane(nullptr, 0, 0, 0);
   const int t = tm.begin(T_PYR);
   if (steps.hess_first) {
      const dim3 grid((g.cols + 255) / 256, g.rows, B);
      hipLaunchKernelGGL(k_hess, grid, dim3(256), 0, c->stream(), P.L[0], P.R[0], sc.norm2[0]);
   }
   for (int i = 1; i <= 4; i++) {
      const BlurStep &b = steps.step[i];
      if (!b.launch) continue;
      const DPlane &in = P.L[b.in], &outL = b.write_L ? P.L[i] : none, &outR = b.write_R ? P.R[i] : none;
      const DPlane &half = b.write_half ? c->L[(o + 1) * 3] : none;
      const float *taps = c->tables.pyr_taps.as<float>() + c->ct.pyr_tap_off[i];
      const int K = c->ct.pyr_K[i];
      const float norm2 = b.write_R ? sc.norm2[i] : 0.0f;
      const int tb = tm.begin(T_BLURHESS, b.bytes_per_px * (double)B * g.rows * g.cols);
      // the five output sets the table can ask for (tests/native/plan_check.cpp enumerates it), each its own instantiation
      if (b.write_R0) launch_march<9, true, true, false, true>(c, in, outL, outR, none, taps, norm2, B, P.R[0], sc.norm2[0]);
      else if (b.write_L && b.write_R && b.write_half) launch_blur_hess<true, true, true>(c, in, outL, outR, half, taps, K, norm2, B);
      else if (b.write_L && b.write_R) launch_blur_hess<true, true, false>(c, in, outL, outR, none, taps, K, norm2, B);
      else if (b.write_L) launch_blur_hess<true, false, false>(c, in, outL, none, none, taps, K, norm2, B);
      else if (b.write_R) launch_blur_hess<false, true, false>(c, in, none, outR, none, taps, K, norm2, B);
      else launch_blur_hess<false, false, true>(c, in, none, none, half, taps, K, norm2, B);
      tm.end(tb);
   }
   tm.end(t);
}

// The scale-space + detection part for the current plan; fills the ordered Hessian list.
void run_detection(hesaff_ctx *c, const SrcImages &src, int B, const Lists &s, StageTimer &tm)
{
   begin_detection(c, s, B);
   build_first_level(c, src, B, tm);
   for (size_t o = 0; o < c->oct.size(); o++) {
      const OctavePlanes P = octave_planes(c, o, B);
      build_octave(c, o, B, P, OctaveWant::Detect, tm);
      detect_octave(c, s, tm, B, o, P.L, P.R);
   }
   order_hessian_list(c, s, tm, B);
}

__global__ void k_desc_starts(const int32_t *__restrict__ hess_starts, int nimg, const uint32_t *__restrict__ rank,
                              const uint32_t *__restrict__ n_hess, const uint32_t *__restrict__ total_desc, int32_t *__restrict__ out)
{
   const int b = blockIdx.x * blockDim.x + threadIdx.x;
   if (b > nimg) return;
   const uint32_t hs = (uint32_t)hess_starts[b];
   out[b] = (b == nimg || hs >= *n_hess) ? (int32_t)*total_desc : (int32_t)rank[hs];
}

void collect_timings(hesaff_ctx *c, StageTimer &tm, int B)
{
   hesaff_timings &t = c->tm;
   memset(&t, 0, sizeof t);
   for (const EvPair &p : tm.pairs) {
      float ms = 0;
      (void)hipEventElapsedTime(&ms, p.a, p.b);
      switch (p.kind) {
         case T_PYR: t.pyramid_ms += ms; break;
         case T_DET: t.detect_ms += ms; break;
         case T_AFF: t.affine_ms += ms; break;
         case T_PATCH: t.patch_ms += ms; break;
         case T_SIFT: t.sift_ms += ms; break;
         case T_PACK: t.pack_ms += ms; break;
         case T_TOTAL: t.total_ms += ms; break;
         case T_BLURHESS:
            if (p.bytes > 0) { t.blur_hess_ms += ms; t.blur_hess_launches++; t.blur_hess_bytes += p.bytes; }
            break;
         case T_EXTREMA: t.extrema_ms += ms; t.extrema_launches++; t.extrema_bytes += p.bytes; break;
      }
   }
   double sumN = 0;
   for (const OctGeom &g : c->oct) sumN += (double)g.rows * g.cols;
   t.pyramid_bytes = (double)B * (5.0 * c->H * c->W + 58.0 * sumN);
   t.export_ms = c->export_ms; t.export_rows = c->export_rows;   // (run_chunks keeps them across the batches of a list)   // (+ the up-sampling pass when upscaleInputImage is set: not counted)
}

// The descriptor kernels (kernels_sift.h) over n patches in HBM.  (Slices of a group, each slice's kernels back to back so that
// the intermediates stay in the memory-side cache, measured no faster: sweep in profiles/r06_notes.md.)
// desc_mode: HESAFF_DESC_SIFT / HESAFF_DESC_ROOTSIFT - the pipeline passes the context's mode, a stage operator its own.
void launch_sift(hesaff_ctx *c, hipStream_t ss, const SiftIO &so, uint32_t n, float2 *vo, int desc_mode)
{
   hipLaunchKernelGGL(k_sift_meanvar, dim3((n + SM_KP - 1) / SM_KP), dim3(64), 0, ss, so, c->tables.view);
   hipLaunchKernelGGL(k_sift_grad, dim3(std::min(n, c->sgrad_grid)), dim3(256), 0, ss, so, c->tables.view, vo);
   const dim3 hg(std::min<uint32_t>((n + 3) / 4, c->g_shist));
   if (desc_mode == HESAFF_DESC_ROOTSIFT)
      hipLaunchKernelGGL(k_sift_hist<HESAFF_DESC_ROOTSIFT>, hg, dim3(64), 0, ss, so, c->tables.view, (const float2 *)vo, c->ct.consts.maxBinValue);
   else
      hipLaunchKernelGGL(k_sift_hist<HESAFF_DESC_SIFT>, hg, dim3(64), 0, ss, so, c->tables.view, (const float2 *)vo, c->ct.consts.maxBinValue);
}

// per-group patch / descriptor buffers: sized once per batch for the largest group
void ensure_group_buffers(hesaff_ctx *c, uint32_t n)
{
   // The patch buffers rotate over HS_NSLOT slots (the patch stage fills one while the descriptor stage reads the others).  The
   // descriptor stage's own intermediates - gradient pairs (10.4 KB per keypoint), mean / variance - live and die on its
   // one stream (the main stream with HESAFF_OVERLAP=0), so one copy of them serves every group.
   const GroupScratch gs = group_scratch(n);   // (buffer_layouts.h: hesaff_stage_sift sizes its arrays with it too)
   for (int slot = 0; slot < HS_NSLOT; slot++) c->b_patches2[slot].ensure_grow(gs.patch_floats * sizeof(float));
   c->b_meanvar2.ensure_grow(gs.meanvar_floats * sizeof(float));
   // the (mask*grad, o) pairs of pixels outside the circular mask stay (0, 0): zero-fill on (re)allocation
   const void *before = c->b_siftvo2.p;
   const size_t bytes_before = c->b_siftvo2.bytes;
   c->b_siftvo2.ensure_grow(gs.vo_floats * sizeof(float));
   if (c->b_siftvo2.p != before || c->b_siftvo2.bytes != bytes_before) HIP_TRY(hipMemsetAsync(c->b_siftvo2.p, 0, c->b_siftvo2.bytes, c->stream()));
}

// The host round trip of a batch: the per-image Hessian starts and the large-window row bounds (all of b_starts: StartsBlock::words_to_copy)
// into pinned memory; the caller's thread sleeps until everything before it on the main stream has run.
const int32_t *fetch_hessian_starts(hesaff_ctx *c, int B)
{
   hipStream_t st = c->stream();
   const size_t bytes = starts_block(c->geo.b_starts.as<int32_t>(), B).words_to_copy() * 4;
   int32_t *hs = (int32_t *)c->h_small_mid.ensure_small(bytes);
   HIP_TRY(hipMemcpyAsync(hs, c->geo.b_starts.p, bytes, hipMemcpyDeviceToHost, st));
   HIP_TRY(hipEventRecord(c->ev_detect_done, st));
   const double dbg_ca = c->debug ? thread_cpu_ms() : 0.0;
   hs_wait_event(c->ev_detect_done);   // sleeps: no core spins while the detection stage runs
   if (c->debug) fprintf(stderr, "[hesaff] run_batch: caller's CPU inside the wait for the detection stage %.2f ms\n", thread_cpu_ms() - dbg_ca);
   return hs;
}

// What a batch produced besides the KeyRec records in b_out: B + 1 Hessian starts and B + 1 descriptor starts (image b owns
// [starts[b], starts[b + 1])) in pinned host memory, and the descriptor starts on the device.  Valid until the next batch.
struct BatchResult {
   const int32_t *hessian_starts, *desc_starts;
   const int32_t *d_desc_starts;
};

// run_group_schedule's device (group_schedule.h): the launches of the keypoint stages of one batch, each with its timer bracket, on
// the stream the schedule names.  The order, the waits and the slots are the schedule's; nothing here decides any of them.
// Rank 0 lives in the base lists and b_desc; with an orientation count K > 1 a rank r >= 1 has its own frames, window sides, flags and
// descriptor rows (mr) - the bins and their counters are the one set, cleared for every pass.
struct GroupDevice : ScheduleDevice {
   const Lists &s;
   StageTimer &tm;
   const std::vector<ImageGroup> &groups;
   const PlaneTab &pt;
   int H, W;
   OrientRanks mr;   // K > 1 only: nothing of it is read for rank 0
   int t_patch = -1;
   GroupDevice(hesaff_ctx *ctx, const Lists &s_, StageTimer &tm_, const std::vector<ImageGroup> &groups_, const PlaneTab &pt_, int H_, int W_, const OrientRanks &mr_)
      : ScheduleDevice{ctx}, s(s_), tm(tm_), groups(groups_), pt(pt_), H(H_), W(W_), mr(mr_)
   {
      while (c->ev_aff.size() < groups.size()) c->ev_aff.emplace_back(hipEventDisableTiming);
   }
   Lists lists(int r) const
   {
      Lists sr = s;
      if (r > 0) { sr.pw.A = mr.A_of(r); sr.pw.P0 = mr.P0_of(r); sr.pw.alive = mr.alive_of(r); }
      return sr;
   }
   void affine(int g, sched::Stream as)
   {
      const int ta = tm.begin(T_AFF, 0, stream(as));
      const uint32_t agrid = std::min<uint32_t>((groups[g].hi - groups[g].lo + HS_AFF_SLOTS - 1) / HS_AFF_SLOTS, (uint32_t)c->n_cu * HS_AFF_BLOCKS_PER_CU);
      hipLaunchKernelGGL(k_affine, dim3(agrid), dim3(64), 0, stream(as), pt, s.hl, groups[g].lo, groups[g].hi, (const uint32_t *)&s.counters->head.hess_total,
                         c->tables.view, c->ct.consts, s.ao);
      tm.end(ta);
   }
   void pass_prepare(int g, int r, sched::Pass pass)
   {
      hipStream_t st = c->stream();
      if (pass == sched::PASS_UPRIGHT || r > 0) t_patch = tm.begin(T_PATCH);   // the unit's first pass; patch_done ends the bracket
      HIP_TRY(hipMemsetAsync(s.counters->bin_count, 0, CounterBlock::bins_bytes(), st));   // bin counts and work counters
      // (the group's end travels as a kernel argument: a 4-byte copy from pageable memory would make the host wait
      //  here until the stream has drained, once per group)
      if (pass == sched::PASS_UPRIGHT)
         hipLaunchKernelGGL(k_prepare_patch, dim3(1024), dim3(256), 0, st, s.hl, groups[g].lo, groups[g].hi, (const uint32_t *)&s.counters->head.hess_total, s.ao, H, W,
                            c->ct.consts, c->tables.view, s.pw);
      else
         hipLaunchKernelGGL(k_prepare_patch_second, dim3(1024), dim3(256), 0, st, s.hl, groups[g].lo, groups[g].hi, (const uint32_t *)&s.counters->head.hess_total, H, W,
                            c->ct.consts, c->tables.view, lists(r).pw);
   }
   void patch_kernels(int g, int r, int slot, int n_side)
   {
      launch_patch_kernels(c, lists(r), c->gray, c->b_patches2[slot].as<float>(), groups[g].lo, groups[g].large_rows, &pt, n_side);
   }
   // inside the patch stage's timer bracket, like the turned pass behind it; the multi form also writes the frames and flags of every rank >= 1
   void orientation(int g, int slot)
   {
      OrientIO oi;
      memset(&oi, 0, sizeof oi);
      oi.patches = c->b_patches2[slot].as<float>(); oi.h_lo = groups[g].lo; oi.h_hi = groups[g].hi;
      oi.n_ptr = &s.counters->head.hess_total; oi.cap = s.hl.cap; oi.alive = s.pw.alive; oi.A = s.pw.A;
      const dim3 grid(orientation_grid(c, groups[g].hi - groups[g].lo));
      if (mr.K > 1) hipLaunchKernelGGL(k_orientation_peaks, grid, dim3(64), 0, c->stream(), oi, c->tables.view, mr);
      else hipLaunchKernelGGL(k_orientation, grid, dim3(64), 0, c->stream(), oi, c->tables.view);
   }
   void patch_done(int) { tm.end(t_patch); }
   void descriptors(int g, int r, int slot, sched::Stream ss)
   {
      SiftIO so;
      so.patches = c->b_patches2[slot].as<float>(); so.alive = lists(r).pw.alive; so.meanvar = c->b_meanvar2.as<float>();
      so.vec = nullptr; so.desc = r > 0 ? mr.desc_of(r) : c->geo.b_desc.as<uint8_t>(); so.h_lo = groups[g].lo; so.h_hi = groups[g].hi;
      const int ts = tm.begin(T_SIFT, 0, stream(ss));
      launch_sift(c, stream(ss), so, groups[g].hi - groups[g].lo, c->b_siftvo2.as<float2>(), c->descriptor);
      tm.end(ts);
   }
};

// The launch of a kernel over the frame of kernels_words.h: one wavefront per work item, HS_WORD_BLOCK_WAVES to a block
template <class Kernel, class... Args>
void launch_word_kernel(Kernel kernel, hipStream_t st, long long waves, Args... args)
{
   const long long blocks = (waves + HS_WORD_BLOCK_WAVES - 1) / HS_WORD_BLOCK_WAVES;
   hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(HS_WORD_BLOCK_WAVES * 64), 0, st, args...);
}
// the wavefronts of the flat kernels: HS_WORD_WAVE_KEYS keys each
long long word_waves(long long n) { return (n + HS_WORD_WAVE_KEYS - 1) / HS_WORD_WAVE_KEYS; }

// k_assign_words against a packed vocabulary of n_tiles tiles (the context's, or the private one of a training call), n >= 1
void launch_assign_kernel(hipStream_t st, const void *tiles, const void *norms, int n_tiles, const void *d_desc, long long n, long long stride, long long offset,
                          void *d_out)
{
   launch_word_kernel(k_assign_words, st, word_waves(n), (const uint8_t *)d_desc, n, stride, offset, (const hs_v4i *)tiles, (const int32_t *)norms, n_tiles,
                      (int32_t *)d_out);
}

// k_assign_neighbours against the same: the R least (dist2, row) per key into d_out [n][R][2], rank 0 into d_words [n][2] as well
// where that is not nullptr; 1 <= R <= HS_NEIGH_MAX, n >= 1.  The list capacity is the least of 2, 4, 8 that holds R.
void launch_neighbours_kernel(hipStream_t st, const void *tiles, const void *norms, int n_tiles, const void *d_desc, long long n, long long stride, long long offset,
                              int R, void *d_out, void *d_words)
{
   const auto launch = [&](auto kernel) {
      launch_word_kernel(kernel, st, word_waves(n), (const uint8_t *)d_desc, n, stride, offset, (const hs_v4i *)tiles, (const int32_t *)norms, n_tiles, R,
                         (int32_t *)d_out, (int32_t *)d_words);
   };
   if (R <= 2) launch(k_assign_neighbours<2>);
   else if (R <= 4) launch(k_assign_neighbours<4>);
   else launch(k_assign_neighbours<8>);
}

// A cell layer and its working arrays as the kernels receive them (kernels_cells.h): the context's (launch_assign_cells) or the private
// ones of a training call (capi_train.h)
struct CellsDevice {
   const void *tiles, *norms;   // the packed coarse rows
   int n_tiles, c;
   const uint32_t *first;       // [c + 1]
   int32_t *coarse, *fine = nullptr;   // fine: with probes only (ProbeScratch), set by launch_assign_cells
   uint32_t *perm, *sub, *cursor, *item_first, *block_sums, *total;
   size_t sub_bytes;
   int slots;
};
CellsDevice cells_device(void *layer, const CellLayerArrays &a, int cells, void *scratch, const CellScratch &s)
{
   const auto at = [](void *base, size_t off) { return (void *)((char *)base + off); };
   CellsDevice d;
   d.tiles = at(layer, a.tiles.off); d.norms = at(layer, a.norms.off); d.first = (const uint32_t *)at(layer, a.first.off);
   d.n_tiles = a.n_tiles; d.c = cells;
   d.coarse = (int32_t *)at(scratch, s.coarse.off); d.perm = (uint32_t *)at(scratch, s.perm.off); d.sub = (uint32_t *)at(scratch, s.sub.off);
   d.cursor = (uint32_t *)at(scratch, s.cursor.off); d.item_first = (uint32_t *)at(scratch, s.item_first.off);
   d.block_sums = (uint32_t *)at(scratch, s.block_sums.off); d.total = (uint32_t *)at(scratch, s.total.off);
   d.sub_bytes = s.sub.bytes(); d.slots = s.slots;
   return d;
}

// k_probe_cells: the `used` nearest cells of each of n >= 1 keys, 1 <= used <= the layer's cells, n * used <= 2^24: (cell, dist2) per
// entry key * used + rank into d_out
void launch_probe_kernel(hipStream_t st, const CellsDevice &d, const void *d_desc, long long n, long long stride, long long offset, int used, void *d_out)
{
   launch_word_kernel(k_probe_cells, st, word_waves(n), (const uint8_t *)d_desc, n, stride, offset, (const hs_v4i *)d.tiles, (const int32_t *)d.norms, d.n_tiles,
                      used, (int32_t *)d_out);
}

// the first two steps of an assignment through cells, for 1 <= n * used <= 2^24 entries (used = 1: an entry is a key): every key's
// coarse cell - with used > 1 its `used` nearest cells, an entry each - then the entries grouped by cell (perm, the cursor) and each
// cell's first work item (item_first).  ev: two events, recorded behind either step, or nullptr.
void launch_cells_group(hesaff_ctx *c, const CellsDevice &d, const void *d_desc, int n_keys, long long stride, long long offset, const DevEvent *ev, int used = 1)
{
   hipStream_t st = c->stream();
   if (used > 1) launch_probe_kernel(st, d, d_desc, n_keys, stride, offset, used, d.coarse);
   else launch_assign_kernel(st, d.tiles, d.norms, d.n_tiles, d_desc, n_keys, stride, offset, d.coarse);
   if (ev) HIP_TRY(hipEventRecord(ev[0], st));
   HIP_TRY(hipMemsetAsync(d.sub, 0, d.sub_bytes, st));
   // (k_word_histogram and k_word_scatter: the same grid, so that a key's wave, and with it its slot, is the same in both)
   const int n = (int)cells_probe_entries(n_keys, used);
   const uint32_t key_blocks = (uint32_t)((n + 255) / 256);
   hipLaunchKernelGGL(k_word_histogram, dim3(key_blocks), dim3(256), 0, st, (const int32_t *)d.coarse, 2, n, d.sub, d.slots, (unsigned long long *)nullptr);
   LoadU32 load;
   load.p = d.sub;
   exclusive_scan(c, load, (long long)d.c * d.slots, d.cursor, d.total, d.block_sums);
   hipLaunchKernelGGL(k_word_scatter, dim3(key_blocks), dim3(256), 0, st, (const int32_t *)d.coarse, 2, n, d.cursor, d.slots, d.perm);
   LoadCellItems items;
   items.p = d.cursor; items.slots = d.slots;
   exclusive_scan(c, items, (long long)d.c, d.item_first, d.item_first + d.c, d.block_sums);
   if (ev) HIP_TRY(hipEventRecord(ev[1], st));
}

// the third step: k_assign_words_cells over the grouped keys against a packed flat vocabulary, (word, dist2) per key into d_out.  With
// used > 1 (d.fine is set): over the grouped entries into d.fine, then k_merge_probes, each key's least (dist2, row) into d_out.
void launch_cells_fine(hipStream_t st, const CellsDevice &d, const void *tiles, const void *norms, const void *d_desc, int n, long long stride, long long offset,
                       void *d_out, int used = 1)
{
   const long long items = cells_probe_item_bound(n, used, d.c);
   const auto launch = [&](auto kernel, int32_t *out) {
      launch_word_kernel(kernel, st, items, (const uint8_t *)d_desc, stride, offset, (const uint32_t *)d.perm, (const uint32_t *)d.cursor, d.slots,
                         (const uint32_t *)d.item_first, d.first, d.c, (const hs_v4i *)tiles, (const int32_t *)norms, out, used);
   };
   if (used > 1) {
      launch(k_assign_words_cells<true>, d.fine);
      hipLaunchKernelGGL(k_merge_probes, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, (const int32_t *)d.fine, n, used, (int32_t *)d_out);
      return;
   }
   launch(k_assign_words_cells<false>, (int32_t *)d_out);
}

// the context's assignment with a layer set: slices of at most 2^24 entries (what the scratch is ever sized for; P' = min(probes, C)
// entries per key, so floor(2^24 / P') keys), each through the three steps; the results are per key, so the cut is invisible.  With
// profiling on, four events per slice for hesaff_get_assign_cells_ms.  With P' = 1 the launches and the scratch are those of a
// context that never heard of probes.
void launch_assign_cells(hesaff_ctx *c, const void *d_desc, long long n, long long stride, long long offset, void *d_out)
{
   hesaff_ctx::Cells &cl = c->cells;
   cl.timed_slices = 0;
   const int used = cells_probes_used(cl.probes, cl.c);
   const int64_t slice = cells_probe_slice_keys(used);
   cl.cap = std::max<int64_t>(cl.cap, std::min<int64_t>(n, slice));
   StagePlan p;
   const ProbeScratch s = probe_scratch(p, std::min<int64_t>(cl.cap, slice), cl.c, used);
   cl.scratch.ensure(p.bytes());   // (grows with the keys, the probes and the cells of a later layer; never shrinks)
   CellsDevice d = cells_device(cl.layer.p, cl.a, cl.c, cl.scratch.p, s.s);
   d.fine = used > 1 ? cl.scratch.at<int32_t>(s.fine.off) : nullptr;
   const bool timed = c->profiling >= 1;
   const int64_t slices = cells_slice_count(n, slice);
   if (timed) while ((int64_t)cl.ev.size() < 4 * slices) cl.ev.emplace_back(hipEventDefault);
   hipStream_t st = c->stream();
   for (int64_t i = 0; i < slices; i++) {
      const int64_t begin = cells_slice_begin(i, slice);
      const int m = (int)cells_slice_keys(i, n, slice);
      const uint8_t *desc = (const uint8_t *)d_desc + begin * stride;
      const DevEvent *ev = timed ? &cl.ev[(size_t)(4 * i)] : nullptr;
      if (ev) HIP_TRY(hipEventRecord(ev[0], st));
      launch_cells_group(c, d, desc, m, stride, offset, ev ? ev + 1 : nullptr, used);
      launch_cells_fine(st, d, c->vocab.tiles.p, c->vocab.norms.p, desc, m, stride, offset, (int32_t *)d_out + 2 * begin, used);
      if (ev) HIP_TRY(hipEventRecord(ev[3], st));
   }
   if (timed) cl.timed_slices = (int)slices;
}

// The assignment (kernels_words.h; through the cell layer where one is set: kernels_cells.h) over n descriptors in device memory, on the
// main stream: (word, dist2) per key into d_out.  With profiling on, it is bracketed for hesaff_get_assign_ms.
void launch_assign_words(hesaff_ctx *c, const void *d_desc, long long n, long long stride, long long offset, void *d_out)
{
   c->assign_timed = false;
   c->cells.timed_slices = 0;
   if (n <= 0) return;
   hipStream_t st = c->stream();
   const bool timed = c->profiling >= 1;
   if (timed && !c->ev_assign[0]) { c->ev_assign[0] = DevEvent(hipEventDefault); c->ev_assign[1] = DevEvent(hipEventDefault); }
   if (timed) HIP_TRY(hipEventRecord(c->ev_assign[0], st));
   if (c->cells.c > 0) launch_assign_cells(c, d_desc, n, stride, offset, d_out);
   else if (c->neighbours > 1) {   // (never beside a layer: the setters refuse the pair)
      c->b_neigh.ensure_grow((size_t)n * (size_t)c->neighbours * 8);
      launch_neighbours_kernel(st, c->vocab.tiles.p, c->vocab.norms.p, c->vocab.n_tiles, d_desc, n, stride, offset, c->neighbours, c->b_neigh.p, d_out);
      c->neigh_device_total = n;
      c->neigh_device_r = c->neighbours;
   }
   else launch_assign_kernel(st, c->vocab.tiles.p, c->vocab.norms.p, c->vocab.n_tiles, d_desc, n, stride, offset, d_out);
   if (timed) { HIP_TRY(hipEventRecord(c->ev_assign[1], st)); c->assign_timed = true; }
}

// hesaff_assign_neighbours_device / hesaff_stage_assign_neighbours: the context's R least (dist2, row) of n descriptors in device
// memory into the caller's d_out [n][R][2], on the main stream; R = 1 as well.  Bracketed for hesaff_get_assign_ms like the assignment.
void launch_assign_neighbours(hesaff_ctx *c, const void *d_desc, long long n, long long stride, long long offset, void *d_out)
{
   c->assign_timed = false;
   c->cells.timed_slices = 0;
   if (n <= 0) return;
   hipStream_t st = c->stream();
   const bool timed = c->profiling >= 1;
   if (timed && !c->ev_assign[0]) { c->ev_assign[0] = DevEvent(hipEventDefault); c->ev_assign[1] = DevEvent(hipEventDefault); }
   if (timed) HIP_TRY(hipEventRecord(c->ev_assign[0], st));
   launch_neighbours_kernel(st, c->vocab.tiles.p, c->vocab.norms.p, c->vocab.n_tiles, d_desc, n, stride, offset, c->neighbours, d_out, nullptr);
   if (timed) { HIP_TRY(hipEventRecord(c->ev_assign[1], st)); c->assign_timed = true; }
}

// k_embed_keys against a packed projection (the context's, or the private one of a threshold training), n >= 1, on stream st
template <bool RAW>
void launch_embed_kernel(hipStream_t st, const void *tiles, const int32_t *bias, const int32_t *tau, const void *d_desc, long long n, long long stride,
                         long long offset, const int32_t *d_words, int word_stride, void *d_out)
{
   const long long blocks = (n + HS_EMBED_BLOCK_WAVES * HS_EMBED_WAVE_KEYS - 1) / (HS_EMBED_BLOCK_WAVES * HS_EMBED_WAVE_KEYS);
   hipLaunchKernelGGL(k_embed_keys<RAW>, dim3((uint32_t)blocks), dim3(HS_EMBED_BLOCK_WAVES * 64), 0, st, (const uint8_t *)d_desc, n, stride, offset, d_words,
                      word_stride, (const hs_v4i *)tiles, bias, tau, d_out);
}

// The signatures (kernels_embed.h) of n descriptors in device memory whose words - by the flat assignment, through cells or through
// probes: the word alone selects the thresholds - are at d_words, on the main stream: a uint64 per key into d_out.  With profiling
// on, it is bracketed for hesaff_get_embedding_ms.
void launch_embed_keys(hesaff_ctx *c, const void *d_desc, long long n, long long stride, long long offset, const int32_t *d_words, int word_stride, void *d_out)
{
   c->embed_timed = false;
   if (n <= 0) return;
   hipStream_t st = c->stream();
   const bool timed = c->profiling >= 1;
   if (timed && !c->ev_embed[0]) { c->ev_embed[0] = DevEvent(hipEventDefault); c->ev_embed[1] = DevEvent(hipEventDefault); }
   if (timed) HIP_TRY(hipEventRecord(c->ev_embed[0], st));
   launch_embed_kernel<false>(st, c->embed.ptr(c->embed.a.tiles), c->embed.ptr(c->embed.a.bias), c->embed.ptr(c->embed.a.tau), d_desc, n, stride, offset, d_words,
                              word_stride, d_out);
   if (timed) { HIP_TRY(hipEventRecord(c->ev_embed[1], st)); c->embed_timed = true; }
}

// the words of a batch's ordered records (b_out), behind the pack stage: b_words row for row; with an embedding set, b_sigs behind them
void assign_batch_words(hesaff_ctx *c, long long total)
{
   c->assign_timed = false;
   c->embed_timed = false;
   if (c->vocab.k == 0 || total <= 0) return;
   c->b_words.ensure_grow((size_t)total * 8);
   launch_assign_words(c, c->geo.b_out.p, total, (long long)sizeof(KeyRec), (long long)offsetof(KeyRec, desc), c->b_words.p);
   if (!c->embed.set) return;
   c->b_sigs.ensure_grow((size_t)total * 8);
   launch_embed_keys(c, c->geo.b_out.p, total, (long long)sizeof(KeyRec), (long long)offsetof(KeyRec, desc), c->b_words.as<int32_t>(), 2, c->b_sigs.p);
}

// hesaff_process_files with an embedding and R > 1: behind assign_batch_words, the signature of every (key, rank) of the batch's `total`
// records for the ranks 1 .. min(R, K) - 1 - the ranks every key has; rank 0 is b_sigs - into b_nsigs, plane r - 1 = rank r.  The
// neighbours array is a words array of stride 2 R that starts at rank r (k_embed_keys reads the word alone).
void embed_batch_ranks(hesaff_ctx *c, long long total)
{
   if (total <= 0 || !c->embed.set || c->neighbours < 2) return;
   const int R = c->neighbours, ranks = std::min(R, c->vocab.k);
   c->b_nsigs.ensure_grow((size_t)total * 8 * (size_t)(R - 1));
   for (int r = 1; r < ranks; r++)
      launch_embed_kernel<false>(c->stream(), c->embed.ptr(c->embed.a.tiles), c->embed.ptr(c->embed.a.bias), c->embed.ptr(c->embed.a.tau), c->geo.b_out.p, total,
                                 (long long)sizeof(KeyRec), (long long)offsetof(KeyRec, desc), c->b_neigh.as<int32_t>() + 2 * r, 2 * R,
                                 c->b_nsigs.at<uint64_t>((size_t)(r - 1) * (size_t)total * 8));
}

// Everything after the Hessian list of a batch is complete - by detection (run_batch) or from the caller's records (run_describe):
// affine shape, patches and descriptors over image groups in the order of group_schedule.h, the stable compaction into KeyRec records,
// the descriptor starts, and the wait for the end of the batch.  hs: fetch_hessian_starts' block.  with_affine = false: the affine
// output is already in place (HESAFF_FROM_SHAPES), k_affine is not launched.  The affine stream starts behind ev_detect_done,
// which the caller has recorded after the last kernel that writes a plane k_affine reads.
BatchResult run_keypoint_stages(hesaff_ctx *c, const Lists &s, StageTimer &tm, int tt, int B, int H, int W, const int32_t *hs, bool with_affine)
{
   hipStream_t st = c->stream();
   CounterBlock *cnt = s.counters;
   int t;
   PlaneTab pt;
   memset(&pt, 0, sizeof pt);
   uint32_t n_hess_host = 0;   // Hessian keypoints of the batch
   const int K = ori_count(c);
   for (size_t o = 0; o < c->oct.size(); o++)
      for (int l = 0; l < 3; l++) pt.L[o][l] = c->L[o * 3 + l];
   {
      // The bin kernels only extract the 41x41 patches (to HBM); the descriptor runs as three kernels with the parallel axis each
      // part wants (kernels_sift.h).  Images are processed in groups so that the patch buffers stay bounded.
      if ((uint32_t)hs[B] > c->cap) throw HsError(HESAFF_ERR_CAPACITY, "keypoint capacity exceeded; raise hesaff_params.max_kpts_per_mpx");
      n_hess_host = (uint32_t)hs[B];
      const StartsBlock<const uint32_t> hb = starts_block((const uint32_t *)hs, B);
      c->batch_max_p = (int)*hb.largest_window();   // largest huge window of the batch (0: none)
      // image groups [lo, hi) of keypoints; the T' rows of a group's huge windows fit the row buffer (form_groups, batch_plan.h)
      const GroupPlan gp = form_groups(hs, hb.large_rows(), B, c->trows_rows);
      if (gp.max_n) ensure_group_buffers(c, gp.max_n);
      const sched::ScheduleOptions so = {!c->no_overlap, c->sift_inside, with_affine, patch_side_streams(c, &pt), c->orientation == HESAFF_ORI_DOMINANT, K};
      if (K > 1) ensure_rank_arrays(c, K);
      GroupDevice dev(c, s, tm, gp.groups, pt, H, W, rank_arrays(c, K));   // (K = 1: no rank above 0, nothing allocated, nothing of it read)
      sched::run_group_schedule(dev, (int)gp.groups.size(), so);
   }
   t = tm.begin(T_PACK);
   // final stable compaction (hesaff.cpp:87: keys.push_back in detection order): exclusive scan of the alive flags of the batch's
   // Hessian keypoints (alive[] is rewritten for h < n_hess each batch; the host knows n_hess since the round trip after detection -
   // the scan used to run over the whole capacity, 85 M flags for 31 M keypoints, behind a kernel that cleared the tail)
   if (K > 1) {
      // an orientation count: a region owns as many adjacent rows as it has keys, so the scan runs over keys per region; the rows may
      // outnumber the capacity b_out is sized for - k_pack_peaks clamps its writes, the host refuses the batch below
      const OrientRanks mr = rank_arrays(c, K);
      LoadKeyCount lk; lk.p = s.pw.alive; lk.ranks = mr.alive; lk.cap = mr.cap; lk.K = K;
      exclusive_scan(c, lk, (long long)n_hess_host, c->geo.b_rank.as<uint32_t>(), &cnt->head.desc_total);
      hipLaunchKernelGGL(k_pack_peaks, dim3(HS_GRID_PACK), dim3(256), 0, st, s.hl, (const uint32_t *)&cnt->head.hess_total, s.pw, mr, (const uint32_t *)c->geo.b_rank.p,
                         (const uint8_t *)c->geo.b_desc.p, c->geo.b_out.as<KeyRec>(), c->cap);
   } else {
      LoadFlagI32 lf; lf.p = s.pw.alive;
      exclusive_scan(c, lf, (long long)n_hess_host, c->geo.b_rank.as<uint32_t>(), &cnt->head.desc_total);
      hipLaunchKernelGGL(k_pack, dim3(HS_GRID_PACK), dim3(256), 0, st, s.hl, (const uint32_t *)&cnt->head.hess_total, s.pw, (const uint32_t *)c->geo.b_rank.p,
                         (const uint8_t *)c->geo.b_desc.p, c->geo.b_out.as<KeyRec>());
   }
   const StartsBlock<int32_t> d_starts = starts_block(c->geo.b_starts.as<int32_t>(), B);
   hipLaunchKernelGGL(k_desc_starts, dim3((B + 1 + 63) / 64), dim3(64), 0, st, (const int32_t *)d_starts.hess(), B,
                      (const uint32_t *)c->geo.b_rank.p, (const uint32_t *)&cnt->head.hess_total, (const uint32_t *)&cnt->head.desc_total,
                      d_starts.desc());
   tm.end(t);
   tm.end(tt);
   // Hessian starts [B + 1], descriptor starts [B + 1], and behind them the head of the counter block
   const size_t final_words = d_starts.words_final();
   int32_t *h_starts = (int32_t *)c->h_small_end.ensure_small(final_words * 4 + sizeof(CounterHead));
   HIP_TRY(hipMemcpyAsync(h_starts, c->geo.b_starts.p, final_words * 4, hipMemcpyDeviceToHost, st));
   HIP_TRY(hipMemcpyAsync(h_starts + final_words, &cnt->head, sizeof(CounterHead), hipMemcpyDeviceToHost, st));
   HIP_TRY(hipEventRecord(c->ev_batch_done, st));
   const double dbg_cb = c->debug ? thread_cpu_ms() : 0.0;
   hs_wait_event(c->ev_batch_done);
   if (c->debug) fprintf(stderr, "[hesaff] run_batch: caller's CPU inside the wait for the end of the batch %.2f ms\n", thread_cpu_ms() - dbg_cb);
   HIP_TRY(hipGetLastError());
   if (c->profiling) collect_timings(c, tm, B);
   const CounterHead *cn = (const CounterHead *)(h_starts + final_words);
   if (cn->overflow != 0 || cn->rec > c->cap)
      throw HsError(HESAFF_ERR_CAPACITY, "keypoint capacity exceeded; raise hesaff_params.max_kpts_per_mpx");
   if (cn->row_overflow != 0) throw HsError(HESAFF_ERR_NOMEM, "large-window row buffer exceeded (internal bound violated)");
   if (K > 1 && cn->desc_total > c->cap)
      throw HsError(HESAFF_ERR_CAPACITY, "the keys of the orientation count exceed the keypoint capacity; raise hesaff_params.max_kpts_per_mpx");
   const StartsBlock<const int32_t> h = starts_block((const int32_t *)h_starts, B);
   assign_batch_words(c, (long long)h.desc()[B]);   // (nothing without a vocabulary)
   return {h.hess(), h.desc(), d_starts.desc()};
}

// hesaff_set_keypoint_limit and hesaff_set_next_masks (kernels_select.h): of the ordered Hessian list run_detection left, every image
// keeps its eligible keypoints - those on a non-zero pixel of its mask, all without one - or the keypoint_limit strongest of them, in
// their order, and the list, its length, the per-image starts and the large-window row bounds become those of the kept keypoints -
// everything behind sees a shorter list.  Only run_batch calls it: the stage operators and run_describe
// neither limit nor mask.  The ranks live in b_rank (free until the pack stage's scan), the kept counts in the descriptor starts
// (written at the end of the batch), the ordered items are still in b_cand, the length detection found stays in the counter block:
// no buffer of its own, nothing allocated.
// With hesaff_set_keypoint_grid (more than one cell, and a limit) k_select_image_grid takes k_select_image's place: the limit's N /
// cells strongest eligible keypoints of every cell of the grid over the H x W image as the caller passed it.
void select_keypoints(hesaff_ctx *c, const Lists &s, StageTimer &tm, int B, int H, int W, const SelMasks &mk)
{
   hipStream_t st = c->stream();
   CounterBlock *cnt = s.counters;
   const uint32_t limit = c->keypoint_limit > 0 ? (uint32_t)c->keypoint_limit : HS_SEL_NO_LIMIT;
   const StartsBlock<int32_t> sb = starts_block(c->geo.b_starts.as<int32_t>(), B);
   int32_t *starts = sb.hess();
   uint32_t *kept = (uint32_t *)sb.desc();
   uint32_t *keep_rank = c->geo.b_rank.as<uint32_t>();
   const int t = tm.begin(T_DET);
   const int cells = c->grid_rows * c->grid_cols;
   if (c->keypoint_limit > 0 && cells > 1)   // (the setters keep keypoint_limit >= cells: the quota is at least 1)
      hipLaunchKernelGGL(k_select_image_grid, dim3(B), dim3(HS_SEL_THREADS), 0, st, (const float *)s.hl.response, (const float *)s.hl.x,
                         (const float *)s.hl.y, (const int32_t *)starts, (const uint32_t *)&cnt->head.hess_total, s.hl.cap, limit / (uint32_t)cells,
                         c->grid_rows, c->grid_cols, W, H, mk, keep_rank, kept);
   else
      hipLaunchKernelGGL(k_select_image, dim3(B), dim3(HS_SEL_THREADS), 0, st, (const float *)s.hl.response, (const float *)s.hl.x, (const float *)s.hl.y,
                         (const int32_t *)starts, (const uint32_t *)&cnt->head.hess_total, s.hl.cap, limit, mk, keep_rank, kept);
   hipLaunchKernelGGL(k_select_starts, dim3(1), dim3(256), 0, st, starts, B, (const uint32_t *)kept, s.hl.cap, &cnt->head.hess_total, &cnt->head.hess_detected);
   hipLaunchKernelGGL(k_hess_deal_kept, dim3(HS_GRID_SCAT), dim3(256), 0, st, (const HessItem *)c->geo.b_cand.p, (const uint32_t *)&cnt->head.hess_detected,
                      (const uint32_t *)keep_rank, (const int32_t *)starts, s.hl);
   launch_image_large_rows(c, s, B);   // the bounds form_groups reads describe the kept keypoints
   tm.end(t);
}

// Whole hot path on a device-resident batch.  Leaves ordered KeyRec records in b_out and
// per-image start offsets (b_starts: StartsBlock::hess() and desc(); BatchResult: their host copies).
// mk: the batch's detection masks (base null: none), H x W like the images.
BatchResult run_batch(hesaff_ctx *c, const SrcImages &src, int B, int H, int W, const SelMasks &mk = SelMasks())
{
   plan(c, B, H, W);
   c->ev_used = 0;
   StageTimer tm(c);
   Lists s = make_lists(c);
   const int tt = tm.begin(T_TOTAL);
   run_detection(c, src, B, s, tm);
   if (c->keypoint_limit > 0 || mk.base) select_keypoints(c, s, tm, B, H, W, mk);
   // the one host round trip of a batch
   return run_keypoint_stages(c, s, tm, tt, B, H, W, fetch_hessian_starts(c, B), true);
}

// hesaff_describe_regions on a device-resident chunk: the caller's records take the place of detection's list.  d_block (device,
// 256-byte aligned): B + 1 record starts (int32, image b owns records starts[b] .. starts[b + 1]), then - describe_records_offset(B)
// bytes in - the chunk's hesaff_region records, already checked by the host (describe_bad_record).  n_rec = starts[B].
// from = HESAFF_FROM_POINTS: the blur planes as detection builds them (which also yields the grey plane), then k_affine over the list.
// from = HESAFF_FROM_SHAPES: the grey plane alone (parity mode) - fast mode 2 builds the scale space too, k_patch_pyramid samples it -
// and the affine output from the records.  Leaves what run_batch leaves.
BatchResult run_describe(hesaff_ctx *c, const SrcImages &src, int B, int H, int W, const uint8_t *d_block, uint32_t n_rec, int from)
{
   plan(c, B, H, W);
   if (n_rec > c->cap) throw HsError(HESAFF_ERR_CAPACITY, "more records than the keypoint capacity; raise hesaff_params.max_kpts_per_mpx");
   c->ev_used = 0;
   StageTimer tm(c);
   Lists s = make_lists(c);
   hipStream_t st = c->stream();
   CounterBlock *cnt = s.counters;
   const bool shapes = from == HESAFF_FROM_SHAPES;
   const int tt = tm.begin(T_TOTAL);
   HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(CounterBlock), st));
   hipLaunchKernelGGL(k_ingest_regions, dim3(std::max<uint32_t>(1u, std::min<uint32_t>((std::max<uint32_t>(n_rec, (uint32_t)B + 1) + 255) / 256, 4096u))), dim3(256), 0, st,
                      (const uint4 *)(d_block + describe_records_offset(B)), n_rec, (const int32_t *)d_block, B, shapes ? 1 : 0, s.hl, s.ao,
                      &cnt->head.hess_total, c->geo.b_starts.as<int32_t>());
   launch_image_large_rows(c, s, B);
   // (the per-image counts are the caller's, but the row bounds are the device's: the round trip stays, behind two short kernels;
   //  the planes below are enqueued after it and run while the groups are formed)
   const int32_t *hs = fetch_hessian_starts(c, B);
   if (!shapes || c->fast_pyramid) {
      // the grey plane and every level findAffineShape can be asked to run on (L0..L2 of each octave): no response plane, no detection
      build_first_level(c, src, B, tm);
      for (size_t o = 0; o < c->oct.size(); o++) build_octave(c, o, B, octave_planes(c, o, B), OctaveWant::BlursOnly, tm);
   } else {
      launch_gray_plane(c, src, B);
   }
   HIP_TRY(hipEventRecord(c->ev_detect_done, st));   // the affine stream starts behind the planes
   return run_keypoint_stages(c, s, tm, tt, B, H, W, hs, !shapes);
}

// ---- exportKeypoints on the device (kernels_export.h) ----
// Lengths of the n rows of `keys`, their 64-row offsets, and the byte offset of every image's first row (d_starts: B + 1 row
// starts on the device).  The host waits for the stream here: it needs the byte counts to size the copy out.
unsigned long long export_text_prepare(hesaff_ctx *c, const KeyRec *keys, uint32_t n, const int32_t *d_starts, int B,
                                       std::vector<unsigned long long> &img_off)
{
   img_off.assign((size_t)B + 1, 0ull);
   if (n == 0) return 0ull;
   hipStream_t st = c->stream();
   const uint32_t nblk = (n + EX_ROWS - 1) / EX_ROWS;
   c->b_ex_len.ensure_grow(((size_t)n + 64) * 2);
   c->b_ex_sums.ensure_grow((size_t)nblk * 4);
   c->b_ex_off.ensure_grow(((size_t)nblk + 1) * 8);
   c->b_ex_imgoff.ensure(((size_t)B + 1) * 8);
   hipLaunchKernelGGL(k_text_len, dim3((n + 255) / 256), dim3(256), 0, st, keys, n, c->par.mrSize, c->b_ex_len.as<uint16_t>(), c->b_ex_sums.as<uint32_t>());
   hipLaunchKernelGGL(k_text_scan, dim3(1), dim3(1024), 0, st, (const uint32_t *)c->b_ex_sums.p, nblk, c->b_ex_off.as<unsigned long long>());
   hipLaunchKernelGGL(k_text_imgoff, dim3((B + 1 + 63) / 64), dim3(64), 0, st, d_starts, B, (const uint16_t *)c->b_ex_len.p,
                      (const unsigned long long *)c->b_ex_off.p, c->b_ex_imgoff.as<unsigned long long>());
   // into pinned memory, then a sleep on the blocking-sync event (a copy into the pageable vector would spin in the runtime)
   unsigned long long *ho = (unsigned long long *)c->h_small_exp.ensure_small(((size_t)B + 1) * 8);
   HIP_TRY(hipMemcpyAsync(ho, c->b_ex_imgoff.p, ((size_t)B + 1) * 8, hipMemcpyDeviceToHost, st));
   HIP_TRY(hipEventRecord(c->ev_batch_done, st));      // (run_batch has returned: the event is free)
   hs_wait_event(c->ev_batch_done);
   HIP_TRY(hipGetLastError());
   memcpy(img_off.data(), ho, ((size_t)B + 1) * 8);
   return img_off[(size_t)B];
}

// ... and the rows themselves into d_text (export_text_prepare's byte count), on the main stream
void export_text_write(hesaff_ctx *c, const KeyRec *keys, uint32_t n, char *d_text)
{
   if (n == 0) return;
   hipLaunchKernelGGL(k_text_write, dim3((n + EX_ROWS - 1) / EX_ROWS), dim3(EX_ROWS), 0, c->stream(), keys, n, c->par.mrSize, (const uint16_t *)c->b_ex_len.p,
                      (const unsigned long long *)c->b_ex_off.p, d_text);
}

// hesaff_jpeg_layout (what the host's entropy stage reports; from a caller, so checked) -> the kernels' geometry
JpegGeom make_jpeg_geom(const hesaff_jpeg_layout &L)
{
   JpegGeom g;
   if (!hesaff_plan::make_jpeg_geom(L, g)) throw HsError(HESAFF_ERR_ARG, "bad JPEG layout");   // jpeg_plan.h
   return g;
}

// coefficient blobs of B images of one layout (device) -> their pixels, W x H x channels bytes each, out_img_stride apart
void jpeg_pixels(hesaff_ctx *c, const uint8_t *d_blobs, const JpegGeom &g, int B, uint8_t *d_out, size_t out_img_stride, hipStream_t st)
{
   if (B < 1) return;
   c->b_jplane.ensure_grow((size_t)g.plane_bytes * (size_t)B);
   const unsigned long long total = (unsigned long long)B * g.blocks_per_image;
   hipLaunchKernelGGL(k_jpeg_idct, dim3((unsigned)std::min<unsigned long long>((total + 255) / 256, 1u << 20)), dim3(256), 0, st, d_blobs,
                      c->b_jplane.as<uint8_t>(), g, B);
   hipLaunchKernelGGL(k_jpeg_pixels, dim3(((g.W + 3) / 4 + 255) / 256, g.H, B), dim3(256), 0, st, d_blobs, (const uint8_t *)c->b_jplane.as<uint8_t>(), d_out, g,
                      (unsigned long long)out_img_stride);
}

void export_bin_rows(hesaff_ctx *c, const KeyRec *keys, uint32_t n, char *d_bin)
{
   if (n == 0) return;
   hipLaunchKernelGGL(k_bin_rows, dim3(std::min<uint32_t>((n + 7) / 8, 4096u)), dim3(256), 0, c->stream(), keys, n, c->par.mrSize, (uint32_t *)d_bin);
}

// hesaff_detect_regions: the n_hess hesaff_region records of the batch run_batch just finished into d_regions, on the main stream
// (the Hessian list, the affine output, the alive flags, rank[] and the descriptor starts stay valid there until the next batch)
void pack_regions(hesaff_ctx *c, uint32_t n_hess, int B, hesaff_region *d_regions)
{
   static_assert(sizeof(hesaff_region) == 4 * HS_REGION_DW, "hesaff_region layout");
   if (n_hess == 0) return;
   if (n_hess > c->cap) throw HsError(HESAFF_ERR_CAPACITY, "keypoint capacity exceeded; raise hesaff_params.max_kpts_per_mpx");
   const Lists s = make_lists(c);
   RegionTab tab;
   for (int o = 0; o < HS_MAX_OCTAVES; o++) tab.pd[o] = c->ct.consts.pd0 * (float)(1 << o);   // pyramid.cpp:288, as run_detection hands it on
   const dim3 grid(std::min<uint32_t>((n_hess + 255) / 256, 4096u));
   const int32_t *desc_starts = starts_block(c->geo.b_starts.as<int32_t>(), B).desc();
   if (ori_count(c) > 1)
      hipLaunchKernelGGL(k_pack_regions_peaks, grid, dim3(256), 0, c->stream(), s.hl, n_hess, s.ao, s.pw, rank_arrays(c, ori_count(c)),
                         (const uint32_t *)c->geo.b_rank.p, desc_starts, tab, (uint4 *)d_regions);
   else
      hipLaunchKernelGGL(k_pack_regions, grid, dim3(256), 0, c->stream(), s.hl, n_hess, s.ao, s.pw, (const uint32_t *)c->geo.b_rank.p, desc_starts, tab,
                         (uint4 *)d_regions);
}

} // namespace
#include "capi_impl.h"
#include "capi_stage.h"
#include "capi_train.h"
#include "capi_cells.h"
#include "capi_index.h"
#include "capi_verify.h"
#include "capi_expand.h"
#include "capi_embed.h"
#include "capi_index_grow.h"
#include "capi_index_remove.h"
#include "capi_index_batch.h"
