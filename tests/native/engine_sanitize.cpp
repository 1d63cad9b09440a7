// Sanitizer driver for the host-only half of the chunk engine (test infrastructure; built by tests/test_host_sanitize.py with
// g++ -fsanitize=thread and -fsanitize=address,undefined from hesaff_amd/csrc/chunk_engine.h + hostio.cpp + jpeg_decode.cpp).
// It runs the product's own chunk loop (run_chunk_loop, chunk_engine.h) - the staging thread that calls ChunkIO::next / staged one
// chunk ahead, the caller's thread that computes a chunk, delivers the previous one and takes a result block, the refusal rule and
// the error path - and replaces only the object the loop drives: MockDevice stands where capi_impl.h's ChunkDevice makes the HIP
// calls.  It fabricates records from the pixels it was handed (so every decoded byte is read while the engine says it is alive, and
// every record is read by a consumer while its block is marked busy).
//   engine_sanitize <max_batch> <decode_threads> <write_threads> <format> <file>...      FileIO in a ring of three blocks, format:
//                   + 4: the mock hands over rows that are already text / packed - ChunkDone::text, text_off, bin - like the device
//                        formatter of kernels_export.h
//                   + 8: JPEG files arrive as coefficient blobs from the pool of recycled blobs, like hesaff_process_files
//                   + 16: the readers fill (mock) page-locked buffers of the context (PinHooks)
//                   + 32: the device refuses (HESAFF_ERR_CAPACITY) every chunk with an image whose index i has i % 11 == 3
//                   + 64: the device fails (HESAFF_ERR_DEVICE) on its third chunk; exit code 0 only when the error came through
//   engine_sanitize array <max_batch> <n_images> [refuse]     ArrayIO: hesaff_detect_batch_cb's chunk source (a sink called per chunk
//                   with records that live in a ring block, the sink's return code read by the staging thread; the sink fails on the
//                   last third of a second run) and hesaff_detect_batch's (no ring: block k for chunk k, results filled in place and
//                   read after the call).  refuse: the refusal of format + 32, which fails an array call as a whole
// prints "chunks=<images per chunk, ...>" and "files=<n> written=<w> unreadable=<u> other=<o> rows=<r>"; exit code 0 unless the pipeline misbehaved.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "../../hesaff_amd/csrc/chunk_engine.h"

using namespace hesaff_engine;

static const float kMrSize = 5.196152f;

// mock of hesaff_ctx::PinReadCache: a budget of a few buffers, so that lists mix chunks of "pinned" and ordinary images; every buffer must
// come back (release) before the run ends, and a chunk may only call itself pinned when all its images are
struct MockPin {
   std::mutex mu;
   std::unordered_map<void *, size_t> out;
   size_t budget = 40000, given = 0, returned = 0;
   static void *alloc(size_t bytes, void *user)
   {
      MockPin *m = (MockPin *)user;
      std::lock_guard<std::mutex> lk(m->mu);
      size_t live = 0;
      for (auto &e : m->out) live += e.second;
      if (live + bytes > m->budget) return nullptr;
      void *q = malloc(bytes);
      if (q) { m->out[q] = bytes; m->given++; }
      return q;
   }
   static void release(void *q, size_t bytes, void *user)
   {
      MockPin *m = (MockPin *)user;
      std::lock_guard<std::mutex> lk(m->mu);
      auto it = m->out.find(q);
      if (it == m->out.end() || it->second != bytes) { fprintf(stderr, "release of a buffer that is not out\n"); abort(); }
      m->out.erase(it); m->returned++;
      free(q);
   }
};

struct MockState : ChunkState {
   std::vector<uint32_t> sum;   // per image: a hash of its staged bytes
};

struct MockDevice {
   using State = MockState;
   int wants = WANT_KEYS;
   bool count_by_index = false;   // rows of an image from its index (what the array runs check their sums against), else from its bytes
   MockPin *pin = nullptr;        // the hooks of the run, if any: where the images of a pinned chunk must come from
   bool refuse = false, fail_third = false;
   std::vector<std::vector<char>> blocks;   // the result blocks: the ring's, or (no ring) one per chunk
   long long rows = 0;
   std::string chunk_sizes;
   int pinned_chunks = 0, computed = 0, drained = 0;

   // "copy to pinned memory": read every byte of every image of the chunk
   void stage(State &s)
   {
      if (s.q.pinned) {
         if (!pin) { fprintf(stderr, "pinned chunk without hooks\n"); abort(); }
         std::lock_guard<std::mutex> lk(pin->mu);
         for (const uint8_t *d : s.q.data) if (!pin->out.count((void *)d)) { fprintf(stderr, "pinned chunk holds an ordinary buffer\n"); abort(); }
         pinned_chunks++;
      }
      for (size_t b = 0; b < s.q.data.size(); b++) {
         uint32_t acc = 0;
         const size_t bytes = s.q.blob_bytes ? s.q.blob_bytes : (size_t)s.q.W * s.q.H * s.q.ch;   // a JPEG file's coefficient blob (recycled by the pool afterwards)
         for (size_t k = 0; k < bytes; k++) acc = acc * 31u + s.q.data[b][k];
         s.sum.push_back(acc);
      }
   }
   void compute(State &s)
   {
      const size_t B = s.q.data.size();
      if (++computed == 3 && fail_third) throw HsError(HESAFF_ERR_DEVICE, "mock device: lost on the third chunk");
      if (refuse)
         for (int i : s.q.index)
            if (i % 11 == 3) throw HsError(HESAFF_ERR_CAPACITY, "mock device: chunk refused");
      chunk_sizes += (chunk_sizes.empty() ? "" : ",") + std::to_string(B);
      for (size_t b = 0; b < B; b++) {
         const int cnt = count_by_index ? (s.q.index[b] * 37) % 200 : (int)(s.sum[b] % 700u);     // rows of this image, 0 included
         s.nh.push_back(cnt + 3); s.nd.push_back(cnt); s.off.push_back((size_t)s.total);
         s.total += cnt;
      }
      rows += s.total;
   }
   // records, text and sidecar rows of the chunk into a fresh block s.block: a consumer still reading the old one would be a race / use after free
   void copy_out(State &s)
   {
      const size_t B = s.q.data.size();
      std::vector<hesaff_keypoint> keys((size_t)s.total);
      size_t o = 0;
      for (size_t b = 0; b < B; b++)
         for (int r = 0; r < s.nd[b]; r++, o++) {
            hesaff_keypoint &k = keys[o];
            k.x = (float)(s.sum[b] % 1000u) + (float)r; k.y = (float)r * 0.5f; k.s = 2.0f + (float)(r % 7);
            k.a11 = 1.25f; k.a12 = 0.0f; k.a21 = 0.1f; k.a22 = 0.8f; k.response = 30.0f; k.type = r & 1;
            for (int j = 0; j < 128; j++) k.desc[j] = (uint8_t)(s.sum[b] + (uint32_t)(r * 131 + j));
         }
      // the "device formatter": every image's rows through the host formatter, headers cut off, back to back
      std::vector<char> text;
      if (wants & WANT_TEXT) {
         s.toff.assign(B + 1, 0ull);
         for (size_t b = 0; b < B; b++) {
            char *txt = nullptr; size_t len = 0;
            if (hesaff_format_sift(keys.data() + s.off[b], s.nd[b], kMrSize, &txt, &len) != HESAFF_OK) throw HsError(HESAFF_ERR_NOMEM, "mock device: formatter failed");
            size_t skip = 0;
            for (int nl = 0; nl < 2; skip++) if (txt[skip] == '\n') nl++;
            s.toff[b] = text.size();
            text.insert(text.end(), txt + skip, txt + len);
            hesaff_free(txt);
         }
         s.toff[B] = text.size();
      }
      // the block's layout, as capi_impl.h lays it out: [records][text rows][sidecar rows], what the consumer wants of them
      size_t at = 0;
      auto place = [&at](size_t bytes) { const size_t p = at; at = (at + bytes + 255) & ~(size_t)255; return p; };
      if (wants & WANT_KEYS) s.keys_at = place(keys.size() * sizeof(hesaff_keypoint));
      if (wants & WANT_TEXT) s.text_at = place(text.size());
      if (wants & WANT_BIN) s.bin_at = place(keys.size() * 148);
      s.bytes = at;
      std::vector<char> blk(at + 1);
      if ((wants & WANT_KEYS) && !keys.empty()) memcpy(blk.data() + s.keys_at, keys.data(), keys.size() * sizeof(hesaff_keypoint));
      if ((wants & WANT_TEXT) && !text.empty()) memcpy(blk.data() + s.text_at, text.data(), text.size());
      if (wants & WANT_BIN)
         for (size_t r = 0; r < keys.size(); r++) {
            const hesaff_keypoint &k = keys[r];
            float v[5] = {k.x, k.y, 0, 0, 0};
            hesaff_ellipse(&k, kMrSize, &v[2], &v[3], &v[4]);
            memcpy(blk.data() + s.bin_at + r * 148, v, 20);
            memcpy(blk.data() + s.bin_at + r * 148 + 20, k.desc, 128);
         }
      if ((int)blocks.size() <= s.block) blocks.resize((size_t)s.block + 1);   // no ring: a block per chunk, kept until the call is over
      blocks[(size_t)s.block] = std::move(blk);
      s.copied = true;
   }
   const char *wait_out(State &s) { return blocks[(size_t)s.block].data(); }
   void drain() { drained++; }
   void finish() {}
};

struct SinkState { long long rows = 0; int calls = 0; int fail_after = -1; uint32_t acc = 0; };
static int array_sink(void *user, int n_images, const int *image_index, const hesaff_result *results)
{
   SinkState *s = (SinkState *)user;
   for (int i = 0; i < n_images; i++) {
      for (int r = 0; r < results[i].count_desc; r++) s->acc = s->acc * 31u + results[i].keys[r].desc[(r + image_index[i]) & 127];   // read the block
      s->rows += results[i].count_desc;
   }
   s->calls++;
   return (s->fail_after >= 0 && s->calls > s->fail_after) ? 1 : 0;
}

// ArrayIO through the chunk loop.  ring_blocks 3: hesaff_detect_batch_cb (done -> sink -> ring release); 0: hesaff_detect_batch (results
// filled in place, every block read when the call is over).  -> the sink's return code, or the code of the error the loop threw
static int run_array(int max_batch, int n, int fail_after, int ring_blocks, bool refuse, long long *rows_out)
{
   std::vector<std::vector<uint8_t>> pix((size_t)n);
   std::vector<const uint8_t *> ptr((size_t)n);
   std::vector<int> w((size_t)n), h((size_t)n), ch((size_t)n);
   for (int i = 0; i < n; i++) {
      w[(size_t)i] = (i % 3 == 1) ? 20 : 32; h[(size_t)i] = 16; ch[(size_t)i] = (i % 5 == 4) ? 3 : 1;
      pix[(size_t)i].assign((size_t)w[(size_t)i] * h[(size_t)i] * ch[(size_t)i], (uint8_t)(i * 7));
      ptr[(size_t)i] = pix[(size_t)i].data();
   }
   BlockRing ring;
   ArrayIO io(&ring, max_batch, n, ptr.data(), w.data(), h.data(), nullptr, ch.data());
   SinkState st;
   st.fail_after = fail_after;
   std::vector<hesaff_result> results((size_t)n);
   if (ring_blocks > 0) { io.sink = array_sink; io.user = &st; }
   else io.results = results.data();
   MockDevice dev;
   dev.wants = io.wants(); dev.count_by_index = true; dev.refuse = refuse;
   dev.blocks.resize((size_t)ring_blocks);
   *rows_out = 0;
   try {
      run_chunk_loop(io, ring, ring_blocks, dev);
   } catch (const HsError &e) {
      if (dev.drained != 1) { fprintf(stderr, "the error path idled the device %d times\n", dev.drained); abort(); }
      return e.code;
   }
   if (ring_blocks == 0)
      for (int i = 0; i < n; i++) {
         for (int r = 0; r < results[(size_t)i].count_desc; r++) st.acc = st.acc * 31u + results[(size_t)i].keys[r].desc[(r + i) & 127];
         st.rows += results[(size_t)i].count_desc;
      }
   *rows_out = st.rows;
   return io.sink_rc.load();
}

int main(int argc, char **argv)
{
   if ((argc == 4 || argc == 5) && !strcmp(argv[1], "array")) {
      const int max_batch = atoi(argv[2]), n = atoi(argv[3]);
      long long rows = 0, want = 0, rows2 = 0, rows3 = 0;
      if (argc == 5) {   // a refused chunk fails the call as a whole (ArrayIO::failed is false)
         const int rc = run_array(max_batch, n, -1, 3, true, &rows), rc0 = run_array(max_batch, n, -1, 0, true, &rows3);
         printf("array images=%d refused rc=%d no_ring_rc=%d\n", n, rc, rc0);
         return (rc == HESAFF_ERR_CAPACITY && rc0 == HESAFF_ERR_CAPACITY) ? 0 : 3;
      }
      for (int i = 0; i < n; i++) want += (i * 37) % 200;
      const int rc = run_array(max_batch, n, -1, 3, false, &rows);
      const int rc2 = run_array(max_batch, n, 2, 3, false, &rows2);     // the sink reports failure on its third call: the run stops early
      const int rc3 = run_array(max_batch, n, -1, 0, false, &rows3);    // no ring
      printf("array images=%d rows=%lld want=%lld rc=%d failing_run_rc=%d rows=%lld no_ring_rc=%d rows=%lld\n", n, rows, want, rc, rc2, rows2, rc3, rows3);
      return (rc == 0 && rows == want && rc2 != 0 && rows2 < want && rc3 == 0 && rows3 == want) ? 0 : 3;
   }
   if (argc < 6) return 2;
   const int max_batch = atoi(argv[1]), dt = atoi(argv[2]), wt = atoi(argv[3]), flags = atoi(argv[4]), fmt = flags & 3;
   const bool device_format = (flags & 4) != 0, device_jpeg = (flags & 8) != 0;
   const bool mock_pin = (flags & 16) != 0;   // the context's page-locked read buffers (PinHooks), here plain malloc with a small budget
   const bool refuse = (flags & 32) != 0, fail_third = (flags & 64) != 0;
   const int n = argc - 5;
   std::vector<const char *> paths((size_t)n);
   for (int i = 0; i < n; i++) paths[(size_t)i] = argv[5 + i];
   std::vector<hesaff_file_status> status((size_t)n);
   for (auto &s : status) { s.rc = HESAFF_ERR_IO; s.stage = HESAFF_FILE_PENDING; s.count_hessian = s.count_desc = 0; }
   BlockRing ring;
   MockPin mp;
   PinHooks pin;
   if (mock_pin) { pin.user = &mp; pin.alloc = MockPin::alloc; pin.release = MockPin::release; }
   MockDevice dev;
   dev.pin = mock_pin ? &mp : nullptr; dev.refuse = refuse; dev.fail_third = fail_third;
   dev.blocks.resize(3);
   bool came_through = false;
   {
      FileIO io(&ring, max_batch, kMrSize, fmt, n, paths.data(), nullptr, status.data(), dt, wt, device_format, false, device_jpeg, pin);
      dev.wants = io.wants();
      try {   // as hesaff_process_files does
         run_chunk_loop(io, ring, 3, dev);
         io.wait_writers();
      } catch (const HsError &e) {
         io.shutdown();
         came_through = fail_third && e.code == HESAFF_ERR_DEVICE && e.msg == "mock device: lost on the third chunk" && dev.drained == 1;
         if (!came_through) { fprintf(stderr, "the chunk loop threw %d: %s\n", e.code, e.msg.c_str()); return 6; }
      }
      io.shutdown();
   }
   if (mock_pin) {
      std::lock_guard<std::mutex> lk(mp.mu);
      printf("pinned_chunks=%d given=%zu returned=%zu out=%zu\n", dev.pinned_chunks, mp.given, mp.returned, mp.out.size());
      if (!mp.out.empty() || mp.given != mp.returned || mp.given == 0) return 5;
   }
   if (fail_third) {
      printf("device_error came_through=%d\n", came_through ? 1 : 0);
      return came_through ? 0 : 6;
   }
   int written = 0, unreadable = 0, rejected = 0, other = 0;
   for (int i = 0; i < n; i++) {
      if (status[(size_t)i].stage == HESAFF_FILE_WRITTEN && status[(size_t)i].rc == HESAFF_OK) written++;
      else if (status[(size_t)i].stage == HESAFF_FILE_UNREADABLE) unreadable++;
      else if (refuse && status[(size_t)i].stage == HESAFF_FILE_REJECTED && status[(size_t)i].rc == HESAFF_ERR_CAPACITY) rejected++;
      else other++;
   }
   printf("chunks=%s\n", dev.chunk_sizes.c_str());
   if (refuse) printf("rejected=%d\n", rejected);
   printf("files=%d written=%d unreadable=%d other=%d rows=%lld\n", n, written, unreadable, other, dev.rows);
   return other == 0 ? 0 : 3;
}
