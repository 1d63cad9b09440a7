// hesaff_cli.cpp -- `hesaff <image>` : same command line, stdout line and output file as
// the reference's main() (hesaff.cpp:133-180); the work runs on the MI355X through
// libhesaff_amd.so.  Input: binary PGM/PPM (P5/P6), PNG or JPEG.
//
// Extensions (the reference has no flags; it would try to open a file called "--batch"):
//   hesaff <image> --mask <mask file>
//       a detection mask for the single-image form (hesaff_set_next_masks): an image file of ONE channel and the image's size; keypoints
//       whose pixel (x and y rounded to nearest) is zero in it are dropped on the device before findAffineShape, and the stdout line
//       and the output file hold what is left, each row as the unmasked run writes it.  Not available with --batch.
//   hesaff --batch <list file> [--devices <spec>]
//       one image path per line; every image gets the `<image>.hesaff.sift` the single-image form writes.
//       --devices 0-7 | 0,2,5 | all   shards the list over several GPUs of the node: one context per device, each on
//       its own host thread, contiguous blocks of images (hesaff_shard_range), no data exchanged between devices;
//       the per-device counts are summed on the host.  A device may be named more than once.
//       --schedule static | dynamic   static (default): one contiguous shard per device context.  dynamic: the list is cut into
//       blocks of 256 images and every device context takes the next block when it has finished its own - for lists whose
//       keypoint density varies strongly along the list; the output files are the same either way.
//       --fast 2                      hesaff_params.fast: windows larger than the patch sampled from the scale space (NOT bit-exact,
//       another algorithm for those keypoints); default 0 = parity mode.
//       --resume | --resume=strict    skip every image whose complete output (of the selected format) already exists (strict: the rows of an
//                                     existing text file are counted too - for outputs a non-renaming writer may have left torn); outputs are written
//       under a temporary name and renamed, so an interrupted run leaves no torn file (checkpoint / resume).
//       --host-share K                this process may use 1/K of the host's CPUs (default 1): one of K processes on a node, e.g. one per GPU.
//       Host threads per device context = hesaff_host_plan_for(devices x K): the library's one rule (include/hesaff_amd.h).
//       On a CPU-starved plan (CPUs of this process <= pool threads + 1, e.g. --host-share 8 on a 16-CPU quota) the threads the HIP runtime creates
//       while the contexts are made - its event thread spins for most of the time the device works - are moved to nice 19: inside a two-CPU share
//       the text path then writes 217 instead of 181 images/s (profiles/r06_notes.md).  --runtime-nice 0 leaves them alone, --runtime-nice 1 forces it.
//       --output text | bin | both    what every image gets: <image>.hesaff.sift (default), the binary sidecar
//       <image>.hesaff.bin (the same rows unprinted, include/hesaff_amd.h: hesaff_write_bin), or both.
//       --max-keypoints N             a keypoint budget per image (hesaff_set_keypoint_limit): the N Hessian keypoints of greatest |response|
//                                     are kept, in the reference's order, the rest dropped on the device before findAffineShape; N bounds the
//                                     "keypoints" count, the "affine shapes" are fewer.  Default 0 = no limit.  Batch form only.
//       --grid RxC                    with --max-keypoints N: the N / (R * C) strongest keypoints of every cell of an R x C grid over the image
//                                     (hesaff_set_keypoint_grid: a spatially uniform budget), R * C <= 64 and <= N.  Default 1x1 = no grid.
//       --orientation up | dominant   the frame every region is described in (hesaff_set_orientation): the reference's "up is up" frame
//                                     (default), or that frame turned by the dominant gradient angle of the region's own patch, which makes
//                                     the descriptors follow an in-plane rotation of the image.  Batch form, and behind a single image.
//       --orientations K              with --orientation dominant: up to K rows per region, K in 1..4 (default 1), one per peak of the region's
//                                     orientation histogram within 80 % of the highest (hesaff_set_orientation_count).  Batch form, and behind a
//                                     single image.
//       --descriptor sift | rootsift  what the 128 bytes of a row hold (hesaff_set_descriptor): the reference's SIFT bytes (default), or RootSIFT -
//                                     the vector L1-normalised and square-rooted on the device before it is quantised, for retrieval and matching
//                                     under the Hellinger kernel.  The file formats are unchanged.  Batch form, and behind a single image.
//   hesaff <image> --vocabulary <vocabulary file>
//       a vocabulary of visual words (hesaff_read_vocabulary: "HESAFFV1", rows of 128 bytes): every key is assigned the lowest row of least
//       squared distance to its descriptor on the device (hesaff_set_vocabulary), and <image>.hesaff.words (hesaff_write_words: x, y, a, b,
//       c and the word per key) is written beside the .hesaff.sift.  With --batch the same for every image of the list; --words-only
//       then writes the words files alone.  A vocabulary file that cannot be read ends the run before any image is read.
//   hesaff --batch <list file> --vocabulary <vocabulary file> --embedding <embedding file>
//       a Hamming embedding over the vocabulary (hesaff_read_embedding: "HESAFFE1", a 64 x 128 projection and 64 thresholds per row; its
//       row count must be the vocabulary's): every key also receives a 64-bit signature (hesaff_set_embedding), and <image>.hesaff.sigs
//       (hesaff_write_signatures) is written beside every words file, row for row with it; --resume counts it as part of the output.
//   hesaff --batch <list file> --vocabulary <vocabulary file> [--cells <cells file> [--probes P]] --train-embedding <embedding file> [--seed S]
//       detects and describes every image of the list on one device, assigns every key its word, takes the default projection of seed S
//       (hesaff_embedding_projection; 0 by default) and sets every word's 64 thresholds to the lower medians of its keys' projections
//       (hesaff_train_embedding); writes <embedding file>.  No per-image file is written.  At most 2^24 keys, as --train-vocabulary.
//   hesaff --batch <list file> --train-vocabulary <vocabulary file> --words K [--iterations T]
//       trains a vocabulary on the list's own descriptors (hesaff_train_vocabulary: exact integer k-means on the device, T = 10 iterations at
//       most, fewer at a fixed point; the initial rows are keys spread evenly over the list's keys in list order).  Detection runs on one device
//       with the run's other options (--descriptor, --orientation, --orientations, --max-keypoints, --grid, --fast); no per-image file is
//       written, <vocabulary file> is, and one line per iteration is printed: the distortion and the number of empty words.  At most 2^24
//       keys: a list that yields more stops with a message naming the count.
//   hesaff <image> --vocabulary <vocabulary file> --cells <cells file>      (and with --batch)
//       a cell layer over the vocabulary (hesaff_read_vocabulary_cells: "HESAFFC1", coarse rows and each cell's first row; its row count must
//       be the vocabulary's): a key is compared with the coarse rows and then only with the rows of its cell (hesaff_set_vocabulary_cells).
//       The files written are the same; the vocabulary file stays an ordinary flat vocabulary of the same rows.
//   hesaff <image> --vocabulary <vocabulary file> --cells <cells file> --probes P      (and with --batch)
//       P = 1..8: a key is searched in its P nearest cells (hesaff_set_vocabulary_probes; 1, the default, is its one cell, and from the
//       layer's cell count on the result is the flat assignment).  Needs --cells <cells file>; refused with --train-vocabulary.
//   hesaff <image> --vocabulary <vocabulary file> --neighbours R      (and with --batch, also beside --embedding)
//       R = 1..8: every key's R nearest rows of the vocabulary, not just the nearest (hesaff_set_vocabulary_neighbours; multiple assignment
//       for QUERY images).  <image>.hesaff.words then holds, for every key in key order, a row per rank in ascending rank - the key's
//       five floats, that rank's word - and <image>.hesaff.sigs is row for row with it: an ordinary words file with up to R rows per
//       key, which --query, --queries, --hamming and --verify take unchanged.  Needs --vocabulary; R > 1 does not combine with --cells.
//   hesaff --batch <list file> --train-vocabulary <vocabulary file> --words K --cells C [--iterations T] [--coarse-iterations Tc]
//       trains C coarse rows (Tc = 10 iterations at most), spreads K initial rows over the list's keys, sorts them into the cells of their
//       nearest coarse rows (hesaff_build_vocabulary_cells) and trains them inside the cells (hesaff_train_vocabulary_cells); writes
//       <vocabulary file> and <vocabulary file>.cells.  Needs K >= C.
//   hesaff --search <list of .hesaff.words files> --query <.hesaff.words file> [--top M] [--device D] [--hamming T]
//       builds an image index on device D (default 0) from the words files the list names, one per line (hesaff_index_build: an inverted
//       file with integer tf-idf weights; every file must state the same vocabulary size), queries it with the words of the query file
//       and prints the M best images (default 10, at most 1024), best first, equal scores in list order: rank<TAB>path<TAB>score, the
//       score as %.17g.  Recognised before --batch and before the single-image form.  With --hamming T (0..64) the signatures file
//       beside every words file (".sigs" in the place of the final ".words": what a context with an embedding writes) is read as well,
//       and a word match counts only where the two 64-bit signatures differ in at most T bits (hesaff_index_query_embedded); a
//       signatures file that is missing, or whose count differs from its words file's, ends the run with a message that names it.
//   hesaff --search <list of .hesaff.words files> --save-index <index file> [--device D] [--hamming T]
//       builds the same index and, instead of asking a query, writes it to <index file> (hesaff_index_save: "HESAFFI1") and the list's
//       paths, one per line, to <index file>.list.  With --hamming (any T) the signatures files are read and the index is an embedded one.
//   hesaff --index <index file> --query <.hesaff.words file> [--top M] [--device D] [--hamming T] [--verify ...]
//       as --search --query, but the index is loaded (hesaff_index_load), not built: no words file but the query's is read.  The paths
//       printed, and the candidates' rows for --verify, are those of <index file>.list.  --hamming needs an embedded index.
//   hesaff --search <list> | --index <index file>  --queries <list of .hesaff.words files> [--top M] [--device D] [--hamming T] [--verify ...]
//       in the place of --query: the listed files are ONE batch (hesaff_index_query_batch).  Per query, in list order, a line
//       "# <query path>" and then exactly the lines --query prints for that file.  --query together with --queries is a usage error.
//   hesaff --search <list> | --index <index file>  --query <.hesaff.words file> --verify [...] --expand [--min-inliers N] [--expand-images E]
//       query expansion (hesaff_expand_query): behind the verified list a line "# expanded: <rows> rows from <images> images", then
//       the list of a second query in the same line format - the query's rows and, back-projected into its frame and cut to the
//       bounding box of its live rows, those of the E best shortlisted files (default 10, at most 1024) with at least N inliers
//       (default 4) - verified with the expanded rows.  The expanded query repeats the words of those files, so the second list's inlier
//       counts need --pairs above 1.  Needs --verify; with --queries a usage error.
//   hesaff --index <index file> --add <list of .hesaff.words files> [--device D]
//       loads the index, adds the listed files behind its images (hesaff_index_add; with their signatures files where the index is an
//       embedded one) and rewrites <index file> and <index file>.list.  Both are written under temporary names and renamed when whole:
//       a run that fails leaves the pair it found.
//   hesaff --index <index file> --remove <list of paths> [--device D]
//       loads the index, removes every image whose line of <index file>.list equals a listed path (hesaff_index_remove; a path listed
//       twice counts once) and rewrites the pair likewise; the images that stay keep their order.  A path the list does not hold, an
//       empty list and a removal that would leave no image print one line, exit 1 and leave both files as they were.
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <dirent.h>
#include <set>
#include <sys/resource.h>
#include <sys/syscall.h>
#include <unistd.h>

#include "hesaff.hpp"

namespace {

std::set<long> g_tids_at_start;   // the threads this process had before it made its first library call

// the thread ids of this process (/proc/self/task)
std::set<long> list_tids()
{
   std::set<long> out;
   if (DIR *d = opendir("/proc/self/task")) {
      while (struct dirent *e = readdir(d)) {
         char *end = nullptr;
         const long t = strtol(e->d_name, &end, 10);
         if (end != e->d_name && *end == 0 && t > 0) out.insert(t);
      }
      closedir(d);
   }
   return out;
}

// "0-7", "0,2,5", "1", "all" -> device ordinals
bool parse_devices(const char *spec, std::vector<int> &out)
{
   out.clear();
   const int ndev = hesaff_device_count();
   if (strcmp(spec, "all") == 0) {
      for (int i = 0; i < ndev; i++) out.push_back(i);
      return !out.empty();
   }
   const char *p = spec;
   while (*p) {
      char *e = nullptr;
      const long a = strtol(p, &e, 10);
      if (e == p || a < 0 || a >= ndev) return false;   // checked before anything is expanded ("0-99999999999")
      long b = a;
      p = e;
      if (*p == '-') {
         b = strtol(p + 1, &e, 10);
         if (e == p + 1 || b < a || b >= ndev) return false;
         p = e;
      }
      if (out.size() + (size_t)(b - a + 1) > 4096) return false;
      for (long d = a; d <= b; d++) out.push_back((int)d);
      if (*p == ',') p++;
      else if (*p) return false;
   }
   return !out.empty();
}

// hesaff --batch: the list is cut into contiguous shards, one per device context (hesaff_shard_range); every shard runs
// through hesaff_process_files - decode threads -> device -> writer threads, bounded memory - on its own host thread.
int run_batch_mode(const char *list_path, const char *devices_spec, int out_format, bool dynamic, int fast, int resume, int host_share, int runtime_nice,
                   int max_keypoints, int orientation, int grid_rows, int grid_cols, int descriptor, int orientations,
                   const uint8_t *vocabulary, int vocabulary_size, const uint8_t *cells_coarse, const uint32_t *cells_first, int cells, int probes,
                   const int8_t *embed_P, const int32_t *embed_tau, int neighbours)
{
   std::ifstream lf(list_path);
   if (!lf) { fprintf(stderr, "hesaff: cannot read list '%s'\n", list_path); return 1; }
   std::vector<std::string> names;
   for (std::string line; std::getline(lf, line);) {
      while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
      if (!line.empty() && line[0] != '#') names.push_back(line);
   }
   std::vector<int> devices;
   if (!parse_devices(devices_spec ? devices_spec : "0", devices)) {
      fprintf(stderr, "hesaff: bad --devices '%s' (%d device(s) visible)\n", devices_spec ? devices_spec : "0", hesaff_device_count());
      return 1;
   }
   const int n = (int)names.size();
   const int world = (int)devices.size();
   std::vector<const char *> paths((size_t)n);
   for (int i = 0; i < n; i++) paths[(size_t)i] = names[(size_t)i].c_str();
   std::vector<hesaff_file_status> status((size_t)n);
   for (auto &st : status) { st.rc = HESAFF_ERR_IO; st.stage = HESAFF_FILE_PENDING; st.count_hessian = 0; st.count_desc = 0; }
   std::vector<std::string> errs((size_t)world);
   int rc = 0;
   const auto t1 = std::chrono::steady_clock::now();
   const int kBlock = 256;
   std::atomic<int> next_block(0);
   // Threads that appear while the contexts are created and that this program did not start are the HIP runtime's helpers (its event
   // thread, which spins while the device works).  On a CPU-starved plan they go to nice 19, below the pool's nice 10: the spinning then
   // yields to the threads that write.  `own`: the device workers' ids, complete before the first context is made (the latch below).
   const std::set<long> &tids_before = g_tids_at_start;   // (taken in main: already hesaff_device_count starts the runtime)
   std::mutex own_mu;
   std::condition_variable own_cv;
   std::set<long> own;
   auto device_worker = [&](int rank) {
      {
         std::unique_lock<std::mutex> lk(own_mu);
         own.insert((long)syscall(SYS_gettid));
         own_cv.notify_all();
         own_cv.wait(lk, [&] { return (int)own.size() >= world; });
      }
      int lo = 0, hi = 0;
      hesaff_shard_range(n, rank, world, &lo, &hi);
      if (!dynamic && hi <= lo) return;
      hesaff_params par;
      hesaff_default_params(&par);
      par.max_batch = std::max(1, std::min(dynamic ? n : hi - lo, 64));
      par.fast = fast;
      hesaff_ctx *ctx = nullptr;
      if (hesaff_create(&ctx, &par, devices[(size_t)rank]) != HESAFF_OK) { errs[(size_t)rank] = hesaff_last_error(nullptr); return; }
      hesaff_set_output_format(ctx, out_format);
      hesaff_set_resume(ctx, resume);
      hesaff_set_keypoint_limit(ctx, max_keypoints);
      hesaff_set_keypoint_grid(ctx, grid_rows, grid_cols);   // (main checked it against the limit)
      hesaff_set_orientation(ctx, orientation);
      hesaff_set_orientation_count(ctx, orientations);
      hesaff_set_descriptor(ctx, descriptor);
      if (vocabulary_size > 0 && hesaff_set_vocabulary(ctx, vocabulary_size, vocabulary) != HESAFF_OK) {
         errs[(size_t)rank] = hesaff_last_error(ctx);
         hesaff_destroy(ctx);
         return;
      }
      if (cells > 0 && hesaff_set_vocabulary_cells(ctx, cells, cells_coarse, cells_first) != HESAFF_OK) {
         errs[(size_t)rank] = "the cells file does not describe the vocabulary";
         hesaff_destroy(ctx);
         return;
      }
      hesaff_set_vocabulary_probes(ctx, probes);   // (main checked the range)
      hesaff_set_vocabulary_neighbours(ctx, neighbours);   // (likewise, and that no layer goes with a count above 1)
      if (embed_P && hesaff_set_embedding(ctx, embed_P, embed_tau) != HESAFF_OK) {   // (main checked its rows against the vocabulary's)
         errs[(size_t)rank] = hesaff_last_error(ctx);
         hesaff_destroy(ctx);
         return;
      }
      hesaff_host_plan hp;   // this device's share of the host: the library's one rule (include/hesaff_amd.h)
      hesaff_host_plan_for(world * host_share, &hp);
      const int wt = hp.write_threads, dt = hp.decode_threads;
      if (runtime_nice == 1 || (runtime_nice < 0 && hp.cpus <= dt + wt + 1)) {   // this device's share of the host is no larger than its pool + the caller
         {
            // one tiny batch through the context first: the runtime starts its helper threads with the first launches and events, not with the context
            std::vector<uint8_t> blank((size_t)64 * 64, 0);
            const uint8_t *img = blank.data();
            const int side = 64, chn = 1;
            hesaff_result res;
            (void)hesaff_detect_batch(ctx, 1, &img, &side, &side, &side, &chn, &res);
         }
         std::lock_guard<std::mutex> lk(own_mu);
         int moved = 0;
         for (long t : list_tids())
            if (!tids_before.count(t) && !own.count(t) && setpriority(PRIO_PROCESS, (id_t)t, 19) == 0) moved++;   // (a refusal changes nothing)
         if (runtime_nice == 1) fprintf(stderr, "hesaff: device %d: %d runtime helper thread(s) at nice 19\n", devices[(size_t)rank], moved);
      }
      for (;;) {
         if (dynamic) {   // the next block of the list nobody has taken yet
            lo = next_block.fetch_add(1) * kBlock;
            hi = std::min(n, lo + kBlock);
         }
         if (hi <= lo) break;
         if (hesaff_process_files(ctx, hi - lo, paths.data() + lo, nullptr, dt, wt, status.data() + lo) != HESAFF_OK) { errs[(size_t)rank] = hesaff_last_error(ctx); break; }
         if (!dynamic) break;
      }
      hesaff_destroy(ctx);
   };
   {
      std::vector<std::thread> th;
      for (int r = 1; r < world; r++) th.emplace_back(device_worker, r);
      device_worker(0);
      for (auto &x : th) x.join();
   }
   const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
   long long tot_h = 0, tot_d = 0;
   int n_ok = 0, n_skipped = 0;
   for (int r = 0; r < world; r++)
      if (!errs[(size_t)r].empty()) { fprintf(stderr, "hesaff: device %d: %s\n", devices[(size_t)r], errs[(size_t)r].c_str()); rc = 1; }
   for (int i = 0; i < n; i++) {
      const hesaff_file_status &st = status[(size_t)i];
      if (st.rc == HESAFF_OK && st.stage == HESAFF_FILE_SKIPPED) {
         std::cout << names[(size_t)i] << ": output exists (" << st.count_desc << " rows), skipped" << std::endl;
         n_skipped++;
      } else if (st.rc == HESAFF_OK) {
         std::cout << names[(size_t)i] << ": Detected " << st.count_hessian << " keypoints and " << st.count_desc << " affine shapes" << std::endl;
         tot_h += st.count_hessian; tot_d += st.count_desc; n_ok++;
      } else {
         rc = 1;
         if (st.stage == HESAFF_FILE_DETECTED) fprintf(stderr, "hesaff: cannot write the output of '%s'\n", names[(size_t)i].c_str());
         else if (st.stage == HESAFF_FILE_UNREADABLE)
            fprintf(stderr, "hesaff: cannot read '%s' (PBM / PGM / PPM, PNG, JPEG, BMP or baseline TIFF expected): skipped\n", names[(size_t)i].c_str());
      }
   }
   std::cout << "Detected " << tot_h << " keypoints and " << tot_d << " affine shapes in " << n_ok << " images in " << dt << " sec.";
   if (n_skipped) std::cout << " (" << n_skipped << " more skipped: complete outputs exist)";
   if (world > 1) std::cout << " (" << world << " device contexts)";
   std::cout << std::endl;
   return rc;
}

// hesaff --batch <list> --train-vocabulary <file> --words K: detect over the list on one device, keep every key's descriptor bytes in host
// memory in list order (a hesaff_detect_batch_cb sink), train K words on them (hesaff_train_vocabulary) and write the vocabulary file.
struct DescSink {
   std::vector<std::vector<uint8_t>> *per_image;
   int first;   // list index of the block's first image
   static int take(void *user, int n_images, const int *image_index, const hesaff_result *results)
   {
      DescSink *s = (DescSink *)user;
      for (int i = 0; i < n_images; i++) {
         std::vector<uint8_t> &d = (*s->per_image)[(size_t)(s->first + image_index[i])];
         d.resize((size_t)results[i].count_desc * 128);
         for (int q = 0; q < results[i].count_desc; q++) memcpy(d.data() + (size_t)q * 128, results[i].keys[q].desc, 128);
      }
      return 0;
   }
};

// With `embed` (hesaff --batch <list> --vocabulary <file> --train-embedding <file>): the same collection of descriptors, then their
// words under the vocabulary (and its cell layer and probes, where given), the default projection of `seed`, the thresholds of every
// word (hesaff_train_embedding) and the embedding file.
struct TrainEmbedding {
   const uint8_t *vocabulary; int vocabulary_size;
   const uint8_t *cells_coarse; const uint32_t *cells_first; int cells; int probes;
   uint64_t seed;
};

int run_train_mode(const char *list_path, const char *devices_spec, const char *out_path, int k, int iterations, int fast, int max_keypoints, int orientation,
                   int grid_rows, int grid_cols, int descriptor, int orientations, int cells, int coarse_iterations, const TrainEmbedding *embed = nullptr)
{
   std::ifstream lf(list_path);
   if (!lf) { fprintf(stderr, "hesaff: cannot read list '%s'\n", list_path); return 1; }
   std::vector<std::string> names;
   for (std::string line; std::getline(lf, line);) {
      while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
      if (!line.empty() && line[0] != '#') names.push_back(line);
   }
   std::vector<int> devices;
   if (!parse_devices(devices_spec ? devices_spec : "0", devices)) {
      fprintf(stderr, "hesaff: bad --devices '%s' (%d device(s) visible)\n", devices_spec ? devices_spec : "0", hesaff_device_count());
      return 1;
   }
   const int n = (int)names.size(), kBlock = 64;
   hesaff_params par;
   hesaff_default_params(&par);
   par.max_batch = std::max(1, std::min(n, kBlock));
   par.fast = fast;
   hesaff_ctx *ctx = nullptr;
   if (hesaff_create(&ctx, &par, devices[0]) != HESAFF_OK) { fprintf(stderr, "hesaff: device %d: %s\n", devices[0], hesaff_last_error(nullptr)); return 1; }
   struct Destroy { hesaff_ctx *c; ~Destroy() { hesaff_destroy(c); } } destroy{ctx};
   hesaff_set_keypoint_limit(ctx, max_keypoints);
   hesaff_set_keypoint_grid(ctx, grid_rows, grid_cols);
   hesaff_set_orientation(ctx, orientation);
   hesaff_set_orientation_count(ctx, orientations);
   hesaff_set_descriptor(ctx, descriptor);
   std::vector<std::vector<uint8_t>> per_image((size_t)n);
   long long total = 0;
   int rc = 0;
   for (int lo = 0; lo < n; lo += kBlock) {
      const int hi = std::min(n, lo + kBlock);
      std::vector<uint8_t *> data;
      std::vector<const uint8_t *> images;
      std::vector<int> widths, heights, strides, channels, index;
      for (int i = lo; i < hi; i++) {
         uint8_t *px = nullptr;
         int w = 0, h = 0, ch = 0;
         if (hesaff_read_image(names[(size_t)i].c_str(), &px, &w, &h, &ch) != HESAFF_OK) {
            fprintf(stderr, "hesaff: cannot read '%s' (PBM / PGM / PPM, PNG, JPEG, BMP or baseline TIFF expected): skipped\n", names[(size_t)i].c_str());
            rc = 1;
            continue;
         }
         data.push_back(px); images.push_back(px); widths.push_back(w); heights.push_back(h); strides.push_back(w * ch); channels.push_back(ch);
         index.push_back(i);
      }
      // (the sink sees positions in this block's arrays: unreadable files leave gaps in the list, so the block's images are re-indexed)
      std::vector<std::vector<uint8_t>> block(images.size());
      DescSink sink{&block, 0};
      const int drc = hesaff_detect_batch_cb(ctx, (int)images.size(), images.data(), widths.data(), heights.data(), strides.data(), channels.data(), DescSink::take, &sink);
      for (uint8_t *px : data) hesaff_free(px);
      if (drc != HESAFF_OK) { fprintf(stderr, "hesaff: %s\n", hesaff_last_error(ctx)); return 1; }
      for (size_t j = 0; j < block.size(); j++) {
         total += (long long)(block[j].size() / 128);
         per_image[(size_t)index[j]] = std::move(block[j]);
      }
      if (total > (1ll << 24)) {
         fprintf(stderr, "hesaff: the list yields more than 2^24 keys (%lld after %d of %d images): train on fewer images, or set --max-keypoints\n", total, hi, n);
         return 1;
      }
   }
   if (embed && total < 1) { fprintf(stderr, "hesaff: the list yields no key to train an embedding on\n"); return 1; }
   if (!embed && total < k) { fprintf(stderr, "hesaff: the list yields %lld keys, fewer than --words %d\n", total, k); return 1; }
   std::vector<uint8_t> desc;
   desc.reserve((size_t)total * 128);
   for (std::vector<uint8_t> &d : per_image) {
      desc.insert(desc.end(), d.begin(), d.end());
      std::vector<uint8_t>().swap(d);
   }
   if (embed) {
      const int K = embed->vocabulary_size;
      if (hesaff_set_vocabulary(ctx, K, embed->vocabulary) != HESAFF_OK ||
          (embed->cells > 0 && hesaff_set_vocabulary_cells(ctx, embed->cells, embed->cells_coarse, embed->cells_first) != HESAFF_OK) ||
          hesaff_set_vocabulary_probes(ctx, embed->probes) != HESAFF_OK) {
         fprintf(stderr, "hesaff: the vocabulary was not set: %s\n", hesaff_last_error(ctx));
         return 1;
      }
      std::vector<int32_t> words((size_t)total * 2), tau((size_t)K * HESAFF_EMBED_BITS);
      std::vector<uint32_t> counts((size_t)K);
      std::vector<int8_t> P((size_t)HESAFF_EMBED_BITS * 128);
      hesaff_embedding_projection(embed->seed, P.data());
      if (hesaff_stage_assign_words(ctx, (int)total, desc.data(), words.data()) != HESAFF_OK ||
          hesaff_train_embedding(ctx, total, desc.data(), words.data(), 2, K, P.data(), tau.data(), counts.data()) != HESAFF_OK) {
         fprintf(stderr, "hesaff: training the embedding failed: %s\n", hesaff_last_error(ctx));
         return 1;
      }
      if (hesaff_write_embedding(out_path, K, P.data(), tau.data()) != HESAFF_OK) { fprintf(stderr, "hesaff: cannot write '%s'\n", out_path); return 1; }
      long long empty_words = 0;
      for (uint32_t m : counts) empty_words += m == 0 ? 1 : 0;
      std::cout << "Trained the thresholds of " << K << " words on " << total << " keys of " << n << " images (seed " << embed->seed << ", " << empty_words
                << " words without keys)" << std::endl;
      return rc;
   }
   std::vector<uint8_t> rows((size_t)k * 128);
   std::vector<int64_t> distortion((size_t)iterations);
   std::vector<int32_t> empty((size_t)iterations);
   int done = 0;
   if (cells > 0) {
      // the composite: C coarse rows, K initial rows spread over the keys, sorted into cells, trained inside them
      std::vector<uint8_t> coarse((size_t)cells * 128), v0((size_t)k * 128), kept((size_t)cells * 128);
      std::vector<uint32_t> first((size_t)cells + 1);
      std::vector<int32_t> order((size_t)k);
      int n_cells = 0;
      if (hesaff_train_vocabulary(ctx, total, desc.data(), cells, nullptr, coarse_iterations, coarse.data(), nullptr, nullptr, nullptr) != HESAFF_OK) {
         fprintf(stderr, "hesaff: training the coarse rows failed: %s\n", hesaff_last_error(ctx));
         return 1;
      }
      for (long long r = 0; r < k; r++) memcpy(&v0[(size_t)r * 128], &desc[(size_t)(r * total / k) * 128], 128);
      if (hesaff_build_vocabulary_cells(ctx, k, v0.data(), cells, coarse.data(), rows.data(), order.data(), kept.data(), first.data(), &n_cells) != HESAFF_OK ||
          hesaff_train_vocabulary_cells(ctx, total, desc.data(), k, rows.data(), n_cells, kept.data(), first.data(), iterations, v0.data(), distortion.data(),
                                        empty.data(), &done) != HESAFF_OK) {
         fprintf(stderr, "hesaff: training failed: %s\n", hesaff_last_error(ctx));
         return 1;
      }
      rows.swap(v0);
      const std::string cells_path = std::string(out_path) + ".cells";
      if (hesaff_write_vocabulary_cells(cells_path.c_str(), n_cells, kept.data(), first.data()) != HESAFF_OK) {
         fprintf(stderr, "hesaff: cannot write '%s'\n", cells_path.c_str());
         return 1;
      }
      std::cout << n_cells << " of " << cells << " cells hold rows" << std::endl;
   } else if (hesaff_train_vocabulary(ctx, total, desc.data(), k, nullptr, iterations, rows.data(), distortion.data(), empty.data(), &done) != HESAFF_OK) {
      fprintf(stderr, "hesaff: training failed: %s\n", hesaff_last_error(ctx));
      return 1;
   }
   if (hesaff_write_vocabulary(out_path, rows.data(), k) != HESAFF_OK) { fprintf(stderr, "hesaff: cannot write '%s'\n", out_path); return 1; }
   for (int t = 0; t < done; t++) std::cout << "iteration " << t + 1 << ": distortion " << distortion[(size_t)t] << ", " << empty[(size_t)t] << " empty words" << std::endl;
   std::cout << "Trained " << k << " words on " << total << " keys of " << n << " images in " << done << " iterations"
             << (done < iterations ? " (fixed point)" : "") << std::endl;
   return rc;
}

// hesaff --search <list> --query <file>: the word columns of the listed files (hesaff_read_words) into one index, one query, the
// ranked list on stdout.  With --verify the rows of the query and of the shortlisted files (hesaff_read_words_rows) go through
// hesaff_verify_matches, and the shortlist is printed in verified order with its inlier counts.  With --hamming T (hamming >= 0) the
// signatures file beside every words file is read as well (hesaff_read_signatures), the index is an embedded one and the query
// counts a word match only within T bits (hesaff_index_query_embedded); verification keeps its pair rule.

// the signatures file beside a words file: its name with ".sigs" in the place of a final ".words", or appended where there is none
std::string sigs_name_for(const std::string &words)
{
   const size_t n = words.size();
   return n >= 6 && words.compare(n - 6, 6, ".words") == 0 ? words.substr(0, n - 6) + ".sigs" : words + ".sigs";
}

// the lines of a list file: trailing blanks cut, empty lines and lines that begin with # skipped
bool read_list(const char *list_path, std::vector<std::string> &names)
{
   std::ifstream lf(list_path);
   if (!lf) { fprintf(stderr, "hesaff: cannot read list '%s'\n", list_path); return false; }
   for (std::string line; std::getline(lf, line);) {
      while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
      if (!line.empty() && line[0] != '#') names.push_back(line);
   }
   return true;
}

// the word columns (and with_sigs the signatures) of words files, one file after the other; k: the vocabulary size they all state
// (0: the first file's)
struct WordsReader {
   std::vector<int32_t> words;
   std::vector<uint64_t> sigs;
   int k = 0;
   bool with_sigs = false;
   bool read_sigs(const char *words_path, int count)
   {
      const std::string path = sigs_name_for(words_path);
      uint64_t *g = nullptr;
      int n = 0;
      if (hesaff_read_signatures(path.c_str(), &g, &n) != HESAFF_OK) {
         fprintf(stderr, "hesaff: --hamming needs the signatures file '%s' beside '%s', and it cannot be read (a .hesaff.sigs file expected)\n", path.c_str(), words_path);
         return false;
      }
      if (n != count) {
         fprintf(stderr, "hesaff: '%s' holds %d signatures, '%s' %d words\n", path.c_str(), n, words_path, count);
         hesaff_free(g);
         return false;
      }
      sigs.insert(sigs.end(), g, g + n);
      hesaff_free(g);
      return true;
   }
   bool read(const char *path, int &count)
   {
      int32_t *w = nullptr;
      int vs = 0;
      if (hesaff_read_words(path, &w, &count, &vs) != HESAFF_OK) { fprintf(stderr, "hesaff: cannot read '%s' (a .hesaff.words file expected)\n", path); return false; }
      words.insert(words.end(), w, w + count);
      hesaff_free(w);
      if (k == 0) k = vs;
      if (vs != k || vs < 1) { fprintf(stderr, "hesaff: '%s' states vocabulary size %d, the files before it %d\n", path, vs, k); return false; }
      return !with_sigs || read_sigs(path, count);
   }
   bool read_all(const std::vector<std::string> &names, std::vector<int32_t> &counts)
   {
      for (const std::string &name : names) {
         int count = 0;
         if (!read(name.c_str(), count)) return false;
         counts.push_back(count);
      }
      return true;
   }
};

hesaff_ctx *search_context(int device)
{
   hesaff_params par;
   hesaff_default_params(&par);
   par.max_batch = 1;
   hesaff_ctx *ctx = nullptr;
   if (hesaff_create(&ctx, &par, device) != HESAFF_OK) { fprintf(stderr, "hesaff: device %d: %s\n", device, hesaff_last_error(nullptr)); return nullptr; }
   return ctx;
}
struct DestroyContext { hesaff_ctx *c; ~DestroyContext() { hesaff_destroy(c); } };

// the rows of a words file that states vocabulary size k, appended to `to`
bool read_rows(const char *path, int k, std::vector<char> &to, int &n)
{
   void *p = nullptr;
   int vs = 0;
   if (hesaff_read_words_rows(path, &p, &n, &vs) != HESAFF_OK || vs != k) { fprintf(stderr, "hesaff: cannot read the rows of '%s'\n", path); hesaff_free(p); return false; }
   to.insert(to.end(), (const char *)p, (const char *)p + (size_t)n * 24);
   hesaff_free(p);
   return true;
}

// a shortlist with the rows of its files, verified against a query's rows
struct Shortlist {
   std::vector<char> rows;
   std::vector<int32_t> row_counts, out, order;
   std::vector<float> hyp;
};
// --expand: the verified shortlist's best `images` files with at least `min_inliers` inliers extend the query
struct ExpandOptions { int min_inliers, images; };

// the verified list of `count` images on stdout; s keeps what the verification read and returned
int print_verified(hesaff_ctx *ctx, const std::vector<std::string> &names, int k, const std::vector<char> &query_rows, int nq_rows, const int32_t *images,
                   const double *scores, int count, float tolerance, int max_pairs, Shortlist &s)
{
   for (int r = 0; r < count; r++) {
      int n = 0;
      if (!read_rows(names[(size_t)images[(size_t)r]].c_str(), k, s.rows, n)) return 1;
      s.row_counts.push_back(n);
   }
   s.out.resize((size_t)count * 6); s.order.resize((size_t)count); s.hyp.resize((size_t)count * 3);
   if (hesaff_verify_matches(ctx, nq_rows, query_rows.data(), count, s.row_counts.data(), s.rows.data(), k, max_pairs, tolerance, s.out.data(), s.hyp.data(),
                             s.order.data()) != HESAFF_OK) {
      fprintf(stderr, "hesaff: the verification failed: %s\n", hesaff_last_error(ctx));
      return 1;
   }
   for (int r = 0; r < count; r++) {
      const size_t c = (size_t)s.order[(size_t)r];
      printf("%d\t%s\t%.17g\t%d\n", r + 1, names[(size_t)images[c]].c_str(), scores[c], s.out[c * 6]);
   }
   return 0;
}

// the ranked list of one query - `count` images of the context's index, whose images are the files `names`, and their scores - on
// stdout; with verify the verified list.  With expand (hesaff_expand_query, the region the bounding box of the query's live rows) a
// line "# expanded: <rows> rows from <images> images" follows, and then the list of the expanded query, verified with the expanded
// rows; with hamming >= 0 the signatures travel with the rows and the second query is an embedded one as the first was.
int print_ranked(hesaff_ctx *ctx, const std::vector<std::string> &names, int k, const char *query_path, const int32_t *images, const double *scores, int count,
                 bool verify, float tolerance, int max_pairs, const ExpandOptions *expand = nullptr, int top = 0, int hamming = -1, const uint64_t *qsigs = nullptr)
{
   if (!verify) {
      for (int r = 0; r < count; r++) printf("%d\t%s\t%.17g\n", r + 1, names[(size_t)images[(size_t)r]].c_str(), scores[(size_t)r]);
      return 0;
   }
   std::vector<char> query_rows;
   int nq_rows = 0;
   if (!read_rows(query_path, k, query_rows, nq_rows)) return 1;
   Shortlist first;
   const int rc = print_verified(ctx, names, k, query_rows, nq_rows, images, scores, count, tolerance, max_pairs, first);
   if (rc != 0 || !expand) return rc;
   WordsReader sigs;   // (--hamming: the signatures of the shortlisted files)
   if (hamming >= 0)
      for (int r = 0; r < count; r++)
         if (!sigs.read_sigs(names[(size_t)images[(size_t)r]].c_str(), first.row_counts[(size_t)r])) return 1;
   float roi[4];
   hesaff_amd::AffineHessianDetector::liveBounds(query_rows.data(), nq_rows, roi);
   const int max_rows = 1 << 18;
   size_t cap = (size_t)nq_rows;
   for (int32_t n : first.row_counts) cap += (size_t)n;
   cap = std::max<size_t>(std::min<size_t>(cap, (size_t)max_rows), 1);
   std::vector<char> rows(cap * 24);
   std::vector<int32_t> words(cap), info((size_t)count * 4);
   std::vector<uint64_t> sigs_out(hamming >= 0 ? cap : 0);
   int n_out = 0;
   if (hesaff_expand_query(ctx, nq_rows, query_rows.data(), hamming >= 0 ? qsigs : nullptr, count, first.row_counts.data(), first.rows.data(),
                           hamming >= 0 ? sigs.sigs.data() : nullptr, first.out.data(), first.hyp.data(), expand->min_inliers, expand->images, roi, k, max_rows, rows.data(),
                           words.data(), hamming >= 0 ? sigs_out.data() : nullptr, &n_out, info.data()) != HESAFF_OK) {
      fprintf(stderr, "hesaff: the expansion failed: %s\n", hesaff_last_error(ctx));
      return 1;
   }
   int selected = 0;
   for (int r = 0; r < count; r++) selected += info[(size_t)r * 4] >= 0 ? 1 : 0;
   printf("# expanded: %d rows from %d images\n", n_out, selected);
   std::vector<int32_t> images2((size_t)top);
   std::vector<double> scores2((size_t)top);
   int count2 = 0;
   const int asked = hamming < 0 ? hesaff_index_query(ctx, n_out, words.data(), 1, top, images2.data(), scores2.data(), &count2)
                                 : hesaff_index_query_embedded(ctx, n_out, words.data(), 1, sigs_out.data(), hamming, top, images2.data(), scores2.data(), &count2);
   if (asked != HESAFF_OK) {
      fprintf(stderr, "hesaff: the expanded query failed: %s\n", hesaff_last_error(ctx));
      return 1;
   }
   rows.resize((size_t)n_out * 24);
   Shortlist second;
   return print_verified(ctx, names, k, rows, n_out, images2.data(), scores2.data(), count2, tolerance, max_pairs, second);
}

// the query over the context's index; the ranked list (with verify: the verified list, with expand the second one as well) on stdout
int answer_query(hesaff_ctx *ctx, const std::vector<std::string> &names, int k, const char *query_path, const int32_t *qwords, int n_query, const uint64_t *qsigs,
                 int top, bool verify, float tolerance, int max_pairs, int hamming, const ExpandOptions *expand = nullptr)
{
   std::vector<int32_t> images((size_t)top);
   std::vector<double> scores((size_t)top);
   int count = 0;
   const int asked = hamming < 0 ? hesaff_index_query(ctx, n_query, qwords, 1, top, images.data(), scores.data(), &count)
                                 : hesaff_index_query_embedded(ctx, n_query, qwords, 1, qsigs, hamming, top, images.data(), scores.data(), &count);
   if (asked != HESAFF_OK) {
      fprintf(stderr, "hesaff: the query failed: %s\n", hesaff_last_error(ctx));
      return 1;
   }
   return print_ranked(ctx, names, k, query_path, images.data(), scores.data(), count, verify, tolerance, max_pairs, expand, top, hamming, qsigs);
}

// hesaff ... --queries <list>: the listed words files (and with --hamming their signatures files) as ONE batch over the context's
// index (hesaff_index_query_batch); per query, in list order, a line "# <query path>" and then exactly what --query prints for that
// file.  --verify runs per query on its own shortlist.
int answer_queries(hesaff_ctx *ctx, const std::vector<std::string> &names, int k, const char *queries_path, int top, bool verify, float tolerance, int max_pairs,
                   int hamming)
{
   std::vector<std::string> queries;
   if (!read_list(queries_path, queries)) return 1;
   if (queries.empty()) { fprintf(stderr, "hesaff: list '%s' names no words file\n", queries_path); return 1; }
   if (queries.size() > 65536) { fprintf(stderr, "hesaff: list '%s' names %zu queries, a batch takes at most 65536\n", queries_path, queries.size()); return 1; }
   std::vector<int32_t> counts;
   WordsReader in;
   in.k = k;
   in.with_sigs = hamming >= 0;
   if (!in.read_all(queries, counts)) return 1;
   const size_t nq = queries.size();
   std::vector<int32_t> images(nq * (size_t)top);
   std::vector<double> scores(nq * (size_t)top);
   int count = 0;
   const int asked = hamming < 0 ? hesaff_index_query_batch(ctx, (int)nq, counts.data(), in.words.data(), 1, top, images.data(), scores.data(), &count)
                                 : hesaff_index_query_batch_embedded(ctx, (int)nq, counts.data(), in.words.data(), 1, in.sigs.data(), hamming, top, images.data(),
                                                                     scores.data(), &count);
   if (asked != HESAFF_OK) {
      fprintf(stderr, "hesaff: the queries failed: %s\n", hesaff_last_error(ctx));
      return 1;
   }
   for (size_t q = 0; q < nq; q++) {
      printf("# %s\n", queries[q].c_str());
      const int rc = print_ranked(ctx, names, k, queries[q].c_str(), images.data() + q * (size_t)top, scores.data() + q * (size_t)top, count, verify, tolerance, max_pairs);
      if (rc != 0) return rc;
   }
   return 0;
}

// the pair of an index: <index> (hesaff_index_save) and <index>.list, the paths of its images one per line.  Both are written under
// temporary names and renamed when both are whole, so that a run that fails leaves the pair it found.
int write_index_pair(hesaff_ctx *ctx, const char *index_path, const std::vector<std::string> &names)
{
   const std::string list = std::string(index_path) + ".list", new_index = std::string(index_path) + ".new", new_list = list + ".new";
   bool ok = hesaff_index_save(ctx, new_index.c_str()) == HESAFF_OK;
   if (!ok) fprintf(stderr, "hesaff: cannot write '%s': %s\n", index_path, hesaff_last_error(ctx));
   if (ok) {
      std::ofstream lf(new_list.c_str(), std::ios::trunc);
      for (const std::string &name : names) lf << name << '\n';
      lf.close();
      ok = !lf.fail();
      if (!ok) fprintf(stderr, "hesaff: cannot write '%s'\n", list.c_str());
   }
   if (ok) {
      ok = rename(new_index.c_str(), index_path) == 0 && rename(new_list.c_str(), list.c_str()) == 0;
      if (!ok) fprintf(stderr, "hesaff: cannot rename the new index to '%s'\n", index_path);
   }
   if (!ok) { remove(new_index.c_str()); remove(new_list.c_str()); }
   return ok ? 0 : 1;
}

// save_path == nullptr: hesaff --search <list> --query <file>, the index built for this one query.  Otherwise hesaff --search <list>
// --save-index <index>: the index is built (an embedded one with --hamming) and written with its list; no query is asked.
int run_search_mode(const char *list_path, const char *query_path, int top, int device, bool verify, float tolerance, int max_pairs, int hamming,
                    const char *save_path = nullptr, const char *queries_path = nullptr, const ExpandOptions *expand = nullptr)
{
   std::vector<std::string> names;
   if (!read_list(list_path, names)) return 1;
   if (names.empty()) { fprintf(stderr, "hesaff: list '%s' names no words file\n", list_path); return 1; }
   std::vector<int32_t> counts;
   WordsReader in;
   in.with_sigs = hamming >= 0;
   if (!in.read_all(names, counts)) return 1;
   const size_t indexed = in.words.size();
   int n_query = 0;
   if (query_path && !in.read(query_path, n_query)) return 1;
   hesaff_ctx *ctx = search_context(device);
   if (!ctx) return 1;
   DestroyContext destroy{ctx};
   const int built = hamming < 0 ? hesaff_index_build(ctx, (int)counts.size(), counts.data(), in.words.data(), 1, in.k)
                                 : hesaff_index_build_embedded(ctx, (int)counts.size(), counts.data(), in.words.data(), 1, in.sigs.data(), in.k);
   if (built != HESAFF_OK) {
      fprintf(stderr, "hesaff: the index was not built: %s\n", hesaff_last_error(ctx));
      return 1;
   }
   if (save_path) return write_index_pair(ctx, save_path, names);
   if (queries_path) return answer_queries(ctx, names, in.k, queries_path, top, verify, tolerance, max_pairs, hamming);
   return answer_query(ctx, names, in.k, query_path, in.words.data() + indexed, n_query, in.sigs.data() + indexed, top, verify, tolerance, max_pairs, hamming, expand);
}

// hesaff --index <index> --query <file>: the index is loaded (hesaff_index_load), not built; the result paths, and the candidates'
// rows for --verify, are those of <index>.list.  hesaff --index <index> --add <list>: the listed words files (and their signatures
// files where the index is an embedded one) are added behind the index's images (hesaff_index_add) and the pair is rewritten.
// hesaff --index <index> --remove <list>: every line of <index>.list equal to a listed path is removed (hesaff_index_remove; a path
// listed twice counts once) and the pair is rewritten.  A path the list does not hold, an empty list and a removal that would leave
// no image end the run before the index is read.
int run_index_mode(const char *index_path, const char *query_path, const char *add_path, int top, int device, bool verify, float tolerance, int max_pairs, int hamming,
                   const char *queries_path = nullptr, const char *remove_path = nullptr, const ExpandOptions *expand = nullptr)
{
   std::vector<std::string> names, more;
   const std::string list = std::string(index_path) + ".list";
   if (!read_list(list.c_str(), names)) return 1;
   if (add_path && !read_list(add_path, more)) return 1;
   if (add_path && more.empty()) { fprintf(stderr, "hesaff: list '%s' names no words file\n", add_path); return 1; }
   std::vector<int32_t> gone;   // --remove: the numbers of the images that go
   std::vector<std::string> kept;
   if (remove_path) {
      if (!read_list(remove_path, more)) return 1;
      if (more.empty()) { fprintf(stderr, "hesaff: list '%s' names no image\n", remove_path); return 1; }
      const std::set<std::string> named(more.begin(), more.end());
      std::set<std::string> found;
      for (size_t i = 0; i < names.size(); i++) {
         if (named.count(names[i])) { gone.push_back((int32_t)i); found.insert(names[i]); }
         else kept.push_back(names[i]);
      }
      for (const std::string &name : more)
         if (!found.count(name)) { fprintf(stderr, "hesaff: '%s' holds no image '%s'\n", list.c_str(), name.c_str()); return 1; }
      if (kept.empty()) { fprintf(stderr, "hesaff: removing every image of '%s' would leave no index\n", index_path); return 1; }
   }
   hesaff_ctx *ctx = search_context(device);
   if (!ctx) return 1;
   DestroyContext destroy{ctx};
   if (hesaff_index_load(ctx, index_path) != HESAFF_OK) { fprintf(stderr, "hesaff: the index was not loaded: %s\n", hesaff_last_error(ctx)); return 1; }
   int n_images = 0, k = 0, embedded = 0;
   hesaff_index_get_info(ctx, &n_images, &k, nullptr, nullptr);
   hesaff_index_get_embedded(ctx, &embedded, nullptr, nullptr, nullptr);
   if ((size_t)n_images != names.size()) { fprintf(stderr, "hesaff: '%s' holds %d images, '%s' names %zu\n", index_path, n_images, list.c_str(), names.size()); return 1; }
   WordsReader in;
   in.k = k;
   if (add_path) {
      std::vector<int32_t> counts;
      in.with_sigs = embedded != 0;
      if (!in.read_all(more, counts)) return 1;
      const int added = embedded ? hesaff_index_add_embedded(ctx, (int)counts.size(), counts.data(), in.words.data(), 1, in.sigs.data())
                                 : hesaff_index_add(ctx, (int)counts.size(), counts.data(), in.words.data(), 1);
      if (added != HESAFF_OK) {
         fprintf(stderr, "hesaff: the images were not added (an index holds at most 2^20 images and 2^28 keys): %s\n", hesaff_last_error(ctx));
         return 1;
      }
      names.insert(names.end(), more.begin(), more.end());
      return write_index_pair(ctx, index_path, names);
   }
   if (remove_path) {
      if (hesaff_index_remove(ctx, (int)gone.size(), gone.data(), nullptr) != HESAFF_OK) {
         fprintf(stderr, "hesaff: the images were not removed: %s\n", hesaff_last_error(ctx));
         return 1;
      }
      return write_index_pair(ctx, index_path, kept);
   }
   if (hamming >= 0 && !embedded) { fprintf(stderr, "hesaff: '%s' holds no signatures: --hamming needs an index saved with --hamming\n", index_path); return 1; }
   if (queries_path) return answer_queries(ctx, names, k, queries_path, top, verify, tolerance, max_pairs, hamming);
   in.with_sigs = hamming >= 0;
   int n_query = 0;
   if (!in.read(query_path, n_query)) return 1;
   return answer_query(ctx, names, k, query_path, in.words.data(), n_query, in.sigs.data(), top, verify, tolerance, max_pairs, hamming, expand);
}

} // namespace

int main(int argc, char **argv)
{
   g_tids_at_start = list_tids();
   if (hesaff_abi_version() != HESAFF_ABI_VERSION || hesaff_sizeof_params() != sizeof(hesaff_params)) {
      fprintf(stderr, "hesaff: libhesaff_amd.so has ABI version %d, this program was built for %d\n", hesaff_abi_version(), HESAFF_ABI_VERSION);
      return 1;
   }
   // batch mode: "--batch <list>" and the other options in any order (the reference has no options: a first argument that does
   // not start with "--" is an image, as in hesaff.cpp:133-137)
   bool search = false, from_index = false;
   for (int i = 1; i < argc; i++) search = search || strcmp(argv[i], "--search") == 0;
   for (int i = 1; i < argc; i++) from_index = from_index || strcmp(argv[i], "--index") == 0;
   bool batch_queries = false;   // --queries without --search or --index: the index form's usage error
   for (int i = 1; i < argc; i++) batch_queries = batch_queries || strcmp(argv[i], "--queries") == 0;
   if (search || from_index || batch_queries) {
      const char *list = nullptr, *query = nullptr, *save = nullptr, *index = nullptr, *add = nullptr, *queries = nullptr, *gone = nullptr;
      long top = 10, device = 0, pairs = 1, hamming = -1, min_inliers = 4, expand_images = 10;
      float tolerance = 8.0f;
      bool bad = false, verify = false, verify_options = false, query_options = false, expand = false, expand_options = false;
      for (int i = 1; i < argc && !bad; i += 2) {
         if (strcmp(argv[i], "--verify") == 0 && !verify) { verify = true; i -= 1; continue; }   // (the two options without a value)
         if (strcmp(argv[i], "--expand") == 0 && !expand) { expand = true; i -= 1; continue; }
         if (i + 1 >= argc) { bad = true; break; }
         char *end = nullptr;
         if (strcmp(argv[i], "--search") == 0 && !list) list = argv[i + 1];
         else if (strcmp(argv[i], "--query") == 0 && !query) query = argv[i + 1];
         else if (strcmp(argv[i], "--queries") == 0 && !queries) queries = argv[i + 1];
         else if (strcmp(argv[i], "--save-index") == 0 && !save) save = argv[i + 1];
         else if (strcmp(argv[i], "--index") == 0 && !index) index = argv[i + 1];
         else if (strcmp(argv[i], "--add") == 0 && !add) add = argv[i + 1];
         else if (strcmp(argv[i], "--remove") == 0 && !gone) gone = argv[i + 1];
         else if (strcmp(argv[i], "--top") == 0) { top = strtol(argv[i + 1], &end, 10); bad = end == argv[i + 1] || *end || top < 1 || top > 1024; query_options = true; }
         else if (strcmp(argv[i], "--device") == 0) { device = strtol(argv[i + 1], &end, 10); bad = end == argv[i + 1] || *end || device < 0 || device > 4095; }
         else if (strcmp(argv[i], "--hamming") == 0) { hamming = strtol(argv[i + 1], &end, 10); bad = end == argv[i + 1] || *end || hamming < 0 || hamming > HESAFF_EMBED_BITS; }
         else if (strcmp(argv[i], "--tolerance") == 0) {
            tolerance = strtof(argv[i + 1], &end);
            bad = end == argv[i + 1] || *end || !(tolerance > 0.0f && tolerance <= 1048576.0f);
            verify_options = true;
         }
         else if (strcmp(argv[i], "--min-inliers") == 0) {
            min_inliers = strtol(argv[i + 1], &end, 10);
            bad = end == argv[i + 1] || *end || min_inliers < 1 || min_inliers > 2147483647L;
            expand_options = true;
         }
         else if (strcmp(argv[i], "--expand-images") == 0) {
            expand_images = strtol(argv[i + 1], &end, 10);
            bad = end == argv[i + 1] || *end || expand_images < 1 || expand_images > 1024;
            expand_options = true;
         }
         else if (strcmp(argv[i], "--pairs") == 0) { pairs = strtol(argv[i + 1], &end, 10); bad = end == argv[i + 1] || *end || pairs < 1 || pairs > 16; verify_options = true; }
         else bad = true;
      }
      bad = bad || (verify_options && !verify) || (expand_options && !expand) || (expand && (!verify || !query));
      const ExpandOptions expand_with = {(int)min_inliers, (int)expand_images};
      if (search) {
         // one of --query, --queries and --save-index; --save-index asks no query, so it takes none of the query's options
         bad = bad || !list || index || add || gone || (query != nullptr) + (queries != nullptr) + (save != nullptr) != 1 || (save && (verify || query_options));
         if (bad) {
            fprintf(stderr, "hesaff: usage: hesaff --search <list of .hesaff.words files> --query <.hesaff.words file> | --queries <list of .hesaff.words files> [--top 1..1024] [--device D] [--hamming 0..64] "
                            "[--verify [--tolerance PX] [--pairs 1..16] [--expand [--min-inliers N] [--expand-images 1..1024]]]   or   hesaff --search <list> --save-index <index file> [--device D] [--hamming 0..64]\n");
            return 1;
         }
         return run_search_mode(list, query, (int)top, (int)device, verify, tolerance, (int)pairs, (int)hamming, save, queries, expand ? &expand_with : nullptr);
      }
      // one of --query, --queries, --add and --remove; the last two take none of the query's options
      bad = bad || !index || save || (query != nullptr) + (queries != nullptr) + (add != nullptr) + (gone != nullptr) != 1 ||
            ((add || gone) && (verify || query_options || hamming >= 0));
      if (bad) {
         fprintf(stderr, "hesaff: usage: hesaff --index <index file> --query <.hesaff.words file> | --queries <list of .hesaff.words files> [--top 1..1024] [--device D] [--hamming 0..64] "
                         "[--verify [--tolerance PX] [--pairs 1..16] [--expand [--min-inliers N] [--expand-images 1..1024]]]   or   hesaff --index <index file> --add <list of .hesaff.words files> [--device D]"
                         "   or   hesaff --index <index file> --remove <list of paths of <index file>.list> [--device D]\n");
         return 1;
      }
      return run_index_mode(index, query, add, (int)top, (int)device, verify, tolerance, (int)pairs, (int)hamming, queries, gone, expand ? &expand_with : nullptr);
   }
   bool batch = false;
   for (int i = 1; i < argc; i++) batch = batch || strcmp(argv[i], "--batch") == 0;
   if (batch) {
      const char *devices = nullptr, *list = nullptr;
      int out_format = HESAFF_OUT_TEXT, fast = 0, host_share = 1, runtime_nice = -1, max_keypoints = 0, orientation = HESAFF_ORI_UP, grid_rows = 1, grid_cols = 1, descriptor = HESAFF_DESC_SIFT, orientations = 1;
      bool bad = false, grid = false, dynamic = false, words_only = false;
      const char *vocabulary_path = nullptr, *train_path = nullptr, *cells_arg = nullptr, *embedding_path = nullptr, *train_embedding_path = nullptr;
      unsigned long long seed = 0;
      bool seed_given = false;
      int resume = 0, train_words = 0, train_iterations = 10, train_cells = 0, coarse_iterations = 10, probes = 1;
      bool probes_given = false;
      int neighbours = 1;
      bool neighbours_given = false;
      for (int i = 1; i < argc && !bad; i += 2) {
         if (strcmp(argv[i], "--resume") == 0) { resume = 1; i--; continue; }
         if (strcmp(argv[i], "--resume=strict") == 0) { resume = 2; i--; continue; }   // also count the rows of existing text outputs
         if (strcmp(argv[i], "--words-only") == 0) { words_only = true; i--; continue; }
         if (i + 1 >= argc) bad = true;
         else if (strcmp(argv[i], "--batch") == 0) list = argv[i + 1];
         else if (strcmp(argv[i], "--devices") == 0) devices = argv[i + 1];
         else if (strcmp(argv[i], "--vocabulary") == 0) vocabulary_path = argv[i + 1];
         else if (strcmp(argv[i], "--embedding") == 0) embedding_path = argv[i + 1];
         else if (strcmp(argv[i], "--train-embedding") == 0) train_embedding_path = argv[i + 1];
         else if (strcmp(argv[i], "--seed") == 0) {
            char *end = nullptr;
            seed = strtoull(argv[i + 1], &end, 10);
            if (argv[i + 1][0] < '0' || argv[i + 1][0] > '9' || *end != 0) bad = true;
            seed_given = true;
         }
         else if (strcmp(argv[i], "--train-vocabulary") == 0) train_path = argv[i + 1];
         else if (strcmp(argv[i], "--cells") == 0) cells_arg = argv[i + 1];   // a cells file, or with --train-vocabulary the number of cells
         else if (strcmp(argv[i], "--probes") == 0) {
            // one digit, 1..8 (hesaff_set_vocabulary_probes)
            if (argv[i + 1][0] < '1' || argv[i + 1][0] > '8' || argv[i + 1][1] != 0) bad = true;
            else { probes = argv[i + 1][0] - '0'; probes_given = true; }
         }
         else if (strcmp(argv[i], "--neighbours") == 0) {
            // one digit, 1..8 (hesaff_set_vocabulary_neighbours)
            if (argv[i + 1][0] < '1' || argv[i + 1][0] > '8' || argv[i + 1][1] != 0) bad = true;
            else { neighbours = argv[i + 1][0] - '0'; neighbours_given = true; }
         }
         else if (strcmp(argv[i], "--coarse-iterations") == 0) {
            char *end = nullptr;
            const long v = strtol(argv[i + 1], &end, 10);
            if (argv[i + 1][0] < '0' || argv[i + 1][0] > '9' || *end != 0 || v < 1 || v > (1L << 20)) bad = true;
            else coarse_iterations = (int)v;
         }
         else if (strcmp(argv[i], "--words") == 0 || strcmp(argv[i], "--iterations") == 0) {
            // digits only, at least 1: K up to 2^20 rows, T up to a million iterations
            char *end = nullptr;
            const long v = strtol(argv[i + 1], &end, 10);
            if (argv[i + 1][0] < '0' || argv[i + 1][0] > '9' || *end != 0 || v < 1 || v > (1L << 20)) bad = true;
            else (argv[i][2] == 'w' ? train_words : train_iterations) = (int)v;
         }
         else if (strcmp(argv[i], "--host-share") == 0) { host_share = atoi(argv[i + 1]); bad = host_share < 1 || host_share > 1024; }
         else if (strcmp(argv[i], "--runtime-nice") == 0) { runtime_nice = atoi(argv[i + 1]); bad = runtime_nice < 0 || runtime_nice > 1; }
         else if (strcmp(argv[i], "--max-keypoints") == 0) {
            // digits only: "-1", "x", "" and "12x" are refused, as is anything beyond int
            char *end = nullptr;
            const long v = strtol(argv[i + 1], &end, 10);
            if (argv[i + 1][0] < '0' || argv[i + 1][0] > '9' || *end != 0 || v > 0x7fffffffL) bad = true;
            else max_keypoints = (int)v;
         } else if (strcmp(argv[i], "--grid") == 0) {
            // <digits>x<digits>, both at least 1, at most 64 cells
            const char *a = argv[i + 1];
            char *end = nullptr, *end2 = nullptr;
            const long r = (a[0] >= '0' && a[0] <= '9') ? strtol(a, &end, 10) : 0;
            const long cc = (end && *end == 'x' && end[1] >= '0' && end[1] <= '9') ? strtol(end + 1, &end2, 10) : 0;
            if (r < 1 || cc < 1 || r > 64 || cc > 64 || r * cc > 64 || !end2 || *end2 != 0) bad = true;
            else { grid_rows = (int)r; grid_cols = (int)cc; grid = true; }
         } else if (strcmp(argv[i], "--orientation") == 0) {
            if (strcmp(argv[i + 1], "up") == 0) orientation = HESAFF_ORI_UP;
            else if (strcmp(argv[i + 1], "dominant") == 0) orientation = HESAFF_ORI_DOMINANT;
            else bad = true;
         } else if (strcmp(argv[i], "--orientations") == 0) {
            // one digit, 1..4 (hesaff_set_orientation_count; read with --orientation dominant only)
            if (argv[i + 1][0] < '1' || argv[i + 1][0] > '4' || argv[i + 1][1] != 0) bad = true;
            else orientations = argv[i + 1][0] - '0';
         } else if (strcmp(argv[i], "--descriptor") == 0) {
            if (strcmp(argv[i + 1], "sift") == 0) descriptor = HESAFF_DESC_SIFT;
            else if (strcmp(argv[i + 1], "rootsift") == 0) descriptor = HESAFF_DESC_ROOTSIFT;
            else bad = true;
         } else if (strcmp(argv[i], "--fast") == 0) {
            if (strcmp(argv[i + 1], "0") == 0 || strcmp(argv[i + 1], "2") == 0) fast = atoi(argv[i + 1]);
            else bad = true;
         } else if (strcmp(argv[i], "--schedule") == 0) {
            if (strcmp(argv[i + 1], "dynamic") == 0) dynamic = true;
            else if (strcmp(argv[i + 1], "static") != 0) bad = true;
         } else if (strcmp(argv[i], "--output") == 0) {
            if (strcmp(argv[i + 1], "text") == 0) out_format = HESAFF_OUT_TEXT;
            else if (strcmp(argv[i + 1], "bin") == 0) out_format = HESAFF_OUT_BIN;
            else if (strcmp(argv[i + 1], "both") == 0) out_format = HESAFF_OUT_TEXT | HESAFF_OUT_BIN;
            else bad = true;
         } else bad = true;
      }
      // a grid divides a budget: without --max-keypoints, or with more cells than keypoints, there is nothing to divide
      if (grid && (max_keypoints < 1 || grid_rows * grid_cols > max_keypoints)) bad = true;
      if (words_only && !vocabulary_path) bad = true;
      // training takes the list's keys and writes one vocabulary file: it needs --words, and nothing that is about per-image files
      if (train_path && (train_words < 1 || vocabulary_path || words_only || resume || dynamic || out_format != HESAFF_OUT_TEXT)) bad = true;
      if (!train_path && (train_words > 0 || train_iterations != 10 || coarse_iterations != 10)) bad = true;
      if (cells_arg && !train_path && !vocabulary_path) bad = true;
      if (embedding_path && (!vocabulary_path || train_path)) bad = true;   // signatures go with words
      // training an embedding takes the list's keys and a vocabulary and writes one embedding file: nothing that is about per-image files
      if (train_embedding_path && (!vocabulary_path || train_path || embedding_path || words_only || resume || dynamic || out_format != HESAFF_OUT_TEXT)) bad = true;
      if (seed_given && !train_embedding_path) bad = true;
      if (cells_arg && train_path) {   // digits only, 1 .. K
         char *end = nullptr;
         const long v = strtol(cells_arg, &end, 10);
         if (cells_arg[0] < '0' || cells_arg[0] > '9' || *end != 0 || v < 1 || v > train_words) bad = true;
         else train_cells = (int)v;
      }
      if (coarse_iterations != 10 && !train_cells) bad = true;
      if (probes_given && (!cells_arg || train_path)) bad = true;   // probes search a cells FILE's layer; training has one probe
      if (neighbours_given && (!vocabulary_path || train_path || train_embedding_path)) bad = true;   // neighbours are rows of a vocabulary, for per-image files
      if (bad || !list) { fprintf(stderr, "hesaff: usage: hesaff --batch <list file> [--devices 0-7|0,2|all] [--output text|bin|both] [--vocabulary <vocabulary file> [--words-only] [--embedding <embedding file>] [--train-embedding <embedding file> [--seed S]]] [--train-vocabulary <vocabulary file> --words K [--iterations T]] [--cells <cells file>|C [--coarse-iterations Tc]] [--probes 1..8] [--neighbours 1..8] [--schedule static|dynamic] [--fast 0|2] [--resume|--resume=strict] [--host-share K] [--runtime-nice 0|1] [--max-keypoints N] [--orientations 1..4] [--descriptor sift|rootsift] [--orientation up|dominant] [--grid RxC]\n"); return 1; }
      if (neighbours > 1 && cells_arg) {   // (the library's refusal, before any file is read)
         fprintf(stderr, "hesaff: --neighbours above 1 and --cells do not combine: the R nearest words are searched in the whole vocabulary\n");
         return 1;
      }
      if (train_path)
         return run_train_mode(list, devices, train_path, train_words, train_iterations, fast, max_keypoints, orientation, grid_rows, grid_cols, descriptor, orientations, train_cells,
                               coarse_iterations);
      uint8_t *vocabulary = nullptr, *cells_coarse = nullptr;
      uint32_t *cells_first = nullptr;
      int vocabulary_size = 0, cells = 0, cells_rows = 0;
      if (vocabulary_path) {   // before any image is read
         if (hesaff_read_vocabulary(vocabulary_path, &vocabulary, &vocabulary_size) != HESAFF_OK) {
            fprintf(stderr, "hesaff: cannot read vocabulary '%s' (a HESAFFV1 file with rows of 128 bytes expected)\n", vocabulary_path);
            return 1;
         }
         out_format = words_only ? HESAFF_OUT_WORDS : (out_format | HESAFF_OUT_WORDS);
      }
      if (cells_arg) {   // likewise
         if (hesaff_read_vocabulary_cells(cells_arg, &cells_coarse, &cells_first, &cells, &cells_rows) != HESAFF_OK || cells_rows != vocabulary_size) {
            fprintf(stderr, "hesaff: cannot read cells '%s' (a HESAFFC1 file over the %d rows of the vocabulary expected)\n", cells_arg, vocabulary_size);
            hesaff_free(vocabulary); hesaff_free(cells_coarse); hesaff_free(cells_first);
            return 1;
         }
      }
      int8_t *embed_P = nullptr;
      int32_t *embed_tau = nullptr;
      if (embedding_path) {   // likewise
         int embed_rows = 0;
         if (hesaff_read_embedding(embedding_path, &embed_P, &embed_tau, &embed_rows) != HESAFF_OK || embed_rows != vocabulary_size) {
            fprintf(stderr, "hesaff: cannot read embedding '%s' (a HESAFFE1 file over the %d rows of the vocabulary expected)\n", embedding_path, vocabulary_size);
            hesaff_free(vocabulary); hesaff_free(cells_coarse); hesaff_free(cells_first); hesaff_free(embed_P); hesaff_free(embed_tau);
            return 1;
         }
      }
      if (train_embedding_path) {
         const TrainEmbedding te = {vocabulary, vocabulary_size, cells_coarse, cells_first, cells, probes, (uint64_t)seed};
         const int trc = run_train_mode(list, devices, train_embedding_path, 0, 1, fast, max_keypoints, orientation, grid_rows, grid_cols, descriptor, orientations, 0, 10, &te);
         hesaff_free(vocabulary); hesaff_free(cells_coarse); hesaff_free(cells_first);
         return trc;
      }
      const int brc = run_batch_mode(list, devices, out_format, dynamic, fast, resume, host_share, runtime_nice, max_keypoints, orientation, grid_rows, grid_cols, descriptor,
                                     orientations, vocabulary, vocabulary_size, cells_coarse, cells_first, cells, probes, embed_P, embed_tau, neighbours);
      hesaff_free(vocabulary); hesaff_free(cells_coarse); hesaff_free(cells_first); hesaff_free(embed_P); hesaff_free(embed_tau);
      return brc;
   }
   if (argc > 1) {
      // --vocabulary <file> behind the image (the last one counts): read first, so that a bad file ends the run before the image is read
      uint8_t *vocabulary = nullptr;
      int vocabulary_size = 0;
      for (int i = 2; i < argc; i++) {
         if (strcmp(argv[i], "--vocabulary") != 0) continue;
         if (vocabulary) { hesaff_free(vocabulary); vocabulary = nullptr; }
         if (i + 1 >= argc) { fprintf(stderr, "hesaff: --vocabulary needs a vocabulary file\n"); return 1; }
         const char *vname = argv[++i];
         if (hesaff_read_vocabulary(vname, &vocabulary, &vocabulary_size) != HESAFF_OK) {
            fprintf(stderr, "hesaff: cannot read vocabulary '%s' (a HESAFFV1 file with rows of 128 bytes expected)\n", vname);
            return 1;
         }
      }
      struct FreeVocabulary { uint8_t *&p; ~FreeVocabulary() { hesaff_free(p); } } free_vocabulary{vocabulary};
      // --cells <file> behind the image (the last one counts): a layer over that vocabulary, read before the image as well
      uint8_t *cells_coarse = nullptr;
      uint32_t *cells_first = nullptr;
      int cells = 0;
      struct FreeCells { uint8_t *&g; uint32_t *&f; ~FreeCells() { hesaff_free(g); hesaff_free(f); } } free_cells{cells_coarse, cells_first};
      for (int i = 2; i < argc; i++) {
         if (strcmp(argv[i], "--cells") != 0) continue;
         hesaff_free(cells_coarse); hesaff_free(cells_first);
         cells_coarse = nullptr; cells_first = nullptr;
         int cells_rows = 0;
         const char *cname = i + 1 < argc ? argv[++i] : "";
         if (!vocabulary || hesaff_read_vocabulary_cells(cname, &cells_coarse, &cells_first, &cells, &cells_rows) != HESAFF_OK || cells_rows != vocabulary_size) {
            fprintf(stderr, "hesaff: cannot read cells '%s' (--vocabulary and a HESAFFC1 file over its rows expected)\n", cname);
            return 1;
         }
      }
      // --probes 1..8 behind the image (the last one counts): needs the layer of a --cells file
      int probes = 1;
      for (int i = 2; i < argc; i++) {
         if (strcmp(argv[i], "--probes") != 0) continue;
         const char *v = i + 1 < argc ? argv[++i] : "";
         if (cells_coarse && v[0] >= '1' && v[0] <= '8' && v[1] == 0) probes = v[0] - '0';
         else {
            fprintf(stderr, "hesaff: --probes takes 1 .. 8 and needs --vocabulary with --cells <cells file>\n");
            return 1;
         }
      }
      // --neighbours 1..8 behind the image (the last one counts): needs --vocabulary, and above 1 no --cells
      int neighbours = 1;
      for (int i = 2; i < argc; i++) {
         if (strcmp(argv[i], "--neighbours") != 0) continue;
         const char *v = i + 1 < argc ? argv[++i] : "";
         if (vocabulary && v[0] >= '1' && v[0] <= '8' && v[1] == 0) neighbours = v[0] - '0';
         else {
            fprintf(stderr, "hesaff: usage: hesaff <image> [--mask <mask file>] [--orientation up|dominant] [--orientations 1..4] [--descriptor sift|rootsift] [--vocabulary <vocabulary file> [--cells <cells file> [--probes 1..8]] [--neighbours 1..8]]\n");
            return 1;
         }
      }
      if (neighbours > 1 && cells_coarse) {
         fprintf(stderr, "hesaff: --neighbours above 1 and --cells do not combine: the R nearest words are searched in the whole vocabulary\n");
         return 1;
      }
      uint8_t *data = nullptr;
      int w = 0, h = 0, ch = 0;
      if (hesaff_read_image(argv[1], &data, &w, &h, &ch) != HESAFF_OK) {
         fprintf(stderr, "hesaff: cannot read '%s' (PBM / PGM / PPM, PNG, JPEG, BMP or baseline TIFF expected)\n", argv[1]);
         return 1;
      }
      // --mask <file> behind the image: refused here, before a device is touched, when it cannot serve as this image's mask
      uint8_t *mask = nullptr;
      for (int i = 2; i < argc; i++) {
         if (strcmp(argv[i], "--mask") != 0) continue;
         if (mask) { hesaff_free(mask); mask = nullptr; }   // (the last --mask counts)
         int mw = 0, mh = 0, mch = 0;
         const char *why = nullptr;
         if (i + 1 >= argc) { fprintf(stderr, "hesaff: --mask needs a mask file\n"); hesaff_free(data); return 1; }
         const char *mname = argv[++i];
         if (hesaff_read_image(mname, &mask, &mw, &mh, &mch) != HESAFF_OK) { why = "cannot be read"; mask = nullptr; }
         else if (mch != 1) why = "has three channels: a mask has one";
         else if (mw != w || mh != h) why = "is not of the image's size";
         if (why) {
            fprintf(stderr, "hesaff: mask '%s' %s", mname, why);
            if (mask && mch == 1) fprintf(stderr, " (%d x %d, the image is %d x %d)", mw, mh, w, h);
            fprintf(stderr, "\n");
            if (mask) hesaff_free(mask);
            hesaff_free(data);
            return 1;
         }
      }
      // --orientation up | dominant behind the image (the last one counts)
      int orientation = HESAFF_ORI_UP;
      for (int i = 2; i < argc; i++) {
         if (strcmp(argv[i], "--orientation") != 0) continue;
         const char *v = i + 1 < argc ? argv[++i] : "";
         if (strcmp(v, "up") == 0) orientation = HESAFF_ORI_UP;
         else if (strcmp(v, "dominant") == 0) orientation = HESAFF_ORI_DOMINANT;
         else {
            fprintf(stderr, "hesaff: --orientation takes up or dominant\n");
            hesaff_free(data);
            if (mask) hesaff_free(mask);
            return 1;
         }
      }
      // --orientations 1..4 behind the image (the last one counts; read with --orientation dominant only)
      int orientations = 1;
      for (int i = 2; i < argc; i++) {
         if (strcmp(argv[i], "--orientations") != 0) continue;
         const char *v = i + 1 < argc ? argv[++i] : "";
         if (v[0] >= '1' && v[0] <= '4' && v[1] == 0) orientations = v[0] - '0';
         else {
            fprintf(stderr, "hesaff: --orientations takes 1, 2, 3 or 4\n");
            hesaff_free(data);
            if (mask) hesaff_free(mask);
            return 1;
         }
      }
      // --descriptor sift | rootsift behind the image (the last one counts)
      int descriptor = HESAFF_DESC_SIFT;
      for (int i = 2; i < argc; i++) {
         if (strcmp(argv[i], "--descriptor") != 0) continue;
         const char *v = i + 1 < argc ? argv[++i] : "";
         if (strcmp(v, "sift") == 0) descriptor = HESAFF_DESC_SIFT;
         else if (strcmp(v, "rootsift") == 0) descriptor = HESAFF_DESC_ROOTSIFT;
         else {
            fprintf(stderr, "hesaff: usage: hesaff <image> [--mask <mask file>] [--orientation up|dominant] [--orientations 1..4] [--descriptor sift|rootsift] [--vocabulary <vocabulary file>]\n");
            hesaff_free(data);
            if (mask) hesaff_free(mask);
            return 1;
         }
      }
      try {
         hesaff_amd::HessianAffineParams par;
         hesaff_amd::AffineHessianDetector detector(par);
         if (mask) detector.setMask(mask);
         detector.setOrientation(orientation);
         detector.setOrientationCount(orientations);
         detector.setDescriptor(descriptor);
         if (vocabulary) detector.setVocabulary(vocabulary, vocabulary_size);
         if (cells_coarse) detector.setVocabularyCells(cells_coarse, cells_first, cells);
         detector.setVocabularyProbes(probes);
         detector.setVocabularyNeighbours(neighbours);
         const auto t1 = std::chrono::steady_clock::now();
         detector.detectPyramidKeypoints(data, w, h, ch);
         const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
         std::cout << "Detected " << detector.g_numberOfPoints << " keypoints and " << detector.g_numberOfAffinePoints
                   << " affine shapes in " << dt << " sec." << std::endl;
         const std::string name = std::string(argv[1]) + ".hesaff.sift";
         std::ofstream out(name.c_str());
         if (!out) { fprintf(stderr, "hesaff: cannot write '%s'\n", name.c_str()); hesaff_free(data); if (mask) hesaff_free(mask); return 1; }
         detector.exportKeypoints(out);
         if (vocabulary) detector.exportWords(std::string(argv[1]) + ".hesaff.words");
      } catch (const std::exception &e) {
         fprintf(stderr, "hesaff: %s\n", e.what());
         hesaff_free(data);
         if (mask) hesaff_free(mask);
         return 1;
      }
      hesaff_free(data);
      if (mask) hesaff_free(mask);
   } else {
      printf("\nUsage: hesaff image_name.ppm\nDetects Hessian Affine points and describes them using SIFT descriptor.\nThe detector assumes that the vertical orientation is preserved.\n\n");
   }
   return 0;
}
