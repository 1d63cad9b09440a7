// group_schedule.h -- the stream / event order of the keypoint stages: which logical stream runs which stage of which image group,
// which stream waits for which event, and when a patch slot may be written again.  No HIP here: run_group_schedule is a template over
// a device object, as run_chunk_loop (chunk_engine.h) is.  pipeline.hip follows it with an adapter that is launches and lookups;
// tests/native/schedule_check.cpp runs the same template over a recording device and checks the happens-before relation of every trace.
#pragma once
#include "plan_consts.h"

namespace hesaff_sched {

// The logical streams of a context, numbered as StreamSet (pipeline.hip) pairs them onto its four HIP streams.
enum Stream { S_MAIN = 0, S_BIN0 = 1, S_DESC = 1 + HS_NSIDE, S_AFFINE = 2 + HS_NSIDE, S_COUNT = 3 + HS_NSIDE };
inline Stream bin_stream(int i) { return (Stream)(S_BIN0 + i); }   // side stream of the patch stage's window-size bin i
// the stream bin i's patch kernel runs on when the stage forks n_side side streams: bins beyond them stay on the main stream
inline Stream patch_stream(int i, int n_side) { return i < n_side ? bin_stream(i) : S_MAIN; }

// The events of the pipeline.  (kind, index) names the event object; an event of a slot or a bin is recorded again for every group,
// and a wait sees whichever record was issued last before it.  `group` says which group's record this record is, or this wait is
// meant to see: the device never needs it, the checker holds every wait to it.
struct Event {
   enum Kind { DETECT_DONE, AFFINE_DONE, EXTRACT_DONE, SIFT_DONE, FORK, JOIN } kind;
   int index;   // AFFINE_DONE: the group; EXTRACT_DONE, SIFT_DONE: the slot; JOIN: the bin; otherwise 0
   int group;   // -1: none (DETECT_DONE, which the caller records before the schedule starts)
};
inline Event ev_detect_done() { return {Event::DETECT_DONE, 0, -1}; }
inline Event ev_affine_done(int g) { return {Event::AFFINE_DONE, g, g}; }
inline Event ev_extract_done(int slot, int g) { return {Event::EXTRACT_DONE, slot, g}; }
inline Event ev_sift_done(int slot, int g) { return {Event::SIFT_DONE, slot, g}; }
inline Event ev_fork(int g) { return {Event::FORK, 0, g}; }
inline Event ev_join(int bin, int g) { return {Event::JOIN, bin, g}; }

// The patch stage's fork onto n_side side streams and the main stream's taking them back (group g; 0: nothing to do).  What is
// enqueued between the patch kernels and the join stands, on a hardware queue the main stream shares, in front of the main stream's
// waits and not behind them.
template <class Device> void fork_side_streams(Device &dev, int g, int n_side)
{
   if (n_side > 0) dev.record(ev_fork(g), S_MAIN);
   for (int i = 0; i < n_side; i++) dev.wait(bin_stream(i), ev_fork(g));
}
template <class Device> void join_side_streams(Device &dev, int g, int n_side)
{
   for (int i = 0; i < n_side; i++) dev.record(ev_join(i, g), bin_stream(i));
   for (int i = 0; i < n_side; i++) dev.wait(S_MAIN, ev_join(i, g));
}

struct ScheduleOptions {
   bool overlap;       // false (HESAFF_OVERLAP=0, tuning build): every logical stream is the main stream, every kernel alone on the device
   bool sift_inside;   // HESAFF_SIFT_INSIDE=1 (tuning build): the other order of submission, below
   bool with_affine;   // false: the affine output is in place already, no affine stage
   int n_side;         // side streams the patch stage forks: 0, 1 (fast mode 2) or HS_NSIDE
};

// Software pipeline over n_groups image groups, one stream per stage:
//   affine shape of group g+1 (S_AFFINE)  |  patch extraction of group g (main + side streams, latency-bound)  |  descriptor
//   kernels of the groups before (S_DESC).
// HS_NSLOT patch buffer slots rotate, group g in slot g % HS_NSLOT.  What the order has to guarantee (schedule_check.cpp asserts
// each of them for every trace):
//   - the patch stage of g, k_prepare_patch included, reads the affine output of g: behind affine(g), and affine(0) behind the
//     caller's detect-done;
//   - a slot is written again only when the descriptors of the group HS_NSLOT back have read it;
//   - the descriptors of g read every patch of g, whichever stream wrote it;
//   - the one copy of the descriptor stage's intermediates (b_meanvar2, b_siftvo2) serves one group at a time: the descriptor
//     chains stand on one stream, one behind the other;
//   - patch_prepare(g) clears the bin counters: behind every patch kernel of g-1 on every stream, which still reads them, and
//     in front of every patch kernel of g, which reads what it counted;
//   - what follows the schedule on the main stream (the pack stage) is behind every descriptor chain, patch kernel and affine.
// Device:
//   wait(stream, event), record(event, stream)   every hipStreamWaitEvent / hipEventRecord of the pipeline, and no other
//   affine(g, stream)                    k_affine of group g
//   patch_prepare(g)                     main stream: the bin counters cleared, k_prepare_patch
//   patch_kernels(g, slot, n_side)       bin i's kernel on patch_stream(i, n_side), the rest (huge windows, or fast mode 2's pyramid
//                                        kernel) on the main stream; patches into `slot`
//   patch_done(g)                        main stream, behind the join: the end of the patch stage's timer bracket
//   descriptors(g, slot, stream)         the descriptor kernels of group g over the patches in `slot`
//
// Order of submission.  The runtime multiplexes the HIP streams of one priority onto its few hardware queues, and a process that
// has streams of its own (under PyTorch: two of the four queues) leaves a context's four streams two queues, the descriptor
// stream on the one the main stream uses.  A hardware queue runs its packets in the order they were submitted, whichever stream
// they came through, so a group's descriptor kernels, submitted behind its patch stage, stand in front of the next group's
// k_prepare_patch: there the two stages take turns (profiles/r07_notes.md).  sift_inside submits the descriptor kernels of group
// g - 1 in the MIDDLE of group g's patch stage instead - behind its kernels and in front of the main stream's wait for the side
// streams - so that the other queue's bins run beside the descriptor chain.  They do, and each runs that much slower: the dense step
// measured 0.8 % slower that way, the photograph step 2 % faster, so the order stays.
//
// The oriented order (ORIENTED, hesaff_set_orientation: run_group_schedule_oriented below) runs the patch stage of a group twice, and
// asks two more launches of the device, both on the main stream:
//   orientation(g, slot)                 k_orientation over the first pass's patches in `slot`: the affine frames of g turned in place
//   patch_rebin(g)                       the bin counters cleared again, k_prepare_patch_second over the turned frames
// between the first pass's join and a second fork / patch_kernels / join into the same slot.  What it adds to the guarantees:
//   - orientation(g) reads every first-pass patch of g and stands in front of the counter clear those kernels still read: behind
//     every first-pass patch kernel on every stream (the join);
//   - every second-pass patch kernel reads the turned frames and what patch_rebin(g) counted: behind both;
//   - the descriptors of g read the second pass's patches: extract-done is recorded behind the second join.
// With the form PLAIN nothing of this is instantiated: the device needs neither member, and the sequence is the one above.
//
// The peaks order (PEAKS, hesaff_set_orientation_count K > 1: run_group_schedule_peaks below) gives a group K rank passes.  The unit
// of the pipeline is the (group, rank) pair, virtual index v = g * K + r, in slot v % HS_NSLOT; the events of a slot carry v where the
// other orders carry g.  Rank 0 of a group is the oriented order's patch stage - pass one, the orientation kernel and rank 0's pass in one
// slot - and each rank r >= 1 is one more patch pass into the next slot and one more descriptor chain.  It asks of the device, besides the
// oriented order's members (orientation(g, slot) being the multi form, which also writes the frames and flags of every rank >= 1):
//   rank_prepare(g, r)                      main stream: the bin counters cleared, k_prepare_patch_second over rank r's frames, restricted
//                                           to the keypoints that have a rank r; the start of the pass's timer bracket
//   rank_patch_kernels(g, r, slot, n_side)  patch_kernels over rank r's frames and bins, patches into `slot`
//   rank_descriptors(g, r, slot, stream)    the descriptor kernels over `slot` into rank r's descriptor rows (r = 0: descriptors(g, ..))
// What it adds to the guarantees (tests/native/schedule_peaks_check.cpp):
//   - rank_prepare(g, r) reads the frames and flags orientation(g) wrote, and clears the counters the pass before still reads: behind
//     orientation(g) and behind every patch kernel of the pair before on every stream;
//   - the patch kernels of (g, r) read what rank_prepare(g, r) counted, and write a slot the descriptors of the pair HS_NSLOT back
//     have finished with;
//   - the descriptors of (g, r) read every patch of (g, r); the chains stand on one stream in ascending v, so a region's ranks are
//     described in order and the one copy of the intermediates serves one pair at a time;
//   - the main stream ends behind the last chain of every slot.
// A pass with no live keypoint costs its launches: the host does not know the counts.
enum Form { PLAIN = 0, ORIENTED = 1, PEAKS = 2 };
template <int FORM, class Device> void run_group_schedule_as(Device &dev, int n_groups, const ScheduleOptions &o, int K = 1)
{
   const Stream as = o.overlap ? S_AFFINE : S_MAIN, ss = o.overlap ? S_DESC : S_MAIN;
   const bool affine_events = o.overlap && o.with_affine;
   if constexpr (FORM != PEAKS) K = 1;
   const int n_units = n_groups * K;
   if (affine_events) dev.wait(as, ev_detect_done());
   auto affine = [&](int g) {
      if (!o.with_affine) return;
      dev.affine(g, as);
      if (o.overlap) dev.record(ev_affine_done(g), as);
   };
   // the descriptor kernels of unit v (group v / K, rank v % K), behind its patches
   auto descriptors = [&](int v) {
      const int slot = v % HS_NSLOT;
      if (o.overlap) dev.wait(ss, ev_extract_done(slot, v));
      if constexpr (FORM == PEAKS) {
         if (v % K) dev.rank_descriptors(v / K, v % K, slot, ss);
         else dev.descriptors(v / K, slot, ss);
      } else {
         dev.descriptors(v, slot, ss);
      }
      dev.record(ev_sift_done(slot, v), ss);
   };
   if (n_groups > 0) affine(0);
   bool slot_used[HS_NSLOT] = {};
   for (int v = 0; v < n_units; v++) {
      const int g = v / K, r = v % K;
      if (r == 0) {
         if (g + 1 < n_groups) affine(g + 1);
         if (affine_events) dev.wait(S_MAIN, ev_affine_done(g));
      }
      const int slot = v % HS_NSLOT;
      if (slot_used[slot]) dev.wait(S_MAIN, ev_sift_done(slot, v - HS_NSLOT));   // the slot's previous descriptors are finished
      if (r == 0) {
         dev.patch_prepare(g);
         fork_side_streams(dev, v, o.n_side);
         dev.patch_kernels(g, slot, o.n_side);
         if (v > 0 && o.sift_inside) descriptors(v - 1);
         join_side_streams(dev, v, o.n_side);
         if constexpr (FORM != PLAIN) {
            dev.orientation(g, slot);
            dev.patch_rebin(g);
            fork_side_streams(dev, v, o.n_side);
            dev.patch_kernels(g, slot, o.n_side);
            join_side_streams(dev, v, o.n_side);
         }
      } else if constexpr (FORM == PEAKS) {
         dev.rank_prepare(g, r);
         fork_side_streams(dev, v, o.n_side);
         dev.rank_patch_kernels(g, r, slot, o.n_side);
         if (o.sift_inside) descriptors(v - 1);
         join_side_streams(dev, v, o.n_side);
      }
      dev.patch_done(g);
      dev.record(ev_extract_done(slot, v), S_MAIN);
      slot_used[slot] = true;
      if (!o.sift_inside) descriptors(v);
   }
   if (n_units > 0 && o.sift_inside) descriptors(n_units - 1);
   for (int sl = 0; sl < HS_NSLOT; sl++)
      if (slot_used[sl]) dev.wait(S_MAIN, ev_sift_done(sl, (n_units - 1 - sl) / HS_NSLOT * HS_NSLOT + sl));   // the slot's last unit
}
template <class Device> void run_group_schedule(Device &dev, int n_groups, const ScheduleOptions &o) { run_group_schedule_as<PLAIN>(dev, n_groups, o); }
template <class Device> void run_group_schedule_oriented(Device &dev, int n_groups, const ScheduleOptions &o) { run_group_schedule_as<ORIENTED>(dev, n_groups, o); }
template <class Device> void run_group_schedule_peaks(Device &dev, int n_groups, int K, const ScheduleOptions &o) { run_group_schedule_as<PEAKS>(dev, n_groups, o, K); }

}   // namespace hesaff_sched
