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

// The events of the pipeline.  (kind, index) names the event object; an event of a slot or a bin is recorded again for every unit,
// and a wait sees whichever record was issued last before it.  `group` says which unit's record this record is, or this wait is
// meant to see (the group, and with an orientation count the unit v below): the device never needs it, the checker holds every wait to it.
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
   bool oriented;      // hesaff_set_orientation(HESAFF_ORI_DOMINANT): rank 0 of a group is an upright pass, the orientation kernel and a turned pass
   int K;              // hesaff_set_orientation_count: the ranks of a group, read only when oriented (otherwise 1)
};

// The two patch passes: over the frames the affine stage left (k_prepare_patch), and over frames the orientation kernel turned
// (k_prepare_patch_second).
enum Pass { PASS_UPRIGHT = 0, PASS_TURNED = 1 };

// Software pipeline over n_groups image groups, one stream per stage:
//   affine shape of group g+1 (S_AFFINE)  |  patch extraction of group g (main + side streams, latency-bound)  |  descriptor
//   kernels of the units before (S_DESC).
// The unit of the pipeline is the (group, rank) pair, v = g * K + r: K ranks per group with an orientation count, otherwise one, and
// v = g.  HS_NSLOT patch buffer slots rotate, unit v in slot v % HS_NSLOT; the events of a slot carry v.  A unit is one or two patch
// passes into its slot and one descriptor chain over it.  A pass is: pass_prepare, fork, patch_kernels, join.  Rank 0 is the upright
// pass; when oriented, the orientation kernel and a turned pass into the same slot follow it.  Rank r >= 1 is one turned pass.
// What the order has to guarantee (schedule_check.cpp asserts each of them for every trace):
//   - every pass of group g, its prepare included, and orientation(g) read the affine output of g: behind affine(g), and affine(0)
//     behind the caller's detect-done;
//   - whatever writes a slot, the bins, their counters or a rank's flags - every prepare, patch kernel and orientation kernel of a
//     unit - stands behind the descriptors of every earlier unit of that slot;
//   - pass_prepare clears the bin counters and counts anew: behind every patch kernel of the pass before on every stream, which
//     still reads them, and in front of every patch kernel of its own pass, which reads what it counted;
//   - orientation(g) reads every upright-pass patch of g: behind every kernel of that pass on every stream (the join), and in front
//     of the turned prepare, whose clear those kernels must not see; every turned pass of g, of any rank, reads the frames and flags
//     orientation(g) wrote: behind it;
//   - the descriptors of a unit read every patch of its last pass, whichever stream wrote it: extract-done is recorded behind that
//     pass's join;
//   - the one copy of the descriptor stage's intermediates (b_meanvar2, b_siftvo2) serves one unit at a time: the descriptor
//     chains stand on one stream, one behind the other in ascending v, so a region's ranks are described in order;
//   - what follows the schedule on the main stream (the pack stage) is behind every descriptor chain, patch kernel and affine.
// A pass with no live keypoint costs its launches: the host does not know the counts.
// Device:
//   wait(stream, event), record(event, stream)   every hipStreamWaitEvent / hipEventRecord of the pipeline, and no other
//   affine(g, stream)                    k_affine of group g
//   pass_prepare(g, r, pass)             main stream: the bin counters cleared, the keypoints of the pass binned - PASS_UPRIGHT (r = 0
//                                        only): k_prepare_patch over the affine output; PASS_TURNED: k_prepare_patch_second over rank
//                                        r's frames, restricted to the keypoints that have a rank r.  A unit's first prepare starts
//                                        the patch stage's timer bracket
//   patch_kernels(g, r, slot, n_side)    over rank r's frames: bin i's kernel on patch_stream(i, n_side), the rest (huge windows, or fast
//                                        mode 2's pyramid kernel) on the main stream; patches into `slot`
//   orientation(g, slot)                 main stream: the orientation kernel over the upright pass's patches in `slot` - the frames of g
//                                        turned in place, and with K > 1 the frames and flags of every rank >= 1 written
//   patch_done(g)                        main stream, behind a unit's last join: the end of the patch stage's timer bracket
//   descriptors(g, r, slot, stream)      the descriptor kernels over the patches in `slot` into rank r's descriptor rows
//
// Order of submission.  The runtime multiplexes the HIP streams of one priority onto its few hardware queues, and a process that
// has streams of its own (under PyTorch: two of the four queues) leaves a context's four streams two queues, the descriptor
// stream on the one the main stream uses.  A hardware queue runs its packets in the order they were submitted, whichever stream
// they came through, so a group's descriptor kernels, submitted behind its patch stage, stand in front of the next group's
// k_prepare_patch: there the two stages take turns (profiles/r07_notes.md).  sift_inside submits the descriptor kernels of unit
// v - 1 in the MIDDLE of unit v's first pass instead - behind its kernels and in front of the main stream's wait for the side
// streams - so that the other queue's bins run beside the descriptor chain.  They do, and each runs that much slower: the dense step
// measured 0.8 % slower that way, the photograph step 2 % faster, so the order stays.
template <class Device> void run_group_schedule(Device &dev, int n_groups, const ScheduleOptions &o)
{
   const Stream as = o.overlap ? S_AFFINE : S_MAIN, ss = o.overlap ? S_DESC : S_MAIN;
   const bool affine_events = o.overlap && o.with_affine;
   const int K = o.oriented ? o.K : 1;
   const int n_units = n_groups * K;
   if (affine_events) dev.wait(as, ev_detect_done());
   auto affine = [&](int g) {
      if (!o.with_affine) return;
      dev.affine(g, as);
      if (o.overlap) dev.record(ev_affine_done(g), as);
   };
   // the descriptor kernels of unit v, behind its patches
   auto descriptors = [&](int v) {
      const int slot = v % HS_NSLOT;
      if (o.overlap) dev.wait(ss, ev_extract_done(slot, v));
      dev.descriptors(v / K, v % K, slot, ss);
      dev.record(ev_sift_done(slot, v), ss);
   };
   // one patch pass of unit v; inside: the descriptors of v - 1 go between its kernels and its join
   auto patch_pass = [&](int v, Pass pass, bool inside) {
      dev.pass_prepare(v / K, v % K, pass);
      fork_side_streams(dev, v, o.n_side);
      dev.patch_kernels(v / K, v % K, v % HS_NSLOT, o.n_side);
      if (inside) descriptors(v - 1);
      join_side_streams(dev, v, o.n_side);
   };
   if (n_groups > 0) affine(0);
   bool slot_used[HS_NSLOT] = {};
   for (int v = 0; v < n_units; v++) {
      const int g = v / K, r = v % K, slot = v % HS_NSLOT;
      if (r == 0) {
         if (g + 1 < n_groups) affine(g + 1);
         if (affine_events) dev.wait(S_MAIN, ev_affine_done(g));
      }
      if (slot_used[slot]) dev.wait(S_MAIN, ev_sift_done(slot, v - HS_NSLOT));   // the slot's previous descriptors are finished
      patch_pass(v, r == 0 ? PASS_UPRIGHT : PASS_TURNED, v > 0 && o.sift_inside);
      if (r == 0 && o.oriented) {
         dev.orientation(g, slot);
         patch_pass(v, PASS_TURNED, false);
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

}   // namespace hesaff_sched
