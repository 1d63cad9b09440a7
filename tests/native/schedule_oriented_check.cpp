// CPU check of the group pipeline's ORIENTED stream / event order (hesaff_amd/csrc/group_schedule.h: run_group_schedule_oriented, the
// order hesaff_set_orientation(HESAFF_ORI_DOMINANT) runs; built and run by tests/test_orientation_host.py with
// g++ -fsanitize=address,undefined).  A recording device of its own turns a run of the template into a trace; the happens-before
// relation is built from the trace as tests/native/schedule_check.cpp builds it - operations of one stream are ordered, a wait is
// ordered behind the record of its event issued last before it, which must be the record of the group the wait names - and the
// conditions the order exists for are asserted of it: the upright order's, with "the patch stage" now both passes, and
//   - k_orientation(g) behind every first-pass patch kernel of g on every stream (it reads their patches, and stands in front of the
//     counter clear they still read);
//   - the re-bin behind k_orientation(g), every second-pass patch kernel of g behind both;
//   - descriptors(g) behind every second-pass patch kernel.
// Three parts: the properties for every group count 0 .. 10 under every option; the upright order untouched (a device WITHOUT the
// two new members still compiles against run_group_schedule, and the oriented trace minus its second pass is that trace, line for
// line); sensitivity (each single wait or record deleted from the overlapped 5-group traces breaks a property, but for a short list).
// Prints "schedule_oriented_check ok"; a failed check prints a message and ends the program with exit code 1.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>
#include "../../hesaff_amd/csrc/group_schedule.h"

using namespace hesaff_sched;

struct Op {
   enum Kind { WAIT, RECORD, AFFINE, PREPARE, PATCH, ORIENT, REBIN, PATCH_DONE, DESCRIPTORS, END } kind;
   Stream stream;
   Event ev;          // WAIT, RECORD
   int group, slot;   // the launches; -1: none
   int pass;          // 1, or 2 between k_orientation and the end of the group's patch stage
};

static std::string num(int v) { return v < 0 ? "-" : std::to_string(v); }
static std::string line(const Op &o)
{
   static const char *kinds[] = {"wait", "record", "affine", "prepare", "patch", "orient", "rebin", "patch_done", "descriptors", "end"};
   static const char *streams[S_COUNT] = {"main", "bin0", "bin1", "bin2", "bin3", "desc", "affine"};
   static const char *events[] = {"detect_done", "affine_done", "extract_done", "sift_done", "fork", "join"};
   static_assert(HS_NSIDE == 4, "one name per side stream");
   const bool ev = o.kind == Op::WAIT || o.kind == Op::RECORD;
   return std::string(kinds[o.kind]) + " " + streams[o.stream] + " " + (ev ? std::string(events[o.ev.kind]) + "[" + std::to_string(o.ev.index) + "]" : "-") + " " +
          num(o.group) + " " + num(o.slot);
}
static std::string describe(const Op &o) { return line(o) + " group " + num(o.ev.group) + " pass " + num(o.pass); }

// today's Device concept, and nothing more: run_group_schedule must go on compiling against it
struct PlainRecorder {
   std::vector<Op> ops;
   int pass = 1;
   void add(Op::Kind k, Stream s, int g, int slot) { ops.push_back(Op{k, s, Event{Event::DETECT_DONE, 0, -1}, g, slot, pass}); }
   void wait(Stream s, const Event &e) { ops.push_back(Op{Op::WAIT, s, e, -1, -1, pass}); }
   void record(const Event &e, Stream s) { ops.push_back(Op{Op::RECORD, s, e, -1, -1, pass}); }
   void affine(int g, Stream s) { add(Op::AFFINE, s, g, -1); }
   void patch_prepare(int g) { add(Op::PREPARE, S_MAIN, g, -1); }
   void patch_kernels(int g, int slot, int n_side)
   {
      for (int i = 0; i < HS_NSIDE; i++)
         if (patch_stream(i, n_side) != S_MAIN) add(Op::PATCH, patch_stream(i, n_side), g, slot);
      add(Op::PATCH, S_MAIN, g, slot);
   }
   void patch_done(int g) { pass = 1; add(Op::PATCH_DONE, S_MAIN, g, -1); }
   void descriptors(int g, int slot, Stream s) { add(Op::DESCRIPTORS, s, g, slot); }
};
struct OrientedRecorder : PlainRecorder {
   void orientation(int g, int slot) { pass = 2; add(Op::ORIENT, S_MAIN, g, slot); }
   void patch_rebin(int g) { add(Op::REBIN, S_MAIN, g, -1); }
};

template <class R, class RUN> static std::vector<Op> full_trace(RUN run)
{
   R r;
   r.record(ev_detect_done(), S_MAIN);
   run(r);
   r.add(Op::END, S_MAIN, -1, -1);
   return r.ops;
}
static std::vector<Op> oriented_trace(int n, const ScheduleOptions &o)
{
   return full_trace<OrientedRecorder>([&](OrientedRecorder &r) { run_group_schedule_oriented(r, n, o); });
}
static std::vector<Op> plain_trace(int n, const ScheduleOptions &o)
{
   return full_trace<PlainRecorder>([&](PlainRecorder &r) { run_group_schedule(r, n, o); });
}

// "" when every property holds of the trace, else the first that does not
static std::string check(const std::vector<Op> &ops, int n, const ScheduleOptions &o)
{
   const size_t N = ops.size();
   std::vector<std::vector<bool>> before(N, std::vector<bool>(N, false));   // before[i][j]: j happens before i
   int last_on[S_COUNT];
   for (int &l : last_on) l = -1;
   auto order = [&](size_t i, int j) {
      if (j < 0) return;
      for (size_t k = 0; k < N; k++)
         if (before[j][k]) before[i][k] = true;
      before[i][j] = true;
   };
   for (size_t i = 0; i < N; i++) {
      order(i, last_on[ops[i].stream]);
      last_on[ops[i].stream] = (int)i;
      if (ops[i].kind != Op::WAIT) continue;
      int rec = -1;
      for (size_t j = 0; j < i; j++)
         if (ops[j].kind == Op::RECORD && ops[j].ev.kind == ops[i].ev.kind && ops[j].ev.index == ops[i].ev.index) rec = (int)j;
      if (rec < 0) return describe(ops[i]) + ": no record of the event was issued before this wait";
      if (ops[rec].ev.group != ops[i].ev.group) return describe(ops[i]) + ": captured " + describe(ops[rec]);
      if (ops[rec].pass != ops[i].pass) return describe(ops[i]) + ": captured the other pass's " + describe(ops[rec]);
      order(i, rec);
   }
   std::vector<int> A(n, -1), PP(n, -1), OR(n, -1), RB(n, -1), D(n, -1);
   std::vector<std::vector<int>> PK1(n), PK2(n);
   int detect = -1, end = -1;
   for (size_t i = 0; i < N; i++) {
      const Op &p = ops[i];
      if (p.kind == Op::RECORD && p.ev.kind == Event::DETECT_DONE) detect = (int)i;
      if (p.kind == Op::END) end = (int)i;
      if (p.kind == Op::AFFINE || p.kind == Op::PREPARE || p.kind == Op::PATCH || p.kind == Op::ORIENT || p.kind == Op::REBIN || p.kind == Op::DESCRIPTORS) {
         if (p.group < 0 || p.group >= n) return line(p) + ": no such group";
         if (p.kind == Op::PATCH) { (p.pass == 1 ? PK1 : PK2)[p.group].push_back((int)i); continue; }
         std::vector<int> &one = p.kind == Op::AFFINE ? A : p.kind == Op::PREPARE ? PP : p.kind == Op::ORIENT ? OR : p.kind == Op::REBIN ? RB : D;
         if (one[p.group] >= 0) return line(p) + ": issued twice";
         one[p.group] = (int)i;
      }
   }
   if (detect < 0 || end < 0) return "the trace lacks the caller's detect-done or its end";
   auto hb = [&](int a, int b) { return before[b][a]; };   // a happens before b
   auto fail = [&](const char *what, int a, int b) { return std::string(what) + ": " + describe(ops[a]) + " is not ordered before " + describe(ops[b]); };
   const size_t per_pass = (size_t)o.n_side + 1;   // one operation per stream that runs a patch kernel
   for (int g = 0; g < n; g++) {
      if (PP[g] < 0 || OR[g] < 0 || RB[g] < 0 || D[g] < 0 || (A[g] >= 0) != o.with_affine) return "group " + std::to_string(g) + ": a stage is missing";
      if (PK1[g].size() != per_pass || PK2[g].size() != per_pass) return "group " + std::to_string(g) + ": not one patch operation per stream and pass";
      const int slot = ops[D[g]].slot;
      std::vector<int> stage = PK1[g];   // the patch stage of g: both passes' kernels on every stream, k_prepare_patch, k_orientation, the re-bin
      stage.insert(stage.end(), PK2[g].begin(), PK2[g].end());
      std::vector<int> kernels = stage;
      stage.push_back(PP[g]); stage.push_back(OR[g]); stage.push_back(RB[g]);
      for (int k : stage) {
         // reads the affine output of g (k_orientation rewrites the frames k_prepare_patch derived from it)
         if (o.with_affine && !hb(A[g], k)) return fail("affine before the patch stage", A[g], k);
         // writes the slot, or the alive flags the descriptors read: every earlier group of that slot has been described
         for (int e = 0; e < g; e++)
            if (ops[D[e]].slot == slot && !hb(D[e], k)) return fail("a slot rewritten before its descriptors are done", D[e], k);
         if (g >= HS_NSLOT && !hb(D[g - HS_NSLOT], k)) return fail("the group HS_NSLOT back not described", D[g - HS_NSLOT], k);
         if (!hb(k, D[g])) return fail("the patch stage before its descriptors", k, D[g]);
         if (!hb(k, end)) return fail("the end behind the patch stage", k, end);
         // k_prepare_patch(g + 1) clears the counters and rewrites the flags this stage uses
         if (g + 1 < n && !hb(k, PP[g + 1])) return fail("the next group's k_prepare_patch under this patch stage", k, PP[g + 1]);
      }
      if (g >= HS_NSLOT && ops[D[g - HS_NSLOT]].slot != slot) return "group " + std::to_string(g) + ": not the slot of the group HS_NSLOT back";
      for (int k : kernels)
         if (ops[k].slot != slot) return "group " + std::to_string(g) + ": patches in one slot, descriptors from another";
      if (ops[OR[g]].slot != slot) return "group " + std::to_string(g) + ": k_orientation reads another slot";
      for (int k : PK1[g]) {
         if (!hb(PP[g], k)) return fail("k_prepare_patch before the first pass's bins", PP[g], k);
         // k_orientation reads every first-pass patch; it and the clear behind it stand behind every reader of the first pass's counters
         if (!hb(k, OR[g])) return fail("first-pass patches before k_orientation", k, OR[g]);
         if (!hb(k, RB[g])) return fail("the bin counters cleared under a first-pass patch kernel", k, RB[g]);
      }
      if (!hb(PP[g], OR[g])) return fail("k_prepare_patch before k_orientation", PP[g], OR[g]);
      if (!hb(OR[g], RB[g])) return fail("k_orientation before the re-bin", OR[g], RB[g]);
      for (int k : PK2[g]) {
         if (!hb(OR[g], k)) return fail("k_orientation before the second pass", OR[g], k);
         if (!hb(RB[g], k)) return fail("the re-bin before the second pass's bins", RB[g], k);
         for (int k1 : PK1[g])   // the same slot (and the per-block T' slots of the row-streamed bins) written again
            if (!hb(k1, k)) return fail("the first pass before the second", k1, k);
      }
      for (int e = 0; e < HS_NSLOT - 1 && e < g; e++)
         if (ops[D[g - 1 - e]].slot == slot) return "group " + std::to_string(g) + ": shares its slot with a group less than HS_NSLOT back";
      if (g > 0 && !hb(D[g - 1], D[g])) return fail("one descriptor chain at a time", D[g - 1], D[g]);
      if (!hb(D[g], end)) return fail("the end behind every descriptor chain", D[g], end);
      if (o.with_affine && !hb(A[g], end)) return fail("the end behind every affine", A[g], end);
   }
   if (o.with_affine && n > 0 && !hb(detect, A[0])) return fail("affine behind detect-done", detect, A[0]);
   return "";
}

static std::string header(int n, const ScheduleOptions &o)
{
   return "# groups=" + std::to_string(n) + " overlap=" + num(o.overlap) + " sift_inside=" + num(o.sift_inside) + " with_affine=" + num(o.with_affine) +
          " side_streams=" + num(o.n_side);
}

#define CHECK(cond, ...)                                                                           \
   do {                                                                                            \
      if (!(cond)) {                                                                               \
         fprintf(stderr, "schedule_oriented_check: %s:%d: %s failed: ", __FILE__, __LINE__, #cond); \
         fprintf(stderr, __VA_ARGS__);                                                             \
         fprintf(stderr, "\n");                                                                    \
         exit(1);                                                                                  \
      }                                                                                            \
   } while (0)

static const int kSides[3] = {0, 1, HS_NSIDE};

static void check_properties_and_upright()
{
   int traces = 0;
   for (int n = 0; n <= 10; n++)
      for (int ov = 0; ov < 2; ov++)
         for (int in = 0; in < 2; in++)
            for (int wa = 0; wa < 2; wa++)
               for (int side : kSides) {
                  const ScheduleOptions o = {ov == 1, in == 1, wa == 1, side};
                  const std::vector<Op> ops = oriented_trace(n, o);
                  const std::string why = check(ops, n, o);
                  CHECK(why.empty(), "%s: %s", header(n, o).c_str(), why.c_str());
                  for (const Op &p : ops)
                     CHECK(o.overlap || p.stream == S_MAIN || (p.stream >= S_BIN0 && p.stream < S_BIN0 + side), "%s: %s", header(n, o).c_str(), line(p).c_str());
                  // the upright order is the oriented one without its second pass
                  const std::vector<Op> plain = plain_trace(n, o);
                  std::vector<Op> first;
                  for (const Op &p : ops)
                     if (p.pass == 1) first.push_back(p);
                  CHECK(first.size() == plain.size(), "%s: %zu operations outside the second pass, %zu in the upright order", header(n, o).c_str(), first.size(), plain.size());
                  for (size_t i = 0; i < plain.size(); i++)
                     CHECK(describe(first[i]) == describe(plain[i]), "%s: '%s' where the upright order has '%s'", header(n, o).c_str(), describe(first[i]).c_str(),
                           describe(plain[i]).c_str());
                  for (const Op &p : plain) CHECK(p.kind != Op::ORIENT && p.kind != Op::REBIN, "%s: the upright order launches %s", header(n, o).c_str(), line(p).c_str());
                  traces++;
               }
   CHECK(traces == 11 * 2 * 2 * 2 * 3, "%d traces", traces);
}

// Every wait and every record of the overlapped 5-group trace is needed, in both orders of submission, except these.
static const char *const kRedundant[] = {
   // the descriptor chains stand on one stream, so the main stream's final wait for the LAST chain (group 4, slot 1) covers the two before it
   "wait main sift_done[0] - - group 3 pass 1",
   "wait main sift_done[2] - - group 2 pass 1",
};

static void check_sensitivity()
{
   for (int in = 0; in < 2; in++) {
      const ScheduleOptions o = {true, in == 1, true, HS_NSIDE};
      const std::vector<Op> ops = oriented_trace(5, o);
      CHECK(check(ops, 5, o).empty(), "the complete trace");
      std::set<std::string> passed;
      int deleted = 0;
      for (size_t i = 1; i < ops.size(); i++) {   // (ops[0] is the caller's record of detect-done)
         if (ops[i].kind != Op::WAIT && ops[i].kind != Op::RECORD) continue;
         std::vector<Op> cut = ops;
         cut.erase(cut.begin() + (long)i);
         deleted++;
         if (!check(cut, 5, o).empty()) continue;
         bool listed = false;
         for (const char *r : kRedundant) listed = listed || describe(ops[i]) == r;
         CHECK(listed, "sift_inside=%d: no property fails without '%s'", in, describe(ops[i]).c_str());
         passed.insert(describe(ops[i]));
      }
      CHECK(deleted > 160, "%d deletions", deleted);
      for (const char *r : kRedundant) CHECK(passed.count(r) == 1, "sift_inside=%d: '%s' is listed as redundant and is not", in, r);
   }
}

int main()
{
   check_properties_and_upright();
   check_sensitivity();
   printf("schedule_oriented_check ok\n");
   return 0;
}
