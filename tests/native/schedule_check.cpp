// CPU check of the group pipeline's stream / event order (hesaff_amd/csrc/group_schedule.h; built and run by tests/test_group_schedule.py
// with g++ -fsanitize=address,undefined).  A recording device turns a run of run_group_schedule - the template pipeline.hip runs - into a
// trace of operations; from the trace the happens-before relation is built, and the conditions the order exists for are asserted of it.
//   - operations of one stream are ordered;
//   - a wait is ordered behind the record of its event that was issued last before it in host order (what a HIP stream wait sees), and
//     behind nothing else; a wait with no earlier record is a failure, and so is one that sees the record of another group than it names.
// Three parts: the properties for every group count 0 .. 10 under every option; sensitivity (each single wait or record deleted from
// the overlapped 5-group traces must break a property, but for a short list of redundant ones); and equality, line for line, with the
// sequences of the code this header replaced (tests/golden/group_schedule_parent.txt, the path in argv[1]).
// Prints "schedule_check ok"; a failed check prints a message and ends the program with exit code 1.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <set>
#include <string>
#include <vector>
#include "../../hesaff_amd/csrc/group_schedule.h"

using namespace hesaff_sched;

struct Op {
   enum Kind { WAIT, RECORD, AFFINE, PREPARE, PATCH, PATCH_DONE, DESCRIPTORS, END } kind;
   Stream stream;
   Event ev;          // WAIT, RECORD
   int group, slot;   // the launches; -1: none
};

static const char *stream_name(Stream s)
{
   static const char *names[S_COUNT] = {"main", "bin0", "bin1", "bin2", "bin3", "desc", "affine"};
   static_assert(HS_NSIDE == 4, "one name per side stream");
   return names[s];
}
static std::string event_name(const Event &e)
{
   static const char *names[] = {"detect_done", "affine_done", "extract_done", "sift_done", "fork", "join"};
   std::string n = names[e.kind];
   if (e.kind != Event::DETECT_DONE && e.kind != Event::FORK) n += "[" + std::to_string(e.index) + "]";
   return n;
}
static std::string num(int v) { return v < 0 ? "-" : std::to_string(v); }
// one line per operation: kind, stream, event, group, slot - what the sequence of HIP calls determines (the group a record or a wait
// is meant for is the header's claim, not the sequence's: it is held against the captured record below, and not printed here)
static std::string line(const Op &o)
{
   static const char *kinds[] = {"wait", "record", "affine", "prepare", "patch", "patch_done", "descriptors", "end"};
   const bool ev = o.kind == Op::WAIT || o.kind == Op::RECORD;
   return std::string(kinds[o.kind]) + " " + stream_name(o.stream) + " " + (ev ? event_name(o.ev) : "-") + " " + num(o.group) + " " + num(o.slot);
}
static std::string describe(const Op &o) { return line(o) + " group " + num(o.ev.group); }   // names a wait or a record of one trace uniquely

struct Recorder {
   std::vector<Op> ops;
   void add(Op::Kind k, Stream s, int g, int slot) { ops.push_back(Op{k, s, Event{Event::DETECT_DONE, 0, -1}, g, slot}); }
   void wait(Stream s, const Event &e) { ops.push_back(Op{Op::WAIT, s, e, -1, -1}); }
   void record(const Event &e, Stream s) { ops.push_back(Op{Op::RECORD, s, e, -1, -1}); }
   void affine(int g, Stream s) { add(Op::AFFINE, s, g, -1); }
   void patch_prepare(int g) { add(Op::PREPARE, S_MAIN, g, -1); }
   // one operation per stream that runs a patch kernel: every bin's, and the main stream (huge windows / fast mode 2's pyramid kernel)
   void patch_kernels(int g, int slot, int n_side)
   {
      for (int i = 0; i < HS_NSIDE; i++)
         if (patch_stream(i, n_side) != S_MAIN) add(Op::PATCH, patch_stream(i, n_side), g, slot);
      add(Op::PATCH, S_MAIN, g, slot);
   }
   void patch_done(int g) { add(Op::PATCH_DONE, S_MAIN, g, -1); }
   void descriptors(int g, int slot, Stream s) { add(Op::DESCRIPTORS, s, g, slot); }
};

// The caller's part around the schedule: detect-done recorded on the main stream before it, and whatever follows on the main stream.
static std::vector<Op> full_trace(int n, const ScheduleOptions &o)
{
   Recorder r;
   r.record(ev_detect_done(), S_MAIN);
   run_group_schedule(r, n, o);
   r.add(Op::END, S_MAIN, -1, -1);
   return r.ops;
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
      order(i, rec);
   }
   // the operations by group
   std::vector<int> A(n, -1), PP(n, -1), D(n, -1);
   std::vector<std::vector<int>> PK(n);
   int detect = -1, end = -1;
   for (size_t i = 0; i < N; i++) {
      const Op &p = ops[i];
      if (p.kind == Op::RECORD && p.ev.kind == Event::DETECT_DONE) detect = (int)i;
      if (p.kind == Op::END) end = (int)i;
      if (p.kind == Op::AFFINE || p.kind == Op::PREPARE || p.kind == Op::PATCH || p.kind == Op::DESCRIPTORS) {
         if (p.group < 0 || p.group >= n) return line(p) + ": no such group";
         std::vector<int> &one = p.kind == Op::AFFINE ? A : p.kind == Op::PREPARE ? PP : D;
         if (p.kind == Op::PATCH) PK[p.group].push_back((int)i);
         else if (one[p.group] >= 0) return line(p) + ": issued twice";
         else one[p.group] = (int)i;
      }
   }
   if (detect < 0 || end < 0) return "the trace lacks the caller's detect-done or its end";
   auto hb = [&](int a, int b) { return before[b][a]; };   // a happens before b
   auto fail = [&](const char *what, int a, int b) { return std::string(what) + ": " + line(ops[a]) + " is not ordered before " + line(ops[b]); };
   for (int g = 0; g < n; g++) {
      if (PP[g] < 0 || D[g] < 0 || PK[g].empty() || (A[g] >= 0) != o.with_affine) return "group " + std::to_string(g) + ": a stage is missing";
      std::vector<int> stage = PK[g];   // the patch stage of g: its kernels on every stream and k_prepare_patch
      stage.push_back(PP[g]);
      for (int k : stage) {
         // reads the affine output of g
         if (o.with_affine && !hb(A[g], k)) return fail("affine before the patch stage", A[g], k);
         // writes the slot (k_prepare_patch: the alive flags the descriptors read): every earlier group of that slot has been described -
         // the group HS_NSLOT back, and with it (the chain below) those before
         for (int e = 0; e < g; e++)
            if (ops[D[e]].slot == ops[PK[g][0]].slot && !hb(D[e], k)) return fail("a slot rewritten before its descriptors are done", D[e], k);
         if (g >= HS_NSLOT && !hb(D[g - HS_NSLOT], k)) return fail("the group HS_NSLOT back not described", D[g - HS_NSLOT], k);
      }
      if (g >= HS_NSLOT && ops[D[g - HS_NSLOT]].slot != ops[PK[g][0]].slot) return "group " + std::to_string(g) + ": not the slot of the group HS_NSLOT back";
      for (int k : PK[g]) {
         if (ops[k].slot != ops[D[g]].slot) return "group " + std::to_string(g) + ": patches in one slot, descriptors from another";
         // the descriptors of g read every patch of g; the bins read what k_prepare_patch(g) counted
         if (!hb(k, D[g])) return fail("patches before their descriptors", k, D[g]);
         if (!hb(PP[g], k)) return fail("k_prepare_patch before the bins", PP[g], k);
         // k_prepare_patch(g + 1) clears the counters the patch kernels of g read
         if (g + 1 < n && !hb(k, PP[g + 1])) return fail("the bin counters cleared under a patch kernel", k, PP[g + 1]);
         if (!hb(k, end)) return fail("the end behind every patch kernel", k, end);
      }
      for (int e = 0; e < HS_NSLOT - 1 && e < g; e++)   // HS_NSLOT slots in rotation: the groups alive together have slots of their own
         if (ops[D[g - 1 - e]].slot == ops[D[g]].slot) return "group " + std::to_string(g) + ": shares its slot with a group less than HS_NSLOT back";
      // one copy of the descriptor stage's intermediates
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

#define CHECK(cond, ...)                                                                  \
   do {                                                                                   \
      if (!(cond)) {                                                                      \
         fprintf(stderr, "schedule_check: %s:%d: %s failed: ", __FILE__, __LINE__, #cond); \
         fprintf(stderr, __VA_ARGS__);                                                    \
         fprintf(stderr, "\n");                                                           \
         exit(1);                                                                         \
      }                                                                                   \
   } while (0)

static const int kSides[3] = {0, 1, HS_NSIDE};

static void check_properties()
{
   int traces = 0;
   for (int n = 0; n <= 10; n++)
      for (int ov = 0; ov < 2; ov++)
         for (int in = 0; in < 2; in++)
            for (int wa = 0; wa < 2; wa++)
               for (int side : kSides) {
                  const ScheduleOptions o = {ov == 1, in == 1, wa == 1, side};
                  const std::vector<Op> ops = full_trace(n, o);
                  const std::string why = check(ops, n, o);
                  CHECK(why.empty(), "%s: %s", header(n, o).c_str(), why.c_str());
                  // without overlap every logical stream is the main stream (the side streams are the caller's choice: the library forks none then)
                  for (const Op &p : ops)
                     CHECK(o.overlap || p.stream == S_MAIN || (p.stream >= S_BIN0 && p.stream < S_BIN0 + side), "%s: %s", header(n, o).c_str(), line(p).c_str());
                  traces++;
               }
   CHECK(traces == 11 * 2 * 2 * 2 * 3, "%d traces", traces);
}

// The checker bites: every wait and every record of the overlapped 5-group trace is needed, in both orders of submission, except these.
// (The schedule issues them all the same: this pull-request-sized list is a finding, not a licence.)
static const char *const kRedundant[] = {
   // the descriptor chains stand on one stream, so the main stream's final wait for the LAST chain (group 4, slot 1) covers the two before it
   "wait main sift_done[0] - - group 3",   // the final wait for slot 0: group 3's chain is in front of group 4's on the descriptor stream
   "wait main sift_done[2] - - group 2",   // the final wait for slot 2: group 2's chain likewise
};

static void check_sensitivity()
{
   for (int in = 0; in < 2; in++) {
      const ScheduleOptions o = {true, in == 1, true, HS_NSIDE};
      const std::vector<Op> ops = full_trace(5, o);
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
      CHECK(deleted > 80, "%d deletions", deleted);
      for (const char *r : kRedundant) CHECK(passed.count(r) == 1, "sift_inside=%d: '%s' is listed as redundant and is not", in, r);
   }
}

// tests/golden/group_schedule_parent.txt: what the code before this header issued, one section per group count and option set
static void check_parent(const char *path)
{
   std::ifstream f(path);
   CHECK(f.good(), "cannot read %s", path);
   std::map<std::string, std::string> sections;
   std::string l, cur;
   while (std::getline(f, l)) {
      if (!l.empty() && l[0] == '#') { cur = l; CHECK(sections.count(cur) == 0, "%s twice", cur.c_str()); sections[cur] = ""; }
      else { CHECK(!cur.empty(), "a line before the first section"); sections[cur] += l + "\n"; }
   }
   const int counts[5] = {0, 1, 2, 4, 5};
   size_t compared = 0;
   for (int n : counts)
      for (int ov = 0; ov < 2; ov++)
         for (int in = 0; in < 2; in++)
            for (int wa = 0; wa < 2; wa++)
               for (int side : kSides) {
                  // the parent chose the side streams by the overlap switch: none without overlap, 1 (fast mode 2) or HS_NSIDE with it
                  if ((side == 0) != (ov == 0)) continue;
                  const ScheduleOptions o = {ov == 1, in == 1, wa == 1, side};
                  const std::string h = header(n, o);
                  CHECK(sections.count(h) == 1, "no section '%s'", h.c_str());
                  const std::vector<Op> ops = full_trace(n, o);
                  std::string text;
                  for (size_t i = 1; i + 1 < ops.size(); i++) text += line(ops[i]) + "\n";   // without the caller's two
                  CHECK(text == sections[h], "%s differs from the parent:\n%s--- parent:\n%s", h.c_str(), text.c_str(), sections[h].c_str());
                  compared++;
               }
   CHECK(compared == 60 && sections.size() == 60, "%zu sections compared of %zu", compared, sections.size());
}

int main(int argc, char **argv)
{
   CHECK(argc == 2, "usage: schedule_check tests/golden/group_schedule_parent.txt");
   check_properties();
   check_sensitivity();
   check_parent(argv[1]);
   printf("schedule_check ok\n");
   return 0;
}
