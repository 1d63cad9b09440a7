// CPU check of the group pipeline's stream / event order (hesaff_amd/csrc/group_schedule.h; built and run by tests/schedule_native.py
// with g++ -fsanitize=address,undefined).  A recording device turns a run of run_group_schedule - the template pipeline.hip runs - into a
// trace of operations; from the trace the happens-before relation is built, and the conditions the order exists for are asserted of it.
//   - operations of one stream are ordered;
//   - a wait is ordered behind the record of its event that was issued last before it in host order (what a HIP stream wait sees), and
//     behind nothing else; a wait with no earlier record is a failure, and so is one that sees another record than the one it names.
// The relation is transitive, so what follows from two asserted orderings is not asserted again.
// usage: schedule_check <tests/golden> [upright | oriented | peaks]; without a part, all three.  Each part has: the properties for
// every group count under every option; sensitivity (each single wait or record deleted from overlapped traces must break a property,
// but for the final waits the last chain covers); and equality, line for line, with recorded sequences: the upright order's with those
// of the code the header replaced (group_schedule_parent.txt), the oriented order's and the orientation counts' with those of the three
// forms the header had before it was one schedule over passes (group_schedule_oriented_parent.txt).
// Prints "schedule_check ok"; a failed check prints a message and ends the program with exit code 1.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <string>
#include <vector>
#include "../../hesaff_amd/csrc/group_schedule.h"

using namespace hesaff_sched;

struct Op {
   enum Kind { WAIT, RECORD, AFFINE, PREPARE, PATCH, ORIENT, PATCH_DONE, DESCRIPTORS, END } kind;
   Stream stream;
   Event ev;                // WAIT, RECORD
   int group, rank, slot;   // the launches; -1: none
   int pass;                // PREPARE, PATCH: PASS_UPRIGHT or PASS_TURNED; -1 otherwise
   int seq;                 // counts the patch passes: a fork or join wait must see the record of its own pass
};

static std::string num(int v) { return v < 0 ? "-" : std::to_string(v); }
// One line per operation - a wait or a record: kind, stream, event; a launch: kind, stream, group, rank, slot, pass - what the sequence
// of HIP calls determines (the unit a record or a wait is meant for is the header's claim, not the sequence's: it is held against the
// captured record below, and not printed here).
// parent_format: the line format of group_schedule_parent.txt - kind, stream, event, group, slot - which knows neither ranks nor passes.
static std::string line(const Op &o, bool parent_format = false)
{
   static const char *kinds[] = {"wait", "record", "affine", "prepare", "patch", "orient", "patch_done", "descriptors", "end"};
   static const char *streams[S_COUNT] = {"main", "bin0", "bin1", "bin2", "bin3", "desc", "affine"};
   static const char *events[] = {"detect_done", "affine_done", "extract_done", "sift_done", "fork", "join"};
   static_assert(HS_NSIDE == 4, "one name per side stream");
   const std::string head = std::string(kinds[o.kind]) + " " + streams[o.stream] + " ";
   if (o.kind == Op::WAIT || o.kind == Op::RECORD) {
      std::string ev = events[o.ev.kind];
      if (o.ev.kind != Event::DETECT_DONE && o.ev.kind != Event::FORK) ev += "[" + std::to_string(o.ev.index) + "]";
      return head + ev + (parent_format ? " - -" : "");
   }
   if (parent_format) return head + "- " + num(o.group) + " " + num(o.slot);
   return head + num(o.group) + " " + num(o.rank) + " " + num(o.slot) + " " + (o.pass < 0 ? "-" : o.pass == PASS_UPRIGHT ? "up" : "turned");
}
static std::string describe(const Op &o) { return line(o) + " names " + num(o.ev.group); }   // names a wait or a record of one trace uniquely

struct Recorder {
   std::vector<Op> ops;
   int pass = -1, seq = 0;   // the patch pass in progress
   void add(Op::Kind k, Stream s, int g, int r, int slot, int p = -1) { ops.push_back(Op{k, s, ev_detect_done(), g, r, slot, p, seq}); }
   void wait(Stream s, const Event &e) { ops.push_back(Op{Op::WAIT, s, e, -1, -1, -1, -1, seq}); }
   void record(const Event &e, Stream s) { ops.push_back(Op{Op::RECORD, s, e, -1, -1, -1, -1, seq}); }
   void affine(int g, Stream s) { add(Op::AFFINE, s, g, -1, -1); }
   void pass_prepare(int g, int r, Pass p)
   {
      pass = p;
      seq++;
      add(Op::PREPARE, S_MAIN, g, r, -1, p);
   }
   // one operation per stream that runs a patch kernel: every bin's, and the main stream (huge windows / fast mode 2's pyramid kernel)
   void patch_kernels(int g, int r, int slot, int n_side)
   {
      for (int i = 0; i < HS_NSIDE; i++)
         if (patch_stream(i, n_side) != S_MAIN) add(Op::PATCH, patch_stream(i, n_side), g, r, slot, pass);
      add(Op::PATCH, S_MAIN, g, r, slot, pass);
   }
   void orientation(int g, int slot) { add(Op::ORIENT, S_MAIN, g, 0, slot); }
   void patch_done(int g) { add(Op::PATCH_DONE, S_MAIN, g, -1, -1); }
   void descriptors(int g, int r, int slot, Stream s) { add(Op::DESCRIPTORS, s, g, r, slot); }
};

// The caller's part around the schedule: detect-done recorded on the main stream before it, and whatever follows on the main stream.
static std::vector<Op> full_trace(int n, const ScheduleOptions &o)
{
   Recorder r;
   r.record(ev_detect_done(), S_MAIN);
   run_group_schedule(r, n, o);
   r.add(Op::END, S_MAIN, -1, -1, -1);
   return r.ops;
}

struct PassOps {
   int prepare = -1;
   std::vector<int> kernels;
};

// "" when every property holds of the trace, else the first that does not
static std::string check(const std::vector<Op> &ops, int n, const ScheduleOptions &o)
{
   const size_t N = ops.size();
   const int K = o.oriented ? o.K : 1, units = n * K;
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
      if ((ops[i].ev.kind == Event::FORK || ops[i].ev.kind == Event::JOIN) && ops[rec].seq != ops[i].seq)
         return describe(ops[i]) + ": captured another pass's " + describe(ops[rec]);
      order(i, rec);
   }
   // The operations by group, unit and pass.  A group's passes in order: rank 0's upright pass, its turned pass when oriented, then
   // one turned pass per rank >= 1.
   const int per_group = K + (o.oriented ? 1 : 0);
   auto pass_of = [&](int v, int pass) { return v / K * per_group + (v % K == 0 ? pass : v % K + 1); };
   auto first_pass = [&](int v) { return pass_of(v, v % K == 0 ? PASS_UPRIGHT : PASS_TURNED); };
   std::vector<int> A(n, -1), OR(n, -1), D(units, -1);
   std::vector<PassOps> P((size_t)n * per_group);
   int detect = -1, end = -1;
   for (size_t i = 0; i < N; i++) {
      const Op &p = ops[i];
      if (p.kind == Op::RECORD && p.ev.kind == Event::DETECT_DONE) detect = (int)i;
      if (p.kind == Op::END) end = (int)i;
      if (p.kind == Op::WAIT || p.kind == Op::RECORD || p.kind == Op::END || p.kind == Op::PATCH_DONE) continue;
      if (p.group < 0 || p.group >= n) return line(p) + ": no such group";
      if (p.kind == Op::PATCH) {
         if (p.pass < 0 || p.rank < 0 || p.rank >= K || (p.pass == PASS_TURNED ? !o.oriented : p.rank != 0)) return line(p) + ": no such pass";
         P[pass_of(p.group * K + p.rank, p.pass)].kernels.push_back((int)i);
         continue;
      }
      int *one = nullptr;
      if (p.kind == Op::AFFINE) one = &A[p.group];
      else if (p.kind == Op::ORIENT) {
         if (!o.oriented) return line(p) + ": the upright order launches it";
         one = &OR[p.group];
      } else {
         if (p.rank < 0 || p.rank >= K) return line(p) + ": no such rank";
         if (p.kind == Op::PREPARE && (p.pass == PASS_TURNED ? !o.oriented : p.rank != 0)) return line(p) + ": no such pass";
         one = p.kind == Op::PREPARE ? &P[pass_of(p.group * K + p.rank, p.pass)].prepare : &D[p.group * K + p.rank];
      }
      if (*one >= 0) return line(p) + ": issued twice";
      *one = (int)i;
   }
   if (detect < 0 || end < 0) return "the trace lacks the caller's detect-done or its end";
   auto hb = [&](int a, int b) { return before[b][a]; };   // a happens before b
   auto fail = [&](const char *what, int a, int b) { return std::string(what) + ": " + describe(ops[a]) + " is not ordered before " + describe(ops[b]); };
   const size_t per_pass = (size_t)o.n_side + 1;   // one operation per stream that runs a patch kernel
   for (int v = 0; v < units; v++) {
      const int g = v / K, r = v % K, slot = v % HS_NSLOT;   // (HS_NSLOT slots in rotation: the units alive together have slots of their own)
      const std::string name = "group " + std::to_string(g) + " rank " + std::to_string(r);
      const bool two = r == 0 && o.oriented;   // the unit has an upright pass, the orientation kernel and a turned pass
      const PassOps &first = P[first_pass(v)], &last = P[first_pass(v) + (two ? 1 : 0)];
      if (D[v] < 0 || first.prepare < 0 || last.prepare < 0 || first.kernels.size() != per_pass || last.kernels.size() != per_pass)
         return name + ": a stage is missing, or not one patch operation per stream and pass";
      if (r == 0 && ((A[g] >= 0) != o.with_affine || (OR[g] >= 0) != o.oriented)) return name + ": a stage is missing";
      // everything of the unit that writes the slot, the bins, their counters or a rank's flags
      std::vector<int> stage = first.kernels;
      stage.push_back(first.prepare);
      if (two) {
         stage.insert(stage.end(), last.kernels.begin(), last.kernels.end());
         stage.push_back(last.prepare);
         stage.push_back(OR[g]);
      }
      if (ops[D[v]].slot != slot) return name + ": descriptors not from slot v % HS_NSLOT";
      for (int k : stage)
         if (ops[k].slot >= 0 && ops[k].slot != slot) return name + ": " + line(ops[k]) + " not in slot v % HS_NSLOT";
      const int next_prepare = v + 1 < units ? P[first_pass(v + 1)].prepare : -1;
      for (int k : stage) {
         // reads the affine output of g (the orientation kernel rewrites the frames k_prepare_patch derived from it)
         if (o.with_affine && !hb(A[g], k)) return fail("affine before the patch stage", A[g], k);
         for (int e = slot; e < v; e += HS_NSLOT)
            if (!hb(D[e], k)) return fail("a slot rewritten before its descriptors are done", D[e], k);
         // the descriptors of the unit read every patch of its last pass, and the flags its prepares wrote
         if (!hb(k, D[v])) return fail("the patch stage before its descriptors", k, D[v]);
         if (!hb(k, end)) return fail("the end behind the patch stage", k, end);
         // the next unit's prepare clears the counters and rewrites the flags this stage uses
         if (next_prepare >= 0 && !hb(k, next_prepare)) return fail("the next unit's prepare under this patch stage", k, next_prepare);
      }
      for (const PassOps *p : {&first, &last})
         for (int k : p->kernels)
            if (!hb(p->prepare, k)) return fail("a pass's prepare before its bins", p->prepare, k);
      if (two) {
         for (int k : first.kernels) {
            // the orientation kernel reads every upright-pass patch; it and the clear behind it stand behind every reader of that pass's counters
            if (!hb(k, OR[g])) return fail("upright-pass patches before the orientation kernel", k, OR[g]);
            if (!hb(k, last.prepare)) return fail("the bin counters cleared under an upright-pass patch kernel", k, last.prepare);
         }
         if (!hb(first.prepare, OR[g])) return fail("k_prepare_patch before the orientation kernel", first.prepare, OR[g]);
      }
      if (o.oriented) {   // every turned pass of g reads the frames and flags orientation(g) wrote
         if (!hb(OR[g], last.prepare)) return fail("the orientation kernel before a turned prepare", OR[g], last.prepare);
         for (int k : last.kernels)
            if (!hb(OR[g], k)) return fail("the orientation kernel before a turned pass", OR[g], k);
      }
      // one copy of the descriptor stage's intermediates
      if (v > 0 && !hb(D[v - 1], D[v])) return fail("one descriptor chain at a time, in ascending rank", D[v - 1], D[v]);
      if (!hb(D[v], end)) return fail("the end behind every descriptor chain", D[v], end);
      if (o.with_affine && !hb(A[g], end)) return fail("the end behind every affine", A[g], end);
   }
   if (o.with_affine && n > 0 && !hb(detect, A[0])) return fail("affine behind detect-done", detect, A[0]);
   return "";
}

static std::string header(int n, const ScheduleOptions &o, bool parent_format = false)
{
   return "# groups=" + std::to_string(n) + (parent_format ? "" : " oriented=" + num(o.oriented) + " K=" + num(o.K)) + " overlap=" + num(o.overlap) +
          " sift_inside=" + num(o.sift_inside) + " with_affine=" + num(o.with_affine) + " side_streams=" + num(o.n_side);
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

// the upright order is the oriented one without its orientation kernel and turned pass, line for line
static void check_upright_inside(int n, const ScheduleOptions &o, const std::vector<Op> &oriented)
{
   ScheduleOptions up = o;
   up.oriented = false;
   const std::vector<Op> plain = full_trace(n, up);
   std::vector<Op> rest;
   bool turned = false;   // between the orientation kernel and the end of the unit's patch stage
   for (const Op &p : oriented) {
      turned = p.kind == Op::ORIENT || (turned && p.kind != Op::PATCH_DONE);
      if (!turned) rest.push_back(p);
   }
   CHECK(rest.size() == plain.size(), "%s: %zu operations outside the turned pass, %zu in the upright order", header(n, o).c_str(), rest.size(), plain.size());
   for (size_t i = 0; i < plain.size(); i++)
      CHECK(describe(rest[i]) == describe(plain[i]), "%s: '%s' where the upright order has '%s'", header(n, o).c_str(), describe(rest[i]).c_str(), describe(plain[i]).c_str());
   for (const Op &p : plain) CHECK(p.kind != Op::ORIENT && p.pass != PASS_TURNED, "%s: the upright order launches %s", header(n, up).c_str(), line(p).c_str());
}

// the properties for 0 .. max_n groups under all 24 option sets, for every orientation count K in [k_lo, k_hi]
static void check_properties(bool oriented, int k_lo, int k_hi, int max_n, int expect)
{
   int traces = 0;
   for (int n = 0; n <= max_n; n++)
      for (int K = k_lo; K <= k_hi; K++)
         for (int ov = 0; ov < 2; ov++)
            for (int in = 0; in < 2; in++)
               for (int wa = 0; wa < 2; wa++)
                  for (int side : kSides) {
                     const ScheduleOptions o = {ov == 1, in == 1, wa == 1, side, oriented, K};
                     const std::vector<Op> ops = full_trace(n, o);
                     const std::string why = check(ops, n, o);
                     CHECK(why.empty(), "%s: %s", header(n, o).c_str(), why.c_str());
                     // without overlap every logical stream is the main stream (the side streams are the caller's choice: the library forks none then)
                     for (const Op &p : ops)
                        CHECK(o.overlap || p.stream == S_MAIN || (p.stream >= S_BIN0 && p.stream < S_BIN0 + side), "%s: %s", header(n, o).c_str(), line(p).c_str());
                     if (oriented && K == 1) check_upright_inside(n, o, ops);
                     traces++;
                  }
   CHECK(traces == expect, "%d traces", traces);
}

// The checker bites: every wait and every record of the overlapped trace of n groups is needed, in both orders of submission, except
// the main stream's final waits for the chains that are not the last.  The descriptor chains stand on one stream, so the final wait for
// the last chain covers the HS_NSLOT - 1 before it: of 5 groups with one unit each, the waits for sift_done[0] of group 3 and for
// sift_done[2] of group 2.  (The schedule issues them all the same: the list is a finding, not a licence.)
static void check_sensitivity(int n, bool oriented, int K, int floor)
{
   for (int in = 0; in < 2; in++) {
      const ScheduleOptions o = {true, in == 1, true, HS_NSIDE, oriented, K};
      const std::vector<Op> ops = full_trace(n, o);
      const int units = n * K;
      CHECK(check(ops, n, o).empty(), "the complete trace");
      int deleted = 0, passed = 0;
      for (size_t i = 1; i < ops.size(); i++) {   // (ops[0] is the caller's record of detect-done)
         if (ops[i].kind != Op::WAIT && ops[i].kind != Op::RECORD) continue;
         std::vector<Op> cut = ops;
         cut.erase(cut.begin() + (long)i);
         deleted++;
         if (check(cut, n, o).empty()) {
            // the final waits come behind every slot's reuse: one that names a unit of the last HS_NSLOT is a final wait
            const Op &p = ops[i];
            bool final_wait = p.kind == Op::WAIT && p.stream == S_MAIN && p.ev.kind == Event::SIFT_DONE && p.ev.group != units - 1 && p.ev.group >= units - HS_NSLOT;
            for (size_t j = i + 1; j < ops.size() && final_wait; j++) final_wait = ops[j].kind == Op::WAIT || ops[j].kind == Op::END;
            CHECK(final_wait, "%s: no property fails without '%s'", header(n, o).c_str(), describe(p).c_str());
            passed++;
         }
      }
      CHECK(deleted > floor, "%d deletions", deleted);
      CHECK(passed == HS_NSLOT - 1, "%s: %d redundant waits", header(n, o).c_str(), passed);
   }
}

// A file of recorded sequences, one section per group count and option set: the traces equal them line for line.
struct Golden {
   std::map<std::string, std::string> sections;
   bool parent_format;
   size_t compared = 0;
   Golden(const std::string &path, bool parent_format_) : parent_format(parent_format_)
   {
      std::ifstream f(path);
      CHECK(f.good(), "cannot read %s", path.c_str());
      std::string l, cur;
      while (std::getline(f, l)) {
         if (!l.empty() && l[0] == '#') { cur = l; CHECK(sections.count(cur) == 0, "%s twice", cur.c_str()); sections[cur] = ""; }
         else { CHECK(!cur.empty(), "a line before the first section"); sections[cur] += l + "\n"; }
      }
   }
   void compare(int n, const ScheduleOptions &o)
   {
      const std::string h = header(n, o, parent_format);
      CHECK(sections.count(h) == 1, "no section '%s'", h.c_str());
      const std::vector<Op> ops = full_trace(n, o);
      std::string text;
      for (size_t i = 1; i + 1 < ops.size(); i++) text += line(ops[i], parent_format) + "\n";   // without the caller's two
      CHECK(text == sections[h], "%s differs from the recorded sequence:\n%s--- recorded:\n%s", h.c_str(), text.c_str(), sections[h].c_str());
      compared++;
   }
};

// group_schedule_parent.txt: what the code before this header issued
static void check_parent(const std::string &dir)
{
   Golden gold(dir + "/group_schedule_parent.txt", true);
   const int counts[5] = {0, 1, 2, 4, 5};
   for (int n : counts)
      for (int ov = 0; ov < 2; ov++)
         for (int in = 0; in < 2; in++)
            for (int wa = 0; wa < 2; wa++)
               for (int side : kSides)
                  // the parent chose the side streams by the overlap switch: none without overlap, 1 (fast mode 2) or HS_NSIDE with it
                  if ((side == 0) == (ov == 0)) gold.compare(n, ScheduleOptions{ov == 1, in == 1, wa == 1, side, false, 1});
   CHECK(gold.compared == 60 && gold.sections.size() == 60, "%zu sections compared of %zu", gold.compared, gold.sections.size());
}

// group_schedule_oriented_parent.txt: what the oriented form (K = 1) and the peaks form (K > 1) of the three-form header issued
static void check_oriented_parent(const std::string &dir, bool peaks)
{
   Golden gold(dir + "/group_schedule_oriented_parent.txt", false);
   static const int cases[5][2] = {{1, 1}, {2, 1}, {5, 1}, {4, 2}, {2, 4}};   // groups, K
   static const ScheduleOptions sets[4] = {{true, false, true, HS_NSIDE, true, 0}, {true, true, true, HS_NSIDE, true, 0}, {true, false, false, 1, true, 0},
                                           {false, false, true, 0, true, 0}};
   for (const int *cs : cases)
      for (ScheduleOptions o : sets) {
         o.K = cs[1];
         if ((o.K > 1) == peaks) gold.compare(cs[0], o);
      }
   CHECK(gold.compared == (peaks ? 8 : 12) && gold.sections.size() == 20, "%zu sections compared of %zu", gold.compared, gold.sections.size());
}

int main(int argc, char **argv)
{
   CHECK(argc == 2 || argc == 3, "usage: schedule_check tests/golden [upright | oriented | peaks]");
   const std::string dir = argv[1], part = argc == 3 ? argv[2] : "";
   CHECK(part.empty() || part == "upright" || part == "oriented" || part == "peaks", "no part '%s'", part.c_str());
   if (part.empty() || part == "upright") {
      check_properties(false, 1, 1, 10, 11 * 2 * 2 * 2 * 3);
      check_sensitivity(5, false, 1, 80);
      check_parent(dir);
   }
   if (part.empty() || part == "oriented") {
      check_properties(true, 1, 1, 10, 11 * 2 * 2 * 2 * 3);   // (and the upright order inside the oriented one at each point)
      check_sensitivity(5, true, 1, 160);
      check_oriented_parent(dir, false);
   }
   if (part.empty() || part == "peaks") {
      static_assert(HS_NSLOT + 2 <= 7, "the group counts reach HS_NSLOT + 2");
      check_properties(true, 2, 4, 7, 8 * 3 * 2 * 2 * 2 * 3);
      check_sensitivity(3, true, 2, 100);
      check_sensitivity(2, true, 4, 100);
      check_oriented_parent(dir, true);
   }
   printf("schedule_check ok\n");
   return 0;
}
