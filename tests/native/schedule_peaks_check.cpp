// CPU check of the group pipeline's PEAKS stream / event order (hesaff_amd/csrc/group_schedule.h: run_group_schedule_peaks, the order
// hesaff_set_orientation_count(K > 1) runs in HESAFF_ORI_DOMINANT; built and run by tests/test_orientation_count_host.py with
// g++ -fsanitize=address,undefined).  A recording device of its own turns a run of the template into a trace; the happens-before
// relation is built from the trace as tests/native/schedule_oriented_check.cpp builds it - operations of one stream are ordered, a wait
// is ordered behind the record of its event issued last before it, which must be the record the wait names - and the conditions the
// order exists for are asserted of it.  The unit is the (group, rank) pair, v = g * K + r, in slot v % HS_NSLOT:
//   - rank 0 of a group is the oriented order's patch stage, with the oriented order's conditions;
//   - rank_prepare(g, r) behind orientation(g), whose frames and flags it reads, and behind every patch kernel of the unit before on
//     every stream, whose counters it clears; the patch kernels of (g, r) behind rank_prepare(g, r);
//   - whatever writes a slot, the bins or a rank's flags stands behind the descriptors of every earlier unit of that slot, and in front
//     of the unit's own descriptors, of the next unit's prepare and of the end;
//   - one descriptor chain at a time, in ascending v.
// Three parts: the properties at 0, 1, 2, HS_NSLOT and HS_NSLOT + 2 groups (and every count up to 7) for K = 2, 3, 4 under every option;
// K = 1 is the oriented order line for line; sensitivity (each single wait or record deleted from overlapped traces breaks a property,
// but for a short list).  Prints "schedule_peaks_check ok"; a failed check prints a message and ends the program with exit code 1.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>
#include "../../hesaff_amd/csrc/group_schedule.h"

using namespace hesaff_sched;

struct Op {
   enum Kind { WAIT, RECORD, AFFINE, PREPARE, PATCH, ORIENT, REBIN, RANK_PREPARE, RANK_PATCH, PATCH_DONE, DESCRIPTORS, END } kind;
   Stream stream;
   Event ev;                // WAIT, RECORD
   int group, rank, slot;   // the launches; -1: none
   int phase;               // counts the patch passes: a fork or join wait must see the record of its own pass
};

static std::string num(int v) { return v < 0 ? "-" : std::to_string(v); }
static std::string line(const Op &o)
{
   static const char *kinds[] = {"wait", "record", "affine", "prepare", "patch", "orient", "rebin", "rank_prepare", "rank_patch", "patch_done", "descriptors", "end"};
   static const char *streams[S_COUNT] = {"main", "bin0", "bin1", "bin2", "bin3", "desc", "affine"};
   static const char *events[] = {"detect_done", "affine_done", "extract_done", "sift_done", "fork", "join"};
   static_assert(HS_NSIDE == 4, "one name per side stream");
   const bool ev = o.kind == Op::WAIT || o.kind == Op::RECORD;
   return std::string(kinds[o.kind]) + " " + streams[o.stream] + " " + (ev ? std::string(events[o.ev.kind]) + "[" + std::to_string(o.ev.index) + "]" : "-") + " " +
          num(o.group) + " " + num(o.rank) + " " + num(o.slot);
}
static std::string describe(const Op &o) { return line(o) + " names " + num(o.ev.group); }

struct OrientedRecorder {
   std::vector<Op> ops;
   int phase = 0;
   void add(Op::Kind k, Stream s, int g, int r, int slot) { ops.push_back(Op{k, s, Event{Event::DETECT_DONE, 0, -1}, g, r, slot, phase}); }
   void wait(Stream s, const Event &e) { ops.push_back(Op{Op::WAIT, s, e, -1, -1, -1, phase}); }
   void record(const Event &e, Stream s) { ops.push_back(Op{Op::RECORD, s, e, -1, -1, -1, phase}); }
   void affine(int g, Stream s) { add(Op::AFFINE, s, g, -1, -1); }
   void patch_prepare(int g) { phase++; add(Op::PREPARE, S_MAIN, g, 0, -1); }
   void kernels(Op::Kind k, int g, int r, int slot, int n_side)
   {
      for (int i = 0; i < HS_NSIDE; i++)
         if (patch_stream(i, n_side) != S_MAIN) add(k, patch_stream(i, n_side), g, r, slot);
      add(k, S_MAIN, g, r, slot);
   }
   void patch_kernels(int g, int slot, int n_side) { kernels(Op::PATCH, g, 0, slot, n_side); }
   void orientation(int g, int slot) { phase++; add(Op::ORIENT, S_MAIN, g, 0, slot); }
   void patch_rebin(int g) { add(Op::REBIN, S_MAIN, g, 0, -1); }
   void patch_done(int g) { add(Op::PATCH_DONE, S_MAIN, g, -1, -1); }
   void descriptors(int g, int slot, Stream s) { add(Op::DESCRIPTORS, s, g, 0, slot); }
};
struct PeaksRecorder : OrientedRecorder {
   void rank_prepare(int g, int r) { phase++; add(Op::RANK_PREPARE, S_MAIN, g, r, -1); }
   void rank_patch_kernels(int g, int r, int slot, int n_side) { kernels(Op::RANK_PATCH, g, r, slot, n_side); }
   void rank_descriptors(int g, int r, int slot, Stream s) { add(Op::DESCRIPTORS, s, g, r, slot); }
};

template <class R, class RUN> static std::vector<Op> full_trace(RUN run)
{
   R r;
   r.record(ev_detect_done(), S_MAIN);
   run(r);
   r.add(Op::END, S_MAIN, -1, -1, -1);
   return r.ops;
}
static std::vector<Op> peaks_trace(int n, int K, const ScheduleOptions &o)
{
   return full_trace<PeaksRecorder>([&](PeaksRecorder &r) { run_group_schedule_peaks(r, n, K, o); });
}
static std::vector<Op> oriented_trace(int n, const ScheduleOptions &o)
{
   return full_trace<OrientedRecorder>([&](OrientedRecorder &r) { run_group_schedule_oriented(r, n, o); });   // (a device WITHOUT the rank members)
}

// "" when every property holds of the trace, else the first that does not
static std::string check(const std::vector<Op> &ops, int n, int K, const ScheduleOptions &o)
{
   const size_t N = ops.size();
   const int units = n * K;
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
      if ((ops[i].ev.kind == Event::FORK || ops[i].ev.kind == Event::JOIN) && ops[rec].phase != ops[i].phase)
         return describe(ops[i]) + ": captured another pass's " + describe(ops[rec]);
      order(i, rec);
   }
   std::vector<int> A(n, -1), PP(n, -1), OR(n, -1), RB(n, -1), RP(units, -1), D(units, -1);
   std::vector<std::vector<int>> PK1(n), LAST(units);   // pass one's kernels of a group; the kernels that write the patches a unit's descriptors read
   int detect = -1, end = -1;
   for (size_t i = 0; i < N; i++) {
      const Op &p = ops[i];
      if (p.kind == Op::RECORD && p.ev.kind == Event::DETECT_DONE) detect = (int)i;
      if (p.kind == Op::END) end = (int)i;
      if (p.kind == Op::WAIT || p.kind == Op::RECORD || p.kind == Op::END || p.kind == Op::PATCH_DONE) continue;
      if (p.group < 0 || p.group >= n) return line(p) + ": no such group";
      if (p.kind == Op::AFFINE) {
         if (A[p.group] >= 0) return line(p) + ": issued twice";
         A[p.group] = (int)i;
         continue;
      }
      if (p.rank < 0 || p.rank >= K) return line(p) + ": no such rank";
      const int v = p.group * K + p.rank;
      if ((p.kind == Op::RANK_PREPARE || p.kind == Op::RANK_PATCH) && p.rank == 0) return line(p) + ": rank 0 has the oriented order's stage";
      if (p.kind == Op::PATCH) { (OR[p.group] < 0 ? PK1[p.group] : LAST[v]).push_back((int)i); continue; }
      if (p.kind == Op::RANK_PATCH) { LAST[v].push_back((int)i); continue; }
      int &one = p.kind == Op::PREPARE ? PP[p.group] : p.kind == Op::ORIENT ? OR[p.group] : p.kind == Op::REBIN ? RB[p.group] : p.kind == Op::RANK_PREPARE ? RP[v] : D[v];
      if (one >= 0) return line(p) + ": issued twice";
      one = (int)i;
   }
   if (detect < 0 || end < 0) return "the trace lacks the caller's detect-done or its end";
   auto hb = [&](int a, int b) { return before[b][a]; };   // a happens before b
   auto fail = [&](const char *what, int a, int b) { return std::string(what) + ": " + describe(ops[a]) + " is not ordered before " + describe(ops[b]); };
   const size_t per_pass = (size_t)o.n_side + 1;   // one operation per stream that runs a patch kernel
   for (int v = 0; v < units; v++) {
      const int g = v / K, r = v % K;
      const std::string name = "group " + std::to_string(g) + " rank " + std::to_string(r);
      if (D[v] < 0 || LAST[v].size() != per_pass) return name + ": a stage is missing, or not one patch operation per stream";
      std::vector<int> stage = LAST[v];   // everything of the unit that writes the slot, the bins, their counters or flags
      if (r == 0) {
         if (PP[g] < 0 || OR[g] < 0 || RB[g] < 0 || (A[g] >= 0) != o.with_affine || PK1[g].size() != per_pass) return name + ": a stage is missing";
         stage.insert(stage.end(), PK1[g].begin(), PK1[g].end());
         stage.push_back(PP[g]); stage.push_back(OR[g]); stage.push_back(RB[g]);
      } else {
         if (RP[v] < 0) return name + ": no rank_prepare";
         stage.push_back(RP[v]);
      }
      const int slot = v % HS_NSLOT;
      if (ops[D[v]].slot != slot) return name + ": descriptors not from slot v % HS_NSLOT";
      for (int k : stage)
         if (ops[k].slot >= 0 && ops[k].slot != slot) return name + ": " + line(ops[k]) + " not in slot v % HS_NSLOT";
      const int next_prepare = v + 1 >= units ? -1 : (v + 1) % K == 0 ? PP[(v + 1) / K] : RP[v + 1];
      for (int k : stage) {
         if (o.with_affine && !hb(A[g], k)) return fail("affine before the patch stage", A[g], k);
         for (int e = 0; e < v; e++)
            if (e % HS_NSLOT == slot && !hb(D[e], k)) return fail("a slot rewritten before its descriptors are done", D[e], k);
         if (!hb(k, D[v])) return fail("the patch stage before its descriptors", k, D[v]);
         if (!hb(k, end)) return fail("the end behind the patch stage", k, end);
         if (next_prepare >= 0 && !hb(k, next_prepare)) return fail("the next unit's prepare under this patch stage", k, next_prepare);
      }
      if (r == 0) {
         for (int k : PK1[g]) {
            if (!hb(PP[g], k)) return fail("k_prepare_patch before the first pass's bins", PP[g], k);
            if (!hb(k, OR[g])) return fail("first-pass patches before the orientation kernel", k, OR[g]);
            if (!hb(k, RB[g])) return fail("the bin counters cleared under a first-pass patch kernel", k, RB[g]);
         }
         if (!hb(PP[g], OR[g])) return fail("k_prepare_patch before the orientation kernel", PP[g], OR[g]);
         if (!hb(OR[g], RB[g])) return fail("the orientation kernel before the re-bin", OR[g], RB[g]);
         for (int k : LAST[v]) {
            if (!hb(OR[g], k)) return fail("the orientation kernel before rank 0's pass", OR[g], k);
            if (!hb(RB[g], k)) return fail("the re-bin before rank 0's bins", RB[g], k);
            for (int k1 : PK1[g])
               if (!hb(k1, k)) return fail("the first pass before rank 0's", k1, k);
         }
      } else {
         if (!hb(OR[g], RP[v])) return fail("the orientation kernel before a rank's prepare", OR[g], RP[v]);
         for (int k : LAST[v - 1])   // they read the counters rank_prepare clears, and the row-streamed bins' per-block slots
            if (!hb(k, RP[v])) return fail("the rank before under this rank's prepare", k, RP[v]);
         for (int k : LAST[v]) {
            if (!hb(RP[v], k)) return fail("rank_prepare before the rank's bins", RP[v], k);
            for (int k1 : LAST[v - 1])
               if (!hb(k1, k)) return fail("the rank before under this rank's patch kernels", k1, k);
         }
      }
      if (v > 0 && !hb(D[v - 1], D[v])) return fail("one descriptor chain at a time, in ascending rank", D[v - 1], D[v]);
      if (!hb(D[v], end)) return fail("the end behind every descriptor chain", D[v], end);
      if (o.with_affine && !hb(A[g], end)) return fail("the end behind every affine", A[g], end);
   }
   if (o.with_affine && n > 0 && !hb(detect, A[0])) return fail("affine behind detect-done", detect, A[0]);
   return "";
}

static std::string header(int n, int K, const ScheduleOptions &o)
{
   return "# groups=" + std::to_string(n) + " K=" + std::to_string(K) + " overlap=" + num(o.overlap) + " sift_inside=" + num(o.sift_inside) + " with_affine=" +
          num(o.with_affine) + " side_streams=" + num(o.n_side);
}

#define CHECK(cond, ...)                                                                        \
   do {                                                                                         \
      if (!(cond)) {                                                                            \
         fprintf(stderr, "schedule_peaks_check: %s:%d: %s failed: ", __FILE__, __LINE__, #cond); \
         fprintf(stderr, __VA_ARGS__);                                                          \
         fprintf(stderr, "\n");                                                                 \
         exit(1);                                                                               \
      }                                                                                         \
   } while (0)

static const int kSides[3] = {0, 1, HS_NSIDE};

static void check_properties()
{
   static_assert(HS_NSLOT + 2 <= 7, "the group counts below reach HS_NSLOT + 2");
   int traces = 0;
   for (int n = 0; n <= 7; n++)
      for (int K = 2; K <= 4; K++)
         for (int ov = 0; ov < 2; ov++)
            for (int in = 0; in < 2; in++)
               for (int wa = 0; wa < 2; wa++)
                  for (int side : kSides) {
                     const ScheduleOptions o = {ov == 1, in == 1, wa == 1, side};
                     const std::vector<Op> ops = peaks_trace(n, K, o);
                     const std::string why = check(ops, n, K, o);
                     CHECK(why.empty(), "%s: %s", header(n, K, o).c_str(), why.c_str());
                     for (const Op &p : ops)
                        CHECK(o.overlap || p.stream == S_MAIN || (p.stream >= S_BIN0 && p.stream < S_BIN0 + side), "%s: %s", header(n, K, o).c_str(), line(p).c_str());
                     traces++;
                  }
   CHECK(traces == 8 * 3 * 2 * 2 * 2 * 3, "%d traces", traces);
}

// an orientation count of 1 given to the peaks form is the oriented order, line for line
static void check_count_one()
{
   for (int n = 0; n <= HS_NSLOT + 2; n++)
      for (int ov = 0; ov < 2; ov++)
         for (int in = 0; in < 2; in++)
            for (int wa = 0; wa < 2; wa++)
               for (int side : kSides) {
                  const ScheduleOptions o = {ov == 1, in == 1, wa == 1, side};
                  const std::vector<Op> a = peaks_trace(n, 1, o), b = oriented_trace(n, o);
                  CHECK(a.size() == b.size(), "%s: %zu operations, the oriented order has %zu", header(n, 1, o).c_str(), a.size(), b.size());
                  for (size_t i = 0; i < a.size(); i++)
                     CHECK(describe(a[i]) == describe(b[i]), "%s: '%s' where the oriented order has '%s'", header(n, 1, o).c_str(), describe(a[i]).c_str(), describe(b[i]).c_str());
               }
}

// Every wait and every record of the overlapped traces of 3 groups with K = 2 and of 2 groups with K = 4 is needed, in both orders of
// submission, except the main stream's final waits for chains that are not the last one: the chains stand on one stream, so the wait for
// the last chain covers those before it.
static bool redundant(const Op &p, int units)
{
   return p.kind == Op::WAIT && p.stream == S_MAIN && p.ev.kind == Event::SIFT_DONE && p.ev.group != units - 1 && p.ev.group >= units - HS_NSLOT;
}

static void check_sensitivity()
{
   static const int cases[2][2] = {{3, 2}, {2, 4}};
   for (const int *cs : cases)
      for (int in = 0; in < 2; in++) {
         const int n = cs[0], K = cs[1];
         const ScheduleOptions o = {true, in == 1, true, HS_NSIDE};
         const std::vector<Op> ops = peaks_trace(n, K, o);
         CHECK(check(ops, n, K, o).empty(), "the complete trace");
         int deleted = 0, passed = 0;
         for (size_t i = 1; i < ops.size(); i++) {   // (ops[0] is the caller's record of detect-done)
            if (ops[i].kind != Op::WAIT && ops[i].kind != Op::RECORD) continue;
            std::vector<Op> cut = ops;
            cut.erase(cut.begin() + (long)i);
            deleted++;
            if (!check(cut, n, K, o).empty()) continue;
            // the final waits come behind every slot's reuse: one that names a unit of the last HS_NSLOT is a final wait
            bool final_wait = redundant(ops[i], n * K);
            for (size_t j = i + 1; j < ops.size() && final_wait; j++) final_wait = ops[j].kind == Op::WAIT || ops[j].kind == Op::END;
            CHECK(final_wait, "%s: no property fails without '%s'", header(n, K, o).c_str(), describe(ops[i]).c_str());
            passed++;
         }
         CHECK(deleted > 100, "%d deletions", deleted);
         CHECK(passed == HS_NSLOT - 1, "%s: %d redundant waits", header(n, K, o).c_str(), passed);
      }
}

int main()
{
   check_properties();
   check_count_one();
   check_sensitivity();
   printf("schedule_peaks_check ok\n");
   return 0;
}
