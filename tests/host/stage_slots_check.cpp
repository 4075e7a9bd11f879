// Host-side check of the in-order step pipeline's bookkeeping (csrc/stage_slots.h), compiled with g++ and run on the CPU by
// tests/test_host_index_algebra.py. Every stage is tagged with the number of the call it belongs to, and the CALLER's side of
// specscan.hip is played: run_batch puts call k's stages into the slots new_detect / new_plan / rows, marks what rides on each of the
// call's launches (riding), a launch takes the ready plan like launch_step does, the call ends with shift(); flush_stages drains.
//   * steady state: the launches of call k carry exactly the stages stage_slots.h promises for the schedule, at its lags;
//   * drain: from every state 0 ... 6 calls reach, the drain ends, runs every waiting stage exactly once, keeps every call's stages
//     in the order rows -> plan -> detect -> emit on strictly later launches each (so a plan shares a launch only with other calls'
//     stages) and leaves nothing waiting;
//   * mixed sessions: contexts of the merged form that take two-launch calls in between (they drain what waits for a row stage
//     first) and drains at random: thousands of calls, no stage lost, run twice or out of its call's order;
//   * a plan never waits without the detect stage it plans.
// A control run puts a merged call's detect stage into the slot of a two-launch call and must be caught.
// (Which of the two row-tile argument sets a merged launch uses — 256- or 1024-point rows — is a tag in the product's row record, set
// where run_batch fills it, and not the slots' business: the two merged schedules differ here in their tile count per frame only.)
#include <algorithm>
#include <array>
#include <cstdio>
#include <random>
#include <vector>

#include "../../rtl-sdr-scanner-cpp_amd/csrc/stage_slots.h"

namespace {

struct Emit { int call; };
struct Det { int call; Emit emit; };
struct Plan { int call; };
struct Rows { int call; int tiles; };
using W = ss::StageSlots<Det, Plan, Emit, Rows>;

enum Kind { ROWS = 0, PLAN = 1, DET = 2, EMIT = 3 };
enum Form { PLAIN = 0, PLAIN_EMIT_ON_COLS = 1, DET_LAG2 = 2, MERGED_256 = 3, MERGED_1024 = 4 };
inline bool merged(Form f) { return f == MERGED_256 || f == MERGED_1024; }
const char* const kFormName[] = {"plain", "plain, emit on the column launch", "det_lag2", "merged, 256-point rows", "merged, 1024-point rows"};

struct Carried {
  Kind kind;
  int call;
  bool operator<(const Carried& o) const { return kind != o.kind ? kind < o.kind : call < o.call; }
  bool operator==(const Carried& o) const { return kind == o.kind && call == o.call; }
};

struct Sim {
  W w;
  bool ctx_merge = false, ctx_lag2 = false, with_plan = true;
  bool wrong_slot = false;  // the control
  long launches = 0;
  int bad = 0;
  std::vector<std::array<long, 4>> ran;   // per call and kind: the launch that ran it (-1: not yet)
  std::vector<std::array<bool, 4>> owed;  // ... whether the call has such a stage at all
  std::vector<Carried> carried;           // what the launches since the last clear carried

  void note(Kind kind, int call) {
    if (ran[call][kind] >= 0 || !owed[call][kind]) ++bad;  // twice, or a stage nobody enqueued
    ran[call][kind] = launches;
    carried.push_back({kind, call});
  }
  // launch_step: det / emit / rows as marked, then the ready plan if the launch takes plans
  void launch(const W::Riders& r) {
    ++launches;
    if (r.det) note(DET, r.det->call);
    if (r.emit) note(EMIT, r.emit->call);
    if (r.rows) note(ROWS, r.rows->call);
    if (r.plan && w.plan_ready.have) {
      note(PLAN, w.plan_ready.v.call);
      w.plan_ready.have = false;
    }
  }
  void invariants() {
    const W::Riders none = w.riding(0);
    if (none.det || none.emit || none.rows || none.plan) ++bad;
    if (w.plan_wants_rows.have && !(w.det_wants_rows.have && w.det_wants_rows.v.call == w.plan_wants_rows.v.call && w.rows.have && w.rows.v.call == w.plan_wants_rows.v.call)) ++bad;
    const ss::StageSlot<Det>& planned_by_ready = ctx_lag2 ? w.det_wants_plan : w.det_planned;
    if (w.plan_ready.have && !(planned_by_ready.have && planned_by_ready.v.call == w.plan_ready.v.call)) ++bad;
    if (w.any_merged() && !w.any()) ++bad;
  }
  // flush_stages
  void flush() {
    const bool two_launch = !w.any_merged();
    if (two_launch && w.plan_ready.have) {  // the ready plan as a launch of its own
      ++launches;
      note(PLAN, w.plan_ready.v.call);
      w.plan_ready.have = false;
    }
    for (int guard = 0; w.any() && guard < 16; ++guard) {
      if (two_launch && (w.plan_ready.have || w.rows.have)) ++bad;  // (such a drain's launches carry a detect and an emit stage, nothing else)
      launch(w.riding(W::ALL));
      w.shift();
      invariants();
    }
    if (w.any()) ++bad;  // (did not end, or left something waiting)
  }
  // run_batch
  void call(Form f) {
    const int k = (int)ran.size();
    const bool m = merged(f);
    ran.push_back({-1, -1, -1, -1});
    owed.push_back({m, with_plan, true, true});
    if (ctx_merge && !m && w.any_merged()) flush();
    carried.clear();
    if (m) {
      launch(w.riding(W::ALL));
    } else if (f == DET_LAG2) {
      launch(w.riding(W::PLAN | W::DET | W::EMIT));  // column launch
      launch(w.riding(0));                           // row launch
    } else {
      launch(w.riding(W::PLAN | (f == PLAIN_EMIT_ON_COLS ? W::EMIT : 0)));
      launch(w.riding(W::DET | (f == PLAIN_EMIT_ON_COLS ? 0 : W::EMIT)));
    }
    w.shift();
    if (m) {
      w.rows.v = Rows{k, f == MERGED_1024 ? 32 : 8};
      w.rows.have = true;
    }
    ss::StageSlot<Det>& slot = wrong_slot ? w.new_detect(false, true) : w.new_detect(m, f == DET_LAG2);
    slot.v = Det{k, Emit{k}};
    slot.have = true;
    if (with_plan) {
      ss::StageSlot<Plan>& plan = w.new_plan(m);
      plan.v = Plan{k};
      plan.have = true;
    }
    invariants();
  }
  // every stage of every call: once, in its call's order, each on a later launch than the one before
  void settle() {
    if (w.any()) ++bad;
    for (size_t k = 0; k < ran.size(); ++k) {
      long last = -1;
      for (int kind = ROWS; kind <= EMIT; ++kind) {
        if (!owed[k][kind]) continue;
        if (ran[k][kind] < 0 || ran[k][kind] <= last) ++bad;  // lost, or not strictly behind the stage before it
        last = ran[k][kind];
      }
    }
  }
};

// what the launches of call k carry in steady state (stage_slots.h)
std::vector<Carried> promised(Form f, int k, bool with_plan) {
  const int lag_rows = 1, lag_plan = merged(f) ? 2 : 1, lag_det = merged(f) ? 3 : f == DET_LAG2 ? 2 : 1, lag_emit = lag_det + 1;
  std::vector<Carried> e;
  if (merged(f) && k >= lag_rows) e.push_back({ROWS, k - lag_rows});
  if (with_plan && k >= lag_plan) e.push_back({PLAN, k - lag_plan});
  if (k >= lag_det) e.push_back({DET, k - lag_det});
  if (k >= lag_emit) e.push_back({EMIT, k - lag_emit});
  return e;
}

Sim context_for(Form f, bool with_plan) {
  Sim s;
  s.ctx_merge = merged(f);
  s.ctx_lag2 = merged(f) || f == DET_LAG2;
  s.with_plan = with_plan;
  return s;
}

}  // namespace

int main() {
  int bad = 0;
  long long calls = 0;
  const Form forms[] = {PLAIN, PLAIN_EMIT_ON_COLS, DET_LAG2, MERGED_256, MERGED_1024};
  for (Form f : forms)
    for (int with_plan = 1; with_plan >= (f == PLAIN ? 0 : 1); --with_plan) {  // (8192 points: the plain schedule without a plan stage)
      // steady state
      Sim s = context_for(f, with_plan);
      int form_bad = 0;
      for (int k = 0; k < 40; ++k, ++calls) {
        s.call(f);
        std::vector<Carried> got = s.carried, want = promised(f, k, with_plan);
        std::sort(got.begin(), got.end());
        std::sort(want.begin(), want.end());
        if (!(got == want)) ++form_bad;
        if (merged(f) && s.w.rows.v.tiles != (f == MERGED_1024 ? 32 : 8)) ++form_bad;
      }
      s.flush();
      s.settle();
      form_bad += s.bad;
      // drain from every state 0 ... 6 calls reach
      for (int n = 0; n <= 6; ++n) {
        Sim d = context_for(f, with_plan);
        for (int k = 0; k < n; ++k, ++calls) d.call(f);
        const long before = d.launches;
        d.flush();
        d.settle();
        if (n == 0 && d.launches != before) ++d.bad;  // (nothing waits: nothing is launched)
        form_bad += d.bad;
      }
      printf("%-34s%s bad %d\n", kFormName[f], with_plan ? "" : " (no plan stage)", form_bad);
      bad += form_bad;
    }
  // mixed sessions
  std::mt19937 rng(20240607);
  int mixed_bad = 0;
  for (int trial = 0; trial < 24; ++trial) {
    Sim s;
    s.ctx_merge = trial % 3 != 0;          // two in three: a context of the merged form ...
    s.ctx_lag2 = s.ctx_merge || trial % 2;  // ... (which is a det_lag2 context too)
    const Form two_launch = s.ctx_lag2 ? DET_LAG2 : (trial & 4) ? PLAIN_EMIT_ON_COLS : PLAIN;
    const Form one_launch = (trial & 8) ? MERGED_1024 : MERGED_256;
    for (int k = 0; k < 4000; ++k, ++calls) {
      const unsigned r = rng();
      s.call(s.ctx_merge && (r & 3) != 0 ? one_launch : two_launch);  // runs of merged calls, a two-launch call now and then
      if ((r >> 8) % 11 == 0) s.flush();                              // (ss_sync, a call that may not overlap, a moved ring window)
    }
    s.flush();
    s.settle();
    mixed_bad += s.bad;
  }
  printf("mixed sessions bad %d\n", mixed_bad);
  bad += mixed_bad;
  // the control: the check must see a detect stage in the wrong slot
  {
    Sim s = context_for(MERGED_256, true);
    s.wrong_slot = true;
    for (int k = 0; k < 8; ++k) s.call(MERGED_256);
    s.flush();
    s.settle();
    printf("control (wrong slot) caught %d\n", s.bad);
    if (s.bad == 0) ++bad;
  }
  printf("calls %lld, bad %d\n", calls, bad);
  return bad ? 1 : 0;
}
