// stage_slots.h — the stages of earlier calls that wait on the host until a later launch carries them: the bookkeeping of specscan.hip's
// in-order step pipeline as fixed slots named for what each stage waits for (no HIP in here, payloads are template parameters:
// tests/host/stage_slots_check.cpp runs it on the CPU against the schedules below). The slots of the pipelined feed are another
// matter: feed_ring.h, under host_feed.h.
//
// A call's stages run in the order rows -> plan -> detect -> emit, each on a later launch than the one before; the launches of the
// calls that follow carry them (scan_step.h), or flush_stages drains them. Buffers a waiting stage reads while a later call already
// writes its own are doubled (mask bits, sparse avg plane, internal PSD plane). A new call's stages enter at new_detect / new_plan /
// rows, every call ends with shift(), and what the launches of call k carry follows from where they entered:
//   PLAIN     8192 points without the deep path; 2^20 points; 65536 points with SS_DET_LAG2=0. The detect stage enters planned; its plan,
//             where the size has one (k_plan_long: which tiles the stage must evaluate), enters ready and runs ahead of it, at the front
//             of the next call's column launch (k_fft_cols1024_plan) or as a role of it: plan(k - 1), detect(k - 1), emit(k - 2).
//   DET_LAG2  65536 points with tile culling, 262144 points: the planned detect stage rides on the COLUMN launch, the longer of a call's
//             two, where the workgroups that evaluate listed tiles (20 us apiece under the launch's streaming loads) end with the column
//             tiles instead of being the row launch's tail. The plan it needs rides on the column launch before, so the stage enters
//             waiting for its plan: plan(k - 1), detect(k - 2), emit(k - 3). (The fold's one launch per call carries the same.)
//   MERGED    65536 points (scan_step.h KIND 7) and 262144 points (KIND 12), one launch per call for calls that keep no dB plane, up to
//             merge_max frames: it carries the column half of call k and the ROW half of call k - 1 (256- or 1024-point row tiles, two
//             work buffers). Plan and detect stage enter waiting for that row stage: rows(k - 1), plan(k - 2), detect(k - 3), emit(k - 4).
// A context of the merged form takes calls of the other forms too (learning frames, planes handed out): such a call drains what waits
// for a row stage first and then follows the two-launch schedule.
#pragma once

namespace ss {

template <class T>
struct StageSlot {
  bool have = false;
  T v{};
  void take(StageSlot& from) {  // the stage that waited in `from`, if there is one, waits here now
    if (from.have) *this = from;
    from.have = false;
  }
};

// Det carries its own emit stage as a member `emit` (ss_ctx::PendDet).
template <class Det, class Plan, class Emit, class Rows>
struct StageSlots {
  StageSlot<Det> det_planned;      // its plan has run (or it needs none): rides on the next launch that takes a detect stage
  StageSlot<Det> det_wants_plan;   // its plan is plan_ready
  StageSlot<Det> det_wants_rows;   // its call's row stage is `rows`
  StageSlot<Plan> plan_ready;      // the launch that carries it takes it (launch_step, launch_cols1024, flush_stages)
  StageSlot<Plan> plan_wants_rows;
  StageSlot<Emit> emit;            // of the detect stage the last launch carried
  StageSlot<Rows> rows;            // the row half of the last call

  bool any() const { return det_planned.have || det_wants_plan.have || plan_ready.have || emit.have || any_merged(); }
  bool any_merged() const { return rows.have || plan_wants_rows.have || det_wants_rows.have; }

  // where a new call's detect stage and its plan enter
  StageSlot<Det>& new_detect(bool merged_call, bool det_lag2) { return merged_call ? det_wants_rows : det_lag2 ? det_wants_plan : det_planned; }
  StageSlot<Plan>& new_plan(bool merged_call) { return merged_call ? plan_wants_rows : plan_ready; }

  // What rides on a launch: the caller names the kinds, present stages of those kinds go. (The deep path fills one from its own queues.)
  static constexpr unsigned DET = 1, EMIT = 2, PLAN = 4, ROWS = 8, ALL = 15;
  struct Riders {
    const Det* det = nullptr;
    const Emit* emit = nullptr;
    const Rows* rows = nullptr;
    bool plan = false;  // plan_ready, if there is one
  };
  Riders riding(unsigned kinds) const {
    return {(kinds & DET) && det_planned.have ? &det_planned.v : nullptr, (kinds & EMIT) && emit.have ? &emit.v : nullptr,
            (kinds & ROWS) && rows.have ? &rows.v : nullptr, (kinds & PLAN) != 0};
  }

  // A call's launches have carried the planned detect stage, the emit stage and the row stage that waited: every stage moves up one
  // slot. (The ready plan is not shift's to move: the launch that carried it took it.)
  void shift() {
    emit.have = det_planned.have;
    emit.v = det_planned.v.emit;
    det_planned.have = false;
    det_planned.take(det_wants_plan);
    det_wants_plan.take(det_wants_rows);  // (the row stage has run: its plan is ready now)
    plan_ready.take(plan_wants_rows);
    rows.have = false;
  }
};

}  // namespace ss
