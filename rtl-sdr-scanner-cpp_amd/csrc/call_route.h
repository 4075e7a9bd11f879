// call_route.h — what one call decides, as plain C++ (no HIP include: the stand-alone check tests/host/call_route_check.cpp compiles it
// with g++). CallAsk: what a call brings. CallRoute: what specscan.hip's run_batch then does — the launch shape, the predicates its
// state-dependent steps read (settle_ring_db, set_ring_form, place_ring, the clash test, any_merged), the chunking of a long call and what
// rides on the first chunk's launches. decide_call: the decision, from the form (scan_form.h), the choices, the flags and the ask alone.
//
//   shape          launches of one chunk                                       chunk (frames)          riders, first chunk: 1st | 2nd launch
//   DEEP           run_call_deep's one launch (its own queues and riders)      the call                - | -
//   FRAMES_8192    8192-point frames as the step's FFT role                    the call                DET EMIT | -
//   COLS_ROWS      columns as the FFT role, launch_fft_rows                    the call                DET EMIT | -
//   FOLD           the radix-8 / radix-16 fold as the FFT role                 the call                DET EMIT PLAN | -
//   MERGED         columns as the FFT role beside the rows of the call before  the call                DET EMIT PLAN ROWS | -
//   ROWS256_STEP   columns, then 256-point rows, both as FFT roles             Diag::chunk_65536       PLAN (DET) EMIT | (DET)   (DET: first with det_lag2)
//   ROWS1024X256   columns as the FFT role, launch_rows1024x256                64                      DET EMIT PLAN | -
//   TWO_PASS       launch_cols1024, then 1024-point rows as the FFT role       Diag::chunk_long        PLAN | DET EMIT   (the column launch takes the ready plan itself)
//   NON_STEP       launch_fft and the back end at once                         the call                - | -
// Later chunks carry nothing.
#pragma once
#include "ring_place.h"
#include "scan_form.h"

namespace {

struct CallAsk {
  int nframes = 0;
  int n_learn = 0;      // leading frames that belong to the noise-learning phase
  bool device = false;  // ss_process_device: the caller's buffers stay untouched until ss_sync, stages may wait (host calls and the feed drain)
  bool psd = false, rel = false, avg = false;  // planes handed out
  bool spec = false;    // a spectrogram container is attached
};

enum CallShape { CALL_DEEP = 0, CALL_FRAMES_8192, CALL_COLS_ROWS, CALL_FOLD, CALL_MERGED, CALL_ROWS256_STEP, CALL_ROWS1024X256, CALL_TWO_PASS, CALL_NON_STEP, kCallShapes };
inline const char* call_shape_name(CallShape s) {
  static const char* const names[kCallShapes] = {"deep", "frames_8192", "cols_rows", "fold", "merged", "rows256_step", "rows1024x256", "two_pass", "non_step"};
  return names[s];
}

// rider kinds, as StageSlots::riding takes them (stage_slots.h; specscan.hip asserts that the two agree)
constexpr unsigned kRideDet = 1, kRideEmit = 2, kRidePlan = 4, kRideRows = 8;

struct CallRoute {
  CallShape shape = CALL_NON_STEP;
  // (one predicate for the three decisions below — fold, dB rows in the ring, no dB plane at all: a device call without learning frames
  // that hands out no plane and keeps none; and the room for a whole batch's rows in the ring's buffer is ring_place.h's `whole` branch,
  // a function of the sizes alone — every culling context has it for every call it accepts, tests/host/call_route_check.cpp — so a fold
  // call knows before the window is rewritten that its rows have a place)
  bool keeps_no_plane = false;
  // 65536 points, int8 IQ: a call that keeps no plane goes through the radix-8 fold (KIND 8) — decided before the ring is placed,
  // because a change of form rewrites the window
  bool dif_call = false;
  // ... and the rows the FFT stage of a detect-mode call leaves in the ring are dB values (ring_db_rows): a call of any other kind, and
  // a call under another ceiling, has them turned into noise-relative rows first
  bool db_call = false;
  // Tile culling for long transforms: the rows kernel leaves the run maxima of every frame and, in a call without learning
  // frames, writes the ring rows of the batch itself (ring_by_rows)
  bool cull_call = false;  // (131072 points: only the fold's calls leave run maxima and write the ring themselves)
  bool ring_by_rows = false;
  // no dB plane at all: a device call that hands out no plane, whose rows the new rows kernel writes — behind the window being read when
  // it is shorter than the ring, as a region place_ring reserves otherwise (ring_place_at's `whole` branch gives one wherever the window
  // starts: a function of the sizes, and with the room above the same thing as db_call)
  bool ring_only = false;
  // (SS_FLAG_STREAM_ORDERED / SS_FLAG_REFERENCE_NAN: every stage of the call before the call returns, in order on the public stream)
  // (CALL_DEEP: what the call allows; run_call_deep adds what the context's state says — deep_eager, deep_iq_recycled)
  bool overlap = false;
  // one launch per call (SS_MERGE_65536): calls that keep no dB plane, in one piece, with stages allowed to overlap; any other call
  // drains what waits in that form and goes the two-launch way
  // (up to 128 frames: two 64 MiB work buffers in flight are what the Infinity Cache holds beside the rest — 256-frame calls lose a tenth
  // this way and have two rounds of workgroups per launch anyway, profiles/r04/s34_summary.txt)
  bool merged_call = false;
  // (the plan of call k rides at the front of call k + 1's column launch: four plan blocks share a column tile's LDS)
  bool plan_fused = false;
  bool det_lag2 = false;  // with merged_call: where the call's detect stage and plan enter (StageSlots::new_detect, new_plan)
  // A call of many frames goes through in chunks, the deferred stages riding on the first chunk's launches:
  //   65536 points, chunks of 256 (a chunk's work buffer: 128 MiB, still in the Infinity Cache when its row half reads it: the row half
  //   of a 512-frame call took 0.206 us per frame against 0.132, profiles/r04/s28_summary.txt);
  //   262144 points, chunks of 64 (a chunk's work buffer: 128 MiB);
  //   2^20 points, chunks of 16: the work buffer of a chunk (128 MiB) is still in the 256 MiB Infinity Cache when the chunk's row half
  //   reads it — 2.8 us per frame for the row half against 4.1-4.3 when a 32- or 64-frame call's work buffer has to come back from HBM
  //   (profiles/r04/s26_summary.txt).
  int chunk = 0;
  // 65536 points with tile culling: what ships (det_lag2, stage_slots.h): plan, planned detect stage and emit stage on the column
  // launch, nothing on the row launch. SS_DET_LAG2=0: plan and emit stage on the column launch, the detect stage on the row launch
  // (29.5 us for a launch that takes 17 alone: profiles/r04/s17_summary.txt). SS_EMIT_ON_ROWS=1 (SS_DIAG): the emit stage on the row launch.
  // 2^20 points: the deferred stages ride on the first chunk's row launch, the plan of the call before on its column launch.
  unsigned ride_first = 0, ride_second = 0;
};

// the chunk a context of this form cuts long calls into (0: none)
inline int call_chunk_limit(const ScanForm& f, const Diag& d) {
  if (f.deep || !f.step_path || f.use_fft8192) return 0;
  return f.rows256_step ? std::max(d.chunk_65536, 0) : f.rows1024x256 ? 64 : f.two_pass ? std::max(d.chunk_long, 0) : 0;
}

inline CallRoute decide_call(const ScanForm& f, const Diag& d, uint32_t flags, const CallAsk& a) {
  CallRoute r{};
  r.chunk = a.nframes;
  if (f.deep) {
    r.shape = CALL_DEEP;
    r.overlap = a.device && d.pipeline && a.n_learn == 0 && a.nframes >= kHistRows;
    return r;
  }
  if (!f.step_path) return r;
  const bool in_order = (flags & (SS_FLAG_STREAM_ORDERED | SS_FLAG_REFERENCE_NAN)) != 0;
  r.keeps_no_plane = a.device && a.n_learn == 0 && !a.psd && !a.rel && !a.avg && !a.spec && !f.ref_nan && !(flags & SS_FLAG_KEEP_PLANES) && d.ring_only;
  r.dif_call = f.dif8 && f.cull_long && d.pipeline && r.keeps_no_plane && !in_order;
  r.cull_call = f.cull_long && (!f.cull_fold_only || r.dif_call);
  r.db_call = r.cull_call && r.keeps_no_plane;
  r.ring_by_rows = r.cull_call && a.n_learn == 0;
  r.ring_only = r.ring_by_rows && r.keeps_no_plane;
  r.overlap = d.pipeline && a.n_learn == 0 && !in_order;
  r.merged_call = f.merge && (f.rows256_step || f.rows1024x256) && r.overlap && r.ring_only && !a.spec && a.nframes <= f.merge_max;
  r.det_lag2 = f.det_lag2;
  const bool rows_by_step = f.two_pass || f.rows256_step || f.rows1024x256;
  r.plan_fused = r.cull_call && (rows_by_step || r.dif_call) && d.plan_fused && r.overlap;
  r.shape = r.dif_call ? CALL_FOLD : r.merged_call ? CALL_MERGED : f.rows256_step ? CALL_ROWS256_STEP : f.rows1024x256 ? CALL_ROWS1024X256 : f.two_pass ? CALL_TWO_PASS :
            f.use_fft8192 ? CALL_FRAMES_8192 : CALL_COLS_ROWS;
  const bool chunked = r.shape == CALL_ROWS256_STEP || r.shape == CALL_ROWS1024X256 || r.shape == CALL_TWO_PASS;
  const int limit = chunked ? call_chunk_limit(f, d) : 0;
  if (limit > 0 && a.nframes > limit) r.chunk = limit;
  switch (r.shape) {
    case CALL_FOLD:  // the plan of the call before, the planned detect stage (of the call before that) and the emit stage behind it ride on the launch
    case CALL_ROWS1024X256: r.ride_first = kRideDet | kRideEmit | kRidePlan; break;
    case CALL_MERGED: r.ride_first = kRideDet | kRideEmit | kRidePlan | kRideRows; break;
    case CALL_ROWS256_STEP:
      r.ride_first = kRidePlan | (f.det_lag2 ? kRideDet : 0) | (d.emit_on_rows ? 0 : kRideEmit);
      r.ride_second = (f.det_lag2 ? 0 : kRideDet) | (d.emit_on_rows ? kRideEmit : 0);
      break;
    case CALL_TWO_PASS:
      // (kRidePlan here is a statement, not a control: the first launch is launch_cols1024, no launch of k_scan_step, and it takes the
      // ready plan itself whenever one waits — on the first chunk, since the call's own plan enters only after the last. launch_chunks
      // never reads ride_first for this shape; the field says what that launch carries, for the record and the table above.)
      r.ride_first = kRidePlan;
      r.ride_second = kRideDet | kRideEmit;
      break;
    default: r.ride_first = kRideDet | kRideEmit; break;
  }
  return r;
}

#ifdef SS_DIAG
// one line per call for SS_ROUTE_RECORD (Diag::route_path) and the host check: the ask, then the route, name=value in this order
inline void print_route(FILE* fp, const CallAsk& a, const CallRoute& r) {
  fprintf(fp, "nframes=%d n_learn=%d device=%d psd=%d rel=%d avg=%d spec=%d shape=%s keeps_no_plane=%d dif_call=%d db_call=%d cull_call=%d ring_by_rows=%d ring_only=%d overlap=%d merged_call=%d plan_fused=%d det_lag2=%d chunk=%d ride_first=%u ride_second=%u\n",
          a.nframes, a.n_learn, a.device, a.psd, a.rel, a.avg, a.spec, call_shape_name(r.shape), r.keeps_no_plane, r.dif_call, r.db_call, r.cull_call, r.ring_by_rows, r.ring_only, r.overlap,
          r.merged_call, r.plan_fused, r.det_lag2, r.chunk, r.ride_first, r.ride_second);
}
#endif

}  // namespace
