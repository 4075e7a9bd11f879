// ctx_buffers.h — the buffers, streams and events of a scan context whose size and number follow from its form: everything ss_ctx owns
// on the device but the constant tables (specscan.hip uploads those: their builders live in kernel headers) and what a call allocates
// on first use. alloc_ctx_buffers is the one place that sizes and zeroes them. It needs ScanForm, ss_config and device_buffers.h only,
// so tests/host/ctx_buffers_check.cpp runs it against a fake HIP runtime with a failure injected at every call.
#pragma once
#include <cstdint>
#include <vector>

#include "device_buffers.h"
#include "scan_form.h"

namespace {

// k_scan_step's dispatch-order table for one launch shape (ss_ctx::order_tables)
struct OrderTable {
  int key[6];  // FFT / detect / emit / plan / row workgroups of the launch shape, and which order pattern it was built from
  ss::device_buffer<uint32_t> d;
  unsigned long long used = 0;   // 0: free
  std::vector<uint32_t> host;    // what was uploaded (kept alive: the copy is asynchronous)
  hipStream_t stream = nullptr;  // the stream it was uploaded on
};

struct CtxBuffers {
  ss::hip_stream stream;  // every kernel and copy of this chain is ordered on this stream
  ss::device_buffer<uint8_t> d_pass;
  ss::device_buffer<unsigned long long> d_stats;  // ss_get_stats: the device-side counters (detect_fused.h kStat*: tiles tested / culled, wait fallbacks)
  // SS_FLAG_REFERENCE_NAN (reference_nan.h): per-frame first non-finite bins of the batch, the state carried between batches, per-frame poison limits
  ss::device_buffer<int> d_nf;         // [max_batch][4]: first NaN / -inf / +inf bin of every frame of the batch (n: none)
  ss::device_buffer<int> d_nan_state;  // ss::NanState
  ss::device_buffer<int> d_bad_from;   // [max_batch]: bins >= this are NaN in the reference's avg row (n: none)
  // back end, fused path: the averager ring (hist_rows rows) and the per-frame candidate counts in rotation
  ss::device_buffer<float> d_hist;
  ss::device_buffer<int> d_cnt3[3 * kMaxQueues];
  // back end, unfused path (any other grouping): one buffer holds the ring rows + the batch rows
  ss::device_buffer<float> d_rel;  // (G-1) history rows + max_batch rows
  ss::device_buffer<float> d_hist_tmp, d_avgy;
  // the rotating sets: internal PSD planes; mask / avg planes / the library's copy of the candidate offsets
  ss::device_buffer<float> d_psd2[2 * kMaxQueues + 1];
  ss::device_buffer<float> d_avg2[2 * kMaxQueues];
  ss::device_buffer<uint32_t> d_mask2[2 * kMaxQueues];
  ss::device_buffer<int> d_off4[2 * kMaxQueues];
  // Tile culling (8192 points, detect_fused.h): the FFT role's per-column maxima of a call's PSD rows, [32][max_batch],
  // rotating with the mask / avg / offset buffers (written by the call's FFT launch, read by its detect stage)
  ss::device_buffer<float> d_segsum[2 * kMaxQueues];
  ss::device_buffer<int> d_live[2 * kMaxQueues];  // DetectArgs::live: the tiles of a call that must be evaluated (plan role -> the launch's other workgroups)
  // deep pipelining: the queues, their halo buffers ([kHistRows][n] each: written by launch L, read by detect(L) in launch L + nq) and events
  ss::hip_stream s_ab[kMaxQueues];
  ss::device_buffer<float> d_halo[2 * kMaxQueues];
  ss::hip_event ev_launch[32], ev_in[4], ev_join[kMaxQueues], ev_tail;
  ss::device_buffer<unsigned long long> d_canary;  // SS_DIAG only (Diag::canary): [64][2]
  ss::hip_event ev_canary;
  std::vector<OrderTable> order_tables;  // one per launch shape met so far (a handful: steady state, pipeline fill, drain)
  ss::device_buffer<int> d_counts;
  // spectrogram: in-detect form, two alternating buffers of partial sums; deep pipelining, a slot per call and the stream that adds them
  ss::device_buffer<float> d_spec_part2[2];
  ss::device_buffer<float> d_spec_ring;
  size_t spec_slot_floats = 0;
  ss::hip_stream s_fold;
  ss::hip_event ev_fold_src[kMaxQueues], ev_fold_done[16];
  ss::device_buffer<float> d_spec_partial;  // the stand-alone form's
  ss::device_buffer<float2> d_work;   // four-step intermediate (N > 8192)
  ss::device_buffer<float2> d_work2;  // one launch per call: the second one
  ss::device_buffer<float> d_perm_tmp;  // the fold: 35 rows, the window on its way from one order to the other
  // tile culling, long transforms
  ss::device_buffer<float> d_zero_row;  // n zeros (what a ring-only call's detect stage subtracts from rows that are noise-relative already)
  ss::device_buffer<float> d_smax;      // the maximum of every 32-bin run per frame, a ring of smax_rows frames
  ss::device_buffer<int> d_tlist[2 * kMaxQueues];  // the tiles that must be evaluated (k_plan_long), rotating with the mask buffers
};

// Everything above, sized from the form; what must start as zeros is zeroed on b.stream (or synchronously): the caller waits for the stream.
inline void alloc_ctx_buffers(CtxBuffers& b, const ScanForm& f, const ss_config& cfg, bool canary, ss::hip_steps& made) {
  const size_t n = (size_t)f.n, batch = (size_t)cfg.max_batch, plane = n * batch;
  const int G = cfg.grouping_y;
  made.stream(b.stream);
  made.alloc(b.d_pass, n);
  made.alloc(b.d_stats, kFormStatWords).zero_async(b.d_stats, kFormStatWords, b.stream);
  if (f.ref_nan) made.alloc(b.d_nf, 4 * batch).alloc(b.d_bad_from, batch).alloc(b.d_nan_state, kFormNanStateInts);
  if (f.fused) {
    made.alloc(b.d_hist, n * (size_t)f.hist_rows).zero_async(b.d_hist, n * (size_t)kHistRows, b.stream);  // Averager ctor, averager.cpp:7-12
    for (int k = 0; k < f.ncnt; ++k) made.alloc(b.d_cnt3[k], batch).zero_async(b.d_cnt3[k], batch, b.stream);
  } else {
    made.alloc(b.d_rel, n * (size_t)(G - 1 + cfg.max_batch)).alloc(b.d_hist_tmp, n * (size_t)(G > 1 ? G - 1 : 1)).alloc(b.d_avgy, plane);
    made.zero_async(b.d_rel, n * (size_t)(G - 1 + cfg.max_batch), b.stream);
  }
  for (int k = 0; k < f.npsd; ++k) made.alloc(b.d_psd2[k], plane);
  for (int k = 0; k < f.nbuf; ++k) {
    made.alloc(b.d_avg2[k], plane);
    made.alloc(b.d_mask2[k], (n / 32) * batch).zero_async(b.d_mask2[k], (n / 32) * batch, b.stream);  // (tile culling relies on it: EmitArgs::clear_masks)
    made.alloc(b.d_off4[k], batch + 1);
  }
  if (f.cull)
    for (int k = 0; k < f.nbuf; ++k) {
      made.alloc(b.d_segsum[k], 32 * batch);
      made.alloc(b.d_live[k], kFormLiveInts).zero_async(b.d_live[k], kFormLiveInts, b.stream);
    }
  if (f.deep) {
    if (canary) {
      made.alloc(b.d_canary, 128).then([&] { return hipMemset(b.d_canary, 0, sizeof(unsigned long long) * 128); }, "hipMemset");
      made.event(b.ev_canary);
    }
    for (int k = 0; k < f.nq; ++k) made.stream(b.s_ab[k]);
    for (int k = 0; k < 2 * f.nq; ++k)  // (+ the halo frames' per-column maxima behind their rows: halo_segsum_of)
      made.alloc(b.d_halo[k], n * (size_t)kHistRows + 32 * (size_t)kFormHaloSegPitch);
    for (auto& e : b.ev_launch) made.event(e);
    for (auto& e : b.ev_in) made.event(e);
    for (auto& e : b.ev_join) made.event(e);
    made.event(b.ev_tail);
  }
  if (f.step_path) {
    b.order_tables.resize(16);
    for (auto& t : b.order_tables) made.alloc(t.d, f.order_capacity);
  }
  made.alloc(b.d_counts, batch);
  if (f.spec_n > 0) {
    if (f.spec_in_detect) {
      const size_t tiles = (batch + kFusedTF - 1) / kFusedTF + 1;
      for (auto& p : b.d_spec_part2) made.alloc(p, (size_t)f.spec_n * tiles);
      if (f.deep) {  // one slot of partial sums per call in flight or not yet added to its container (ss_ctx::deep_folds)
        b.spec_slot_floats = (size_t)f.spec_n * tiles;
        made.alloc(b.d_spec_ring, b.spec_slot_floats * (size_t)kDeepSpecSlots).stream(b.s_fold);
        for (auto& e : b.ev_fold_src) made.event(e);
        for (auto& e : b.ev_fold_done) made.event(e);
      }
    } else {
      made.alloc(b.d_spec_partial, (size_t)f.spec_n * ((batch + 31) / 32));
    }
  }
  if (f.logn > 13) made.alloc(b.d_work, plane);
  // (the one-launch form only takes calls of up to merge_max frames: the second work buffer need not hold more)
  if (f.merge) made.alloc(b.d_work2, n * (size_t)std::min(cfg.max_batch, f.merge_max));
  if (f.dif8) made.alloc(b.d_perm_tmp, n * (size_t)kHistRows);
  if (f.cull_long) {
    made.alloc(b.d_zero_row, n).then([&] { return hipMemset(b.d_zero_row, 0, sizeof(float) * n); }, "hipMemset");
    made.alloc(b.d_smax, (size_t)f.smax_rows * (n / 32));
    if (f.rows1024x256) made.zero_async(b.d_smax, (size_t)f.smax_rows * (n / 32), b.stream);  // (keys: 0 = nothing seen)
    const size_t max_tiles = (batch / kFusedTF + 2) * (n / 256);
    for (int k = 0; k < std::max(2, f.nbuf); ++k) made.alloc(b.d_tlist[k], max_tiles + 2);  // (count, entries, one slot behind an odd count)
  }
}

}  // namespace
