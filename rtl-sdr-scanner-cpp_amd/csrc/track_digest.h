// track_digest.h — the device side of the tracking digest (include/specscan_track.h): what host/signal_tracker.cpp reads of a batch's
// rel and avg planes, computed where the planes are, so that neither plane crosses PCIe.
//
//   k_best_blocked  (track_digest_blocked.h) per candidate (f, c): Transmission::getBestIndex(c) at frame f (transmission.cpp:132-154)
//                   — the mode (mostFrequentValue, collection_utils.h:29-50) of the window arg-maxes (getMaxIndex, :8-14) of the newest
//                   ceil(grouping_y / 2) rel rows — and the candidate's own avg value (the sort key of transmission.cpp:95)
//   k_window_peaks  per frame and watch key: arg-max and maximum of the avg row over the key's window (updateSignals, :113-130)
//   k_save_tail     the batch's last ceil(grouping_y / 2) - 1 rel rows, kept for the next batch's first frames
// This file holds the rel rows (RelRows, rel_at), the window peak (window_peak, shared with k_feed_peaks of track_feed.h) and the last
// two kernels. The first candidates' kernel, which walked each candidate's windows bin by bin with every row staged in LDS at once and
// so stopped near 977 bins, was retired in favour of k_best_blocked (DESIGN.md has its measurements).
//
// Arg-max means std::max_element: best = lo; for i in lo + 1 .. hi - 1: if (v[best] < v[i]) best = i. The first maximum wins, a NaN at
// lo wins the window, a NaN anywhere else never wins. k_best_blocked answers from two tables per row that hold exactly that rule;
// window_peak reduces across a wave and states it as a total order (wave_argmax below).
//
// Rel rows are never stored by the fused back end: a row of the batch is rebuilt as the detect stage forms it, psd - thr in fp32
// (noise_learner.cpp:55), or SS_NO_DATA for a learning frame (:49); the unfused back end keeps them, and rows of frames before the
// batch come from the tail k_save_tail left.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ss {

constexpr int kTrackTile = 256;  // bins per k_best_blocked workgroup, and its threads

// Where a rel row lives. Frames are batch-relative: 0 .. nframes - 1 the batch, -tail_rows .. -1 the tail (newest last).
struct RelRows {
  const float* psd;   // fused back end: the batch's dB plane ...
  const float* thr;   // ... and the noise ceiling
  const float* rel;   // unfused back end: the batch's rel rows as stored (psd / thr unused)
  const float* tail;  // [tail_rows][n]
  int n;
  int n_learn;
  int tail_rows;
};

__device__ __forceinline__ float rel_at(const RelRows& r, int frame, int bin) {
  if (frame < 0) return r.tail[(size_t)(r.tail_rows + frame) * r.n + bin];
  if (r.rel) return r.rel[(size_t)frame * r.n + bin];
  if (frame < r.n_learn) return -100.0f;  // SS_NO_DATA
  return r.psd[(size_t)frame * r.n + bin] - r.thr[bin];
}

struct WindowPeaksArgs {
  const float* avg;      // the batch's avg plane
  const int32_t* watch;  // [nwatch]
  int32_t* peak_idx;     // [nframes][nwatch]
  float* peak_avg;
  int n, nframes, nwatch, half;
};

// max_element over lanes. Every lane brings the first maximum of its own bins under the rule "NaN never wins" (v, i; i < 0: nothing);
// of two, the larger value wins and the lower bin on a tie — which is what the sequential walk leaves when its first element is no NaN.
__device__ __forceinline__ void wave_argmax(float& v, int& i) {
  for (int d = 32; d > 0; d >>= 1) {
    const float ov = __shfl_xor(v, d, 64);
    const int oi = __shfl_xor(i, d, 64);
    const bool take = oi >= 0 && (i < 0 || v < ov || (v == ov && oi < i));
    if (take) {
      v = ov;
      i = oi;
    }
  }
}

// The window peak of one (frame, key), by one wave: std::max_element over the bins [key - half, key + half] of the frame's avg row,
// clipped to the row. Every lane returns the same bin.
__device__ __forceinline__ int window_peak(const float* row, int n, int half, int key, int lane) {
  const int lo = key - half < 0 ? 0 : key - half;
  const int hi = key + half + 1 < n ? key + half + 1 : n;
  const float head = row[lo];
  float v = 0.0f;
  int best = -1;
  for (int i = lo + lane; i < hi; i += 64) {
    const float x = row[i];
    if (x != x) continue;  // a NaN behind lo never wins (and one at lo is settled below)
    if (best < 0 || v < x) {
      v = x;
      best = i;
    }
  }
  wave_argmax(v, best);
  return head != head || best < 0 ? lo : best;  // a NaN at lo is never displaced (v[best] < x is false for every x)
}

// one wave per (frame, watch key); 256 threads = four of them
__global__ __launch_bounds__(256) void k_window_peaks(const WindowPeaksArgs a) {
  const int lane = threadIdx.x & 63;
  const long long item = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= (long long)a.nframes * a.nwatch) return;
  const int f = (int)(item / a.nwatch), w = (int)(item % a.nwatch);
  const float* row = a.avg + (size_t)f * a.n;
  const int best = window_peak(row, a.n, a.half, a.watch[w], lane);
  if (lane == 0) {
    a.peak_idx[item] = best;
    a.peak_avg[item] = row[best];
  }
}

// tail_out[k] = rel row of frame nframes - tail_rows + k (k < tail_rows): from the batch, or — a batch shorter than the tail — from
// the old tail (another buffer). n is a multiple of 4 (fft sizes are powers of two >= 64) but the rows are taken bin by bin.
// Rows: where the rel rows live — RelRows, or track_digest_sparse.h's RingRows; anything with n, tail_rows and a rel_at.
template <class Rows>
__device__ __forceinline__ void save_tail_rows(const Rows& rows, int nframes, float* __restrict__ tail_out) {
  const size_t total = (size_t)rows.tail_rows * rows.n;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int k = (int)(e / rows.n), bin = (int)(e % rows.n);
    tail_out[e] = rel_at(rows, nframes - rows.tail_rows + k, bin);
  }
}

__global__ __launch_bounds__(256) void k_save_tail(const RelRows rows, int nframes, float* __restrict__ tail_out) { save_tail_rows(rows, nframes, tail_out); }

}  // namespace ss
