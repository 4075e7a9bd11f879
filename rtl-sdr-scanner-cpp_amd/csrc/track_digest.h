// track_digest.h — the device side of the tracking digest (include/specscan_track.h): what host/signal_tracker.cpp reads of a batch's
// rel and avg planes, computed where the planes are, so that neither plane crosses PCIe.
//
//   k_cand_best     per candidate (f, c): Transmission::getBestIndex(c) at frame f (transmission.cpp:132-154) — the mode
//                   (mostFrequentValue, collection_utils.h:29-50) of the window arg-maxes (getMaxIndex, :8-14) of the newest
//                   ceil(grouping_y / 2) rel rows — and the candidate's own avg value (the sort key of transmission.cpp:95)
//   k_window_peaks  per frame and watch key: arg-max and maximum of the avg row over the key's window (updateSignals, :113-130)
//   k_save_tail     the batch's last ceil(grouping_y / 2) - 1 rel rows, kept for the next batch's first frames
//
// Arg-max means std::max_element: best = lo; for i in lo + 1 .. hi - 1: if (v[best] < v[i]) best = i. The first maximum wins, a NaN at
// lo wins the window, a NaN anywhere else never wins. k_cand_best walks its windows in exactly that order (one lane per candidate, the
// rows staged in LDS); k_window_peaks reduces across a wave and states the same rule as a total order (wave_argmax below).
//
// Rel rows are never stored by the fused back end: a row of the batch is rebuilt as the detect stage forms it, psd - thr in fp32
// (noise_learner.cpp:55), or SS_NO_DATA for a learning frame (:49); the unfused back end keeps them, and rows of frames before the
// batch come from the tail k_save_tail left.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ss {

constexpr int kTrackTile = 256;  // bins per k_cand_best workgroup, and its threads

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

struct CandBestArgs {
  RelRows rows;
  const float* avg;         // the batch's avg plane
  const int32_t* cand_off;  // [nframes + 1], clipped to ncand
  const int32_t* cand_idx;  // [ncand], ascending inside a frame
  int32_t* cand_best;       // [ncand]
  float* cand_avg;          // [ncand]
  int nframes;
  int tiles;       // ceil(n / kTrackTile)
  int half;        // group_size / 2
  int nrows;       // ceil(grouping_y / 2) = tail_rows + 1
  int width;       // staged bins per row: kTrackTile + 2 * half
  float start_level;
};

// first candidate of the frame's list [a, b) at or above bin: the lists are ascending
__device__ __forceinline__ int cand_lower_bound(const int32_t* idx, int a, int b, int bin) {
  while (a < b) {
    const int m = (a + b) >> 1;
    if (idx[m] < bin) a = m + 1;
    else b = m;
  }
  return a;
}

// grid nframes * tiles, 256 threads, dynamic LDS: nrows * width floats + nrows * 256 ints.
// A workgroup whose tile of its frame holds no candidate returns at once; otherwise it stages the nrows rel rows of the bins its
// candidates' windows can touch, and lane t takes the tile's t-th candidate (a tile holds at most 256).
__global__ __launch_bounds__(kTrackTile) void k_cand_best(const CandBestArgs a) {
  extern __shared__ float lds[];
  const int n = a.rows.n;
  const int f = blockIdx.x / a.tiles;
  const int t0 = (blockIdx.x % a.tiles) * kTrackTile;
  const int list_lo = a.cand_off[f], list_hi = a.cand_off[f + 1];
  if (list_lo >= list_hi) return;
  const int first = cand_lower_bound(a.cand_idx, list_lo, list_hi, t0);
  const int last = cand_lower_bound(a.cand_idx, first, list_hi, t0 + kTrackTile);
  if (first >= last) return;  // (uniform over the workgroup: nobody waits at the barrier below)
  float* rows = lds;                                                  // [nrows][width]
  int* sorted = reinterpret_cast<int*>(lds + a.nrows * a.width);      // [nrows][256]: lane t's qualifying arg-maxes, ascending
  const int base = t0 - a.half;                                       // bin of rows[r][0]
  const int s_lo = base < 0 ? 0 : base;
  const int s_hi = t0 + kTrackTile - 1 + a.half < n ? t0 + kTrackTile - 1 + a.half : n - 1;  // last staged bin
  for (int r = 0; r < a.nrows; ++r) {
    const int frame = f - (a.nrows - 1) + r;
    for (int i = s_lo + (int)threadIdx.x; i <= s_hi; i += kTrackTile) rows[r * a.width + (i - base)] = rel_at(a.rows, frame, i);
  }
  __syncthreads();
  const int j = first + (int)threadIdx.x;
  if (j >= last) return;
  const int c = a.cand_idx[j];
  const int lo = c - a.half < 0 ? 0 : c - a.half;
  const int hi = c + a.half + 1 < n ? c + a.half + 1 : n;
  int* mine = sorted + threadIdx.x;
  int m = 0;
  for (int r = 0; r < a.nrows; ++r) {
    const float* row = rows + r * a.width - base;
    int best = lo;
    float vbest = row[lo];
    for (int i = lo + 1; i < hi; ++i) {
      const float v = row[i];
      if (vbest < v) {
        best = i;
        vbest = v;
      }
    }
    if (a.start_level <= vbest) {  // insert into the ascending list
      int k = m;
      while (k > 0 && mine[(k - 1) * kTrackTile] > best) {
        mine[k * kTrackTile] = mine[(k - 1) * kTrackTile];
        --k;
      }
      mine[k * kTrackTile] = best;
      ++m;
    }
  }
  int result = c;  // no row qualifies: the candidate itself (signal_tracker.cpp, getBestIndex)
  if (m > 0) {
    // runs of equal values: the longest count, how many runs reach it, and of those the one at position size / 2
    int top = 0, ties = 0;
    for (int i = 0; i < m;) {
      const int v = mine[i * kTrackTile];
      int e = i + 1;
      while (e < m && mine[e * kTrackTile] == v) ++e;
      if (e - i > top) {
        top = e - i;
        ties = 1;
      } else if (e - i == top) {
        ++ties;
      }
      i = e;
    }
    int want = ties / 2;
    for (int i = 0; i < m;) {
      const int v = mine[i * kTrackTile];
      int e = i + 1;
      while (e < m && mine[e * kTrackTile] == v) ++e;
      if (e - i == top) {
        if (want == 0) {
          result = v;
          break;
        }
        --want;
      }
      i = e;
    }
  }
  a.cand_best[j] = result;
  a.cand_avg[j] = a.avg[(size_t)f * n + c];
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

// one wave per (frame, watch key); 256 threads = four of them
__global__ __launch_bounds__(256) void k_window_peaks(const WindowPeaksArgs a) {
  const int lane = threadIdx.x & 63;
  const long long item = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= (long long)a.nframes * a.nwatch) return;
  const int f = (int)(item / a.nwatch), w = (int)(item % a.nwatch);
  const int key = a.watch[w];
  const int lo = key - a.half < 0 ? 0 : key - a.half;
  const int hi = key + a.half + 1 < a.n ? key + a.half + 1 : a.n;
  const float* row = a.avg + (size_t)f * a.n;
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
  if (head != head || best < 0) best = lo;  // a NaN at lo is never displaced (v[best] < x is false for every x)
  if (lane == 0) {
    a.peak_idx[item] = best;
    a.peak_avg[item] = row[best];
  }
}

// tail_out[k] = rel row of frame nframes - tail_rows + k (k < tail_rows): from the batch, or — a batch shorter than the tail — from
// the old tail (another buffer). n is a multiple of 4 (fft sizes are powers of two >= 64) but the rows are taken bin by bin.
__global__ __launch_bounds__(256) void k_save_tail(const RelRows rows, int nframes, float* __restrict__ tail_out) {
  const size_t total = (size_t)rows.tail_rows * rows.n;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int k = (int)(e / rows.n), bin = (int)(e % rows.n);
    tail_out[e] = rel_at(rows, nframes - rows.tail_rows + k, bin);
  }
}

}  // namespace ss
