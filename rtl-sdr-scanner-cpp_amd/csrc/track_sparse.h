// track_sparse.h — the tracked feed on a scan context that keeps no planes (stf_create_sparse, include/specscan_track_feed.h).
//
// Without SS_FLAG_KEEP_PLANES a batch leaves avg only where a tile found hits (DetectArgs::avg_sparse). The digest's candidates need no
// more than that; its window peaks (k_feed_peaks) read avg over the window of every watch key in every frame of the batch, hits or
// not, culled tile or not. So between the watch list and the peaks the tile columns those windows touch are evaluated once more, by
// the tile code that ships, on the batch's own arguments, with the batch's sparse plane as avg_out:
//
//   k_feed_watch_cols   watch[0 .. min(nwatch, max_watch)) -> one flag per 256-bin tile column (an overflowed list marks nothing)
//   k_watch_tiles       grid = the batch's frame tiles x columns; a workgroup of an unmarked column returns at once, the others count
//                       themselves and run detect_tile<21, 21, 16, 256, false>
//
// Same body, same inputs: every value is the one a context with SS_FLAG_KEEP_PLANES writes, bit for bit. What the replay must NOT do
// is the host's business (host_track_feed.h, stf_replay_watch_tiles): mask bits and counts go to scratch of the tracker's own, no ring row, rel row,
// statistic or spectrogram sum is written.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include "detect_fused.h"
#include "track_feed.h"
#define SS_WATCH_HD __host__ __device__ inline
#else  // (tests/host/watch_cols_check.cpp: plain C++)
#define SS_WATCH_HD inline
#endif

namespace ss {

constexpr int kWatchCol = 256;  // bins per tile column: DetectTile<..., 256>::TB
constexpr int kWatchTF = 16;    // frames per tile (specscan.hip: kFusedTF)

struct WatchColRange {
  int lo, hi;  // first and last tile column the window touches
};

// The window of k_feed_peaks / window_peak around `key`, [max(0, key - half), min(n - 1, key + half)], in tile columns.
// key in [0, n), half >= 0 (tests/host/watch_cols_check.cpp holds it against a loop over the bins).
SS_WATCH_HD WatchColRange watch_col_range(int key, int half, int n) {
  const int lo = key - half < 0 ? 0 : key - half;
  const int hi = key + half + 1 < n ? key + half : n - 1;
  return WatchColRange{lo / kWatchCol, hi / kWatchCol};
}

#ifdef __HIPCC__

// One workgroup. The list's length is the header's; more than max_watch keys: no list, no peaks (k_feed_peaks), nothing marked.
// Every writer of a flag in the second phase writes 1: plain stores.
__global__ __launch_bounds__(256) void k_feed_watch_cols(const int32_t* __restrict__ watch, const FeedDigestHeader* __restrict__ hdr, int n, int half,
                                                        int32_t* __restrict__ col_flag) {
  const int ncols = (n + kWatchCol - 1) / kWatchCol;
  for (int c = (int)threadIdx.x; c < ncols; c += 256) col_flag[c] = 0;
  __syncthreads();
  const int nwatch = (hdr->flags & kFeedOverflow) ? 0 : hdr->nwatch;
  for (int w = (int)threadIdx.x; w < nwatch; w += 256) {
    const int key = watch[w];
    if (key < 0 || key >= n) continue;  // (k_feed_scatter writes bins of [0, n) only)
    const WatchColRange r = watch_col_range(key, half, n);
    for (int c = r.lo; c <= r.hi; ++c) col_flag[c] = 1;
  }
}

struct WatchTilesArgs {
  DetectArgs det;                 // the batch's own, with the replay's overrides (stf_enqueue)
  const int32_t* col_flag;        // [ceil(n / 256)]
  unsigned long long* evaluated;  // += 1 per tile that runs
};

// grid: ceil((nframes + shift) / 16) x ceil(n / 256) workgroups, numbered as k_detect_fused numbers its tiles
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void k_watch_tiles(const WatchTilesArgs a) {
  using T = DetectTile<21, 21, kWatchTF, kWatchCol>;
  __shared__ __attribute__((aligned(16))) float tile[kWatchTF * T::P];
  __shared__ int cnt[kWatchTF];
  const int cols = (a.det.n + kWatchCol - 1) / kWatchCol;
  if (a.col_flag[(int)blockIdx.x % cols] == 0) return;  // (block-uniform)
  if (threadIdx.x == 0) atomicAdd(a.evaluated, 1ull);
  detect_tile<21, 21, kWatchTF, kWatchCol, false>(a.det, (int)blockIdx.x, (int)threadIdx.x, tile, cnt, true);
}

#endif  // __HIPCC__

}  // namespace ss
