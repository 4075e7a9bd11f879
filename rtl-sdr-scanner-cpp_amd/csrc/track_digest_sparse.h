// track_digest_sparse.h — the tracking digest (st_digest) on a scan context that keeps no planes (st_create_sparse,
// include/specscan_track_digest_sparse.h). Three things differ from the digest on kept planes:
//
//   the rel rows   a call that leaves no dB plane leaves its rows in the averager ring's buffer (ss_ctx::last_rel_rows): batch frame f
//                  is row f, as dB values (ss_ctx::last_rows_db; rel = x - thr[bin], the tiles' own fp32 subtraction) and, after a
//                  fold call, in the fold's blocked order (fft65536_dif8.h: dif_bin_offset). RingRows / ring_cell say where a cell
//                  is and what to do with it — what ss_read_window(SS_PLANE_REL) does on the host (read_perm8_row, sub_thr_window) —
//                  and k_ring_best / k_ring_tail are k_best_blocked's and k_save_tail's bodies over that source. Frames before the
//                  batch come from the tail as ever: it holds bin-order rel values whatever the call that produced them.
//   the columns    k_digest_cols marks the 256-bin tile columns the watch windows touch from the list st_digest formed on the host
//                  (watch_col_range of track_sparse.h; k_feed_watch_cols reads a header the synchronous digest does not have)
//   the replay     k_digest_tiles<LAYOUT>: k_watch_tiles' recipe with the tile of the batch's own form — rows in bin order (0), the
//                  radix-8 fold's (3), the radix-16 fold's (4), as scan_step.h's step_detect_layout names them
//
// ring_cell is a plain function: tests/host/ring_rows_check.cpp compiles it for the host.
#pragma once
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#include "track_digest_blocked.h"
#include "track_sparse.h"
#define SS_RING_HD __host__ __device__ inline
#else
#define SS_RING_HD inline
#endif

namespace ss {

// The rows a no-plane call left, and the tail in front of them. Frames are batch-relative, as RelRows' are.
struct RingRows {
  const float* rows;  // ss_ctx::last_rel_rows: [nframes][n]
  const float* thr;   // the noise ceiling, in bin order
  const float* tail;  // [tail_rows][n], bin order, rel values
  int n;
  int n_learn;
  int tail_rows;
  int logq;            // 0: the rows are in bin order; 3, 4: in the radix-8 / radix-16 fold's blocked order
  int db_from, db_to;  // the frames [db_from, db_to) hold dB values, every other one rel values as stored (settled since, or written so)
};

enum RingCellKind { kRingStored = 0, kRingMinusThr = 1, kRingNoData = 2 };

struct RingCell {
  size_t at;  // index into RingRows::rows
  int kind;   // the value as stored; the value minus thr[bin]; SS_NO_DATA (a learning frame among the dB rows)
};

// Where bin `bin` of a row sits: the bin itself, or — the fold's rows, 8192 Q bins (Q = 1 << logq) in blocks of 32 Q — bin Q k' + g at
// (k' / 32) * 32 Q + 32 g + k' % 32 (dif_bin_offset, restated here so that a host compiler can read this file)
SS_RING_HD int ring_bin_offset(int bin, int logq) {
  if (logq == 0) return bin;
  const int g = bin & ((1 << logq) - 1), k = bin >> logq;
  return ((k >> 5) << (5 + logq)) + (g << 5) + (k & 31);
}

// cell (frame, bin) of the batch, frame in [0, nframes), bin in [0, n)
SS_RING_HD RingCell ring_cell(int n, int n_learn, int logq, int db_from, int db_to, int frame, int bin) {
  const bool db = frame >= db_from && frame < db_to;
  return RingCell{(size_t)frame * (size_t)n + (size_t)ring_bin_offset(bin, logq), !db ? kRingStored : frame < n_learn ? kRingNoData : kRingMinusThr};
}

struct RingDbRange {
  int from, to;
};

// RingRows::db_from / db_to of a batch of nframes rows: rows_db = the call left dB values (ss_ctx::last_rows_db); [settled_a, settled_b)
// = the batch frames whose rows the host has turned into rel values in place since (settle_ring_db: the newest rows of the ring's
// window, so the range reaches the batch's end or lies in front of the batch; a >= b: none).
SS_RING_HD RingDbRange ring_db_range(int nframes, bool rows_db, long long settled_a, long long settled_b) {
  if (!rows_db) return RingDbRange{0, 0};
  if (settled_a >= settled_b || settled_b <= 0 || settled_a >= nframes) return RingDbRange{0, nframes};
  if (settled_a <= 0) return RingDbRange{settled_b < nframes ? (int)settled_b : nframes, nframes};
  return RingDbRange{0, (int)settled_a};
}

#ifdef __HIPCC__

__device__ __forceinline__ float rel_at(const RingRows& r, int frame, int bin) {
  if (frame < 0) return r.tail[(size_t)(r.tail_rows + frame) * r.n + bin];
  const RingCell c = ring_cell(r.n, r.n_learn, r.logq, r.db_from, r.db_to, frame, bin);
  if (c.kind == kRingNoData) return -100.0f;  // SS_NO_DATA
  const float x = r.rows[c.at];
  return c.kind == kRingMinusThr ? x - r.thr[bin] : x;
}

// k_best_blocked over the ring's rows: same grid, same dynamic LDS (blocked_lds_bytes)
__global__ __launch_bounds__(kTrackTile) void k_ring_best(const CandBestArgsOf<RingRows> a) {
  extern __shared__ float lds_ring_best[];
  best_blocked_tile(a, lds_ring_best);
}

// k_save_tail over the ring's rows: the tail it writes is in bin order
__global__ __launch_bounds__(256) void k_ring_tail(const RingRows rows, int nframes, float* __restrict__ tail_out) { save_tail_rows(rows, nframes, tail_out); }

// One workgroup: col_flag[c] = 1 for every tile column a window of watch[0 .. nwatch) touches, 0 for the others.
// Every writer of a flag in the second phase writes 1: plain stores.
__global__ __launch_bounds__(256) void k_digest_cols(const int32_t* __restrict__ watch, int nwatch, int n, int half, int32_t* __restrict__ col_flag) {
  const int ncols = (n + kWatchCol - 1) / kWatchCol;
  for (int c = (int)threadIdx.x; c < ncols; c += 256) col_flag[c] = 0;
  __syncthreads();
  for (int w = (int)threadIdx.x; w < nwatch; w += 256) {
    const int key = watch[w];
    if (key < 0 || key >= n) continue;  // (st_digest checks its keys; cand_best is checked before the list is formed)
    const WatchColRange r = watch_col_range(key, half, n);
    for (int c = r.lo; c <= r.hi; ++c) col_flag[c] = 1;
  }
}

// grid: ceil((nframes + shift) / 16) x ceil(n / 256) workgroups, numbered as k_detect_fused numbers its tiles; a workgroup of an
// unmarked column returns at once, a marked one counts itself. LAYOUT: detect_tile's PERM8.
// The fold's tile as k_scan_step runs it holds two columns' 36 rows in registers at once (124 VGPRs, four waves per SIMD): worth it where a
// residue's transform waits for the workgroup's slot, not in a launch of tiles alone. Here the tile takes its columns in two passes
// (detect_tile's ONE_FLIGHT = false: the same values through the same arithmetic): 62 VGPRs, eight waves per SIMD, no scratch.
template <int LAYOUT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void k_digest_tiles(const WatchTilesArgs a) {
  using T = DetectTile<21, 21, kWatchTF, kWatchCol>;
  __shared__ __attribute__((aligned(16))) float tile[kWatchTF * T::P];
  __shared__ int cnt[kWatchTF];
  const int cols = (a.det.n + kWatchCol - 1) / kWatchCol;
  if (a.col_flag[(int)blockIdx.x % cols] == 0) return;  // (block-uniform)
  if (threadIdx.x == 0) atomicAdd(a.evaluated, 1ull);
  detect_tile<21, 21, kWatchTF, kWatchCol, false, LAYOUT, false>(a.det, (int)blockIdx.x, (int)threadIdx.x, tile, cnt, true);
}

#endif  // __HIPCC__

}  // namespace ss
