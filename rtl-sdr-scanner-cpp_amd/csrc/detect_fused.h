// detect_fused.h — fused back end for the reference's own grouping (GROUPING_X = GROUPING_Y = 21,
// sources/config.h:28-29). Other groupings use the unfused kernels of detect_kernels.h.
//
// k_detect_fused reads the PSD plane ONCE and produces candidate mask bits + per-frame counts; nothing
// else is written unless the caller asked for the rel / avg planes:
//   rel(f,i) = psd(f,i) - thr(i)   (-100 for learning frames; ring rows before the batch come from hist_in)
//                                                            sources/radio/blocks/noise_learner.cpp:49,55
//   avgY     = mean over the newest G frames (or -100 during the averager warm-up)   sources/radio/averager.cpp:52-61
//   avgXY    = centred GX-bin mean of avgY, window clipped at the band edges         sources/utils/utils.cpp:31-53
//   hit      = start_level <= avgXY && pass(i)                                       sources/radio/blocks/transmission.cpp:91
//
// Tiling: one workgroup = TF frames x 256 bins. Frame tiles are aligned to the ABSOLUTE frame index (frames
// since the last reset), not to the batch: tile boundaries, and with them every rounding below, do not depend
// on how the frame stream is cut into batches (bit for bit: tests/test_gpu_fullsize.py). A batch that starts
// in the middle of a tile re-reads the tile's earlier rows from the ring, which therefore holds
// H = G-1 + TF-1 rows instead of the Averager's G-1.
//   phase 1: thread = column. The G-1+TF rel values of the column sit in registers. The first time mean of
//            the tile is a fixed-order G-term sum, oldest frame first; the next TF-1 slide it the way the
//            reference's Averager does (sum -= oldest row; sum += new row, averager.cpp:14-25,40-50) —
//            restarted every TF frames, so the drift of the reference's never-re-zeroed sum cannot build up.
//   the avgY tile goes through LDS once and changes owner
//   phase 2: thread = (frame, 16-bin segment). 36 avgY values in registers; the first window of the
//            segment is a fixed-order GX-term sum, the next 15 slide it the way the reference does
//            (sum -= leaving bin; sum += entering bin, utils.cpp:39-48) — restarted every 16 bins, so the
//            drift of the reference's whole-row running sum never builds up.
// Tiles of a steady-state batch (no ring rows, no learning frames, all TF frames inside the batch) take a
// straight-line path; the few others take a general path. The tiles that hold the newest H frames of the
// batch also write them to hist_out, the ring the next batch starts from.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "detect_kernels.h"
#include "fft1024_kernels.h"
#include "fft256_kernels.h"
#include "fft8192_v2.h"

namespace ss {

// The detect tiles' row loads, default cache policy (tried: non-temporal — no gain)
__device__ __forceinline__ float load_row_value(const char* p) { return *reinterpret_cast<const float*>(p); }

// Tile culling (8192-point frames): a tile that provably holds no candidate need not read its 36 x 276 rel values at all. The
// bound: the FFT role leaves, per frame and 256-bin tile column, the maximum dB value M_g over the column's bins and 32 more on
// either side (Fft8192Args::segsum); with m the minimum of the noise ceiling over the same 320 bins (thr_tilemin, kept up to date
// by k_thr_tilemin) every rel = fl(psd - thr) of frame g is <= fl(M_g - m) because rounding is monotonic, so the 21-bin mean of
// any frame is, and the 21 x 21 mean ending at frame f is at most mean(M_{f-20} .. M_f) - m. The fp32 sums behind a mean of 441
// such values (|rel| < 1000 dB: finite dB values lie in [-450, 400]) and behind the bound are off by < 0.01 dB, so a tile whose
// bound stays below start_level - kCullMargin for each of its 16 frames has no candidate whatever the rounding. -inf and NaN rows need no care: they make no candidates either (a NaN never passes `start_level <= avg`), and
// +inf is not below any level. The decision is exact — culled tiles produce what the full evaluation would have produced:
// zero mask bits, no counts (tests/test_gpu_cull.py: identical candidate lists with SS_FLAG_NO_CULL and against oracle/_ref).
// What a culled tile must not cost is a workgroup: inside the step kernel every detect workgroup holds one of a CU's four
// slots for ~7 us whatever it does (its first loads queue behind the frames the CU streams), and with five tiles in six
// culled that was a third of the step; a launch of their own behind the step costs two kernel boundaries
// per queue instead (measured: worse). So the decision is taken for ALL tiles of a call by a handful of workgroups (the
// plan role of k_scan_step, dispatched first: one lane per tile) which compact the tiles that must be evaluated into a
// list and clear the mask words of the others; the FFT workgroups of the same launch — which live ~14 us before they
// need to know — pick the lists up when their frame is done (scan_step.h). Plan workgroup s owns the tiles of 8 (or 4) tile
// columns and a list of its own; consumer p serves list p mod S, entries 2 (p div S) and the next one, so all it has to
// read is ONE header word, count | ready. The hand-over inside the launch follows MI355X_MICROARCH.md: write-through (sc1) stores
// for the entries, drained (vmcnt 0 — not a release fence: that would write back an L2 full of dB rows being produced),
// then the header word, sc1; consumers read header and entries with sc1 loads. Plan workgroups never wait for anybody
// and are dispatched before every consumer in practice — but HIP promises nothing about dispatch order, so no consumer
// relies on it: a consumer polls its list's header a bounded number of times (StepArgs::wait_limit) and then makes the plan
// of its list ITSELF (plan_tiles again, with the same inputs: the same list, the same count, written to the same words — two
// writers of identical values are harmless) and goes on from there; ss_get_stats counts those workgroups. Nothing in a launch
// waits without bound (scan_step.h; tests/test_gpu_wait_bound.py runs the chain with plan workgroups that never publish,
// and under HSA_CU_MASK with a handful of CUs).
constexpr float kCullMargin = 0.0625f;
// (ss_get_stats) The counters live in kStatShards copies a cache line apart and a workgroup adds to the copy of its block index:
// a thousand plan workgroups adding to ONE word queue up behind each other at 12 ns apiece (measured: k_plan_long went from 7 to
// 20 us per 16-frame call of 2^20 points); the host adds the copies up.
enum { kStatTested = 0, kStatCulled = 1, kStatWaitFallbacks = 2, kStatWords = 4, kStatShards = 64, kStatShardStride = 16 };
__device__ __forceinline__ unsigned long long* stat_word(unsigned long long* stats, int which) { return stats + (blockIdx.x & (kStatShards - 1)) * kStatShardStride + which; }

// s / D for a compile-time integer D, correctly rounded like the reference's `sum / count`
// (float / int -> IEEE division): q0 = s * RN(1/D), one Newton correction with exact residuals (FMA).
// Verified against the hardware division for every finite float by ss_selftest (tests/test_gpu_selftest.py).
// An infinite sum (a -inf dB row inside the window: a frame of zeros) stays the infinity the IEEE division gives — the residual
// inf - inf is not a number, and then the first quotient is the answer (round 4: until then the engine's avg plane held NaN where
// the reference's holds -inf; no candidate either way).
template <int D>
__device__ __forceinline__ float div_const(float s) {
  constexpr float r = 1.0f / (float)D;
  const float q0 = s * r;
  const float e = fmaf(-(float)D, q0, s);
  const float q1 = fmaf(e, r, q0);
  return q1 == q1 ? q1 : q0;
}

template <int G, int GX, int TF, int TB_ = 256>
struct DetectTile {
  static constexpr int A = GX / 2;
  static constexpr int TB = TB_;           // bins per tile = threads per workgroup
  static constexpr int P = TB + 2 * A;     // tile pitch in floats (276 for GX = 21: rows stay 16-byte aligned)
  static constexpr int ROWS = G - 1 + TF;  // rel rows a column needs
  static constexpr int H = G - 1 + TF - 1; // ring rows kept between batches (a tile may start TF-1 frames before the batch)
  static constexpr int SEGW = 16;          // bins per phase-2 thread
  static constexpr int NSEG = TB / SEGW;   // 16
  static constexpr int YW = SEGW + 2 * A;  // 36 avgY values per phase-2 thread
  static_assert((2 * A) % 4 == 0 && P % 4 == 0 && YW % 4 == 0, "tile rows must stay 16-byte aligned");
  static_assert(TF == 16 || TF == 32, "phase 2 pairs lanes l and l+TF inside one wave");
};

struct DetectArgs {
  const float* psd;
  const float* thr;
  const float* hist_in;
  float* hist_out;
  // Rows before the batch straight from the PREVIOUS call's PSD plane instead of the ring (null: the ring). rel = psd - thr is
  // the same fp32 subtraction either way, so the results are the same bits; what changes is the dependence: the ring was
  // written by the previous call's detect stage, the plane by its FFT stage (specscan.hip, deep pipelining). Only between
  // calls without learning frames; halo_rows = frames of that plane (>= H).
  const float* halo_psd;
  int halo_rows;
  // Ring rows that hold dB values, not noise-relative ones (round 5): the FFT stage of a long transform's detect-mode call leaves its
  // rows in the ring's buffer as dB values — the ceiling loads cost its launch 7-9 % — and the tiles that are evaluated subtract the
  // ceiling, the same fp32 subtraction on the same values (noise_learner.cpp:55). Rows of the window from batch-relative frame
  // ring_db_from (<= 0) on are such rows, the ones before it are noise-relative (learning frames' -100, rows a call with planes wrote);
  // 0: none. The host settles the window (subtracts the ceiling in place) before anything else writes to it or the ceiling changes.
  int ring_db_from;
  int n, nframes, n_learn, pushed_before;
  int shift;  // (frames since reset, before this batch) mod TF: tile t covers batch frames [t*TF - shift, t*TF - shift + TF)
  float start_level;
  const uint8_t* pass;
  uint32_t* maskbits;
  int* counts;
  float* rel_out;
  float* avg_out;
  float* avg_sparse;
  // Spectrogram side branch (k_detect_fused<..., SPEC = true> only; spectrogram.cpp:45-60)
  float* spec_partial;             // [frame tile][spec_n]: the tile's frames, bin-decimated and summed in frame order
  const float* spec_prev_partial;  // the previous launch's partial sums, not yet added to their container (or null)
  float* spec_prev_sum;            // [spec_n] Container::m_sum they belong to
  int spec_prev_tiles;
  int spec_m, spec_n;              // m_decimatorFactor (a power of two <= 256), m_outputSize
  // Tile culling (tile_is_culled, 8192 points): per-column maxima of this batch's PSD rows (Fft8192Args::segsum), or null
  const float* segsum;             // [32][seg_pitch]
  int seg_pitch;
  // ... and of the halo_rows frames before the batch (deep pipelining: the frames the launch transformed once more into halo_psd left
  // their maxima too, [32][kHaloSegPitch], frame -halo_rows + i at [c][i]); null: tiles that reach back before the batch are not tested
  const float* halo_segsum;
  const float* thr_tilemin;        // [32] min of thr over bins [256 c - 32, 256 c + 288)
  // [s], s < 8: nonzero once list s has been written through; [16 + kLiveCap s ...] the tiles of plan workgroup s that must be
  // evaluated; [kLiveCounts + kLiveCopyStride k + s], k < kLiveCopies: kLiveReady | their number, published as soon as it is
  // known (most consumers learn from it that there is nothing for them), in copies a page apart.
  // Written by the plan role (plan_tiles), consumed by the workgroups of the same launch (list_pair), the header set back to
  // zero by the call's emit stage.
  int* live;
  // Tile culling, long transforms (N = 256 x N2; plan_long.h: k_plan_long): [0] = how many tiles must be evaluated, [1 ...] = their
  // numbers, written by a launch of its own between the call's FFT and detect stages; null = every tile. hist_by_fft: no tile
  // writes ring rows — the FFT stage has written those of this batch itself (long transforms: fft256_kernels.h, RowsExtra), or
  // nobody needs them before the pipeline is drained, which then writes them from the call's PSD plane (8192 points, deep
  // pipelining: k_ring_fill, specscan.hip).
  const int* tile_list;
  int hist_by_fft;
  // What the library did (ss_get_stats): [0] tiles that went through a culling test, [1] tiles the test proved empty,
  // [2] workgroups that stopped waiting for a launch's plan and made it themselves (kStat*). Null: not counted.
  unsigned long long* stats;
#ifdef SS_DIAG
  long long* stamp_mid;  // measurement builds, four per tile: wall clock at the tile's start, after the first pass of phase 1 (thread 0's 36 rows have landed), after phase 1 and after phase 2
  unsigned* cull_stats;  // measurement builds: {tiles, tiles on the culling path, tiles culled}
#endif
};

// plane[row][byte offset coff]: block-uniform row base (scalar registers) + one 32-bit per-thread offset
__device__ __forceinline__ void store_row(float* plane, int row, int n, uint32_t coff, float v) {
  *reinterpret_cast<float*>(reinterpret_cast<char*>(plane + (size_t)row * n) + coff) = v;
}

// time means of one column's tile, written into the LDS tile: direct sum for the tile's first frame, then the
// Averager's own update. frames_seen = Averager::m_frames after the tile's first frame (warm-up: -100 until G).
template <int G, int TF, int P, bool WARMUP>
__device__ __forceinline__ void time_means_to_tile(const float (&x)[G - 1 + TF], float* __restrict__ tile_col, int frames_seen) {
  float sum = 0.0f;
#pragma unroll
  for (int g = 0; g < G; ++g) sum += x[g];  // oldest first
#pragma unroll
  for (int j = 0; j < TF; ++j) {
    if (j > 0) {
      sum -= x[j - 1];      // Averager::subtract(front)
      sum += x[j + G - 1];  // Averager::add(new row)
    }
    const float m = div_const<G>(sum);  // m_sum[i] / m_groupSize
    tile_col[j * P] = (!WARMUP || frames_seen + j >= G) ? m : kNoData;  // Averager::updateAverage: m_groupSize <= m_frames
  }
}

// Spectrogram side branch inside the detect kernel (spectrogram.cpp:45-60). Every tile reduces its own frames:
//   spectrogram_tile_means   all 256 threads: wave w takes the tile's frames 4w..4w+3, lane l the bins 4l..4l+3 of the
//                            tile (one 16-byte load per frame; the rows were just read by phase 1 and come from L2).
//                            Per frame the mean of m adjacent raw-PSD bins, summed in ascending bin order as the
//                            reference does (for m > 4 the lanes to the right hand their four values over one by one),
//                            then / m. The means go to LDS (the avgY tile is free by then).
//   spectrogram_tile_sum     thread = output bin: the tile's frames added in frame order -> spec_partial[tile][bin]
// The partial sums of a batch are added to the container (in frame-tile order, whatever ran when) by the NEXT launch —
// spectrogram_fold, by the first-dispatched tile of each bin column — or by k_spec_combine when the host needs the
// container before that (ss_spectrogram_read, retune): kernel boundaries order the writes, no fences or counters.
template <int TF, int TB>
__device__ __forceinline__ void spectrogram_tile_means(const DetectArgs& a, float* __restrict__ means, int tid, int f0, int b0) {
  static_assert(TF == 16 && TB == 256, "four waves x four frames, 64 lanes x four bins");
  const int m = a.spec_m, n = a.n;
  const int per_tile = TB / m > 0 ? TB / m : 1;
  const int lane = tid & 63, w = tid >> 6;
  const int bin = b0 + 4 * lane;
  const bool inside = bin < n;
  float4 v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int fr = min(max(f0 + 4 * w + i, 0), a.nframes - 1);  // always a legal row; frames outside the batch are skipped by the sum
    v[i] = *reinterpret_cast<const float4*>(a.psd + (size_t)fr * n + (inside ? bin : 0));
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float* row = means + (4 * w + i) * per_tile;
    if (m == 1) {
      if (inside) *reinterpret_cast<float4*>(row + 4 * lane) = v[i];
    } else if (m == 2) {
      if (inside) *reinterpret_cast<float2*>(row + 2 * lane) = make_float2((v[i].x + v[i].y) / 2.0f, (v[i].z + v[i].w) / 2.0f);
    } else {
      float sum = ((v[i].x + v[i].y) + v[i].z) + v[i].w;
      const int lanes_per_bin = m >> 2;
      for (int d = 1; d < lanes_per_bin; ++d) {  // wave-uniform trip count
        sum += __shfl_down(v[i].x, d);
        sum += __shfl_down(v[i].y, d);
        sum += __shfl_down(v[i].z, d);
        sum += __shfl_down(v[i].w, d);
      }
      if (inside && (lane & (lanes_per_bin - 1)) == 0) row[lane / lanes_per_bin] = sum / (float)m;
    }
  }
}

template <int TF, int TB>
__device__ __forceinline__ void spectrogram_tile_sum(const DetectArgs& a, const float* __restrict__ means, int tid, int ft, int f0, int b0) {
  const int m = a.spec_m;
  const int per_tile = TB / m > 0 ? TB / m : 1;
  const int ob = b0 / m + tid;
  if (tid >= per_tile || ob >= a.spec_n) return;
  const int j_lo = max(0, -f0), j_hi = min(TF, a.nframes - f0);  // the tile's frames that belong to this batch
  float acc = 0.0f;
#pragma unroll
  for (int j = 0; j < TF; ++j)
    if (j >= j_lo && j < j_hi) acc += means[j * per_tile + tid];
  a.spec_partial[(size_t)ft * a.spec_n + ob] = acc;
}

template <int TB>
__device__ __forceinline__ void spectrogram_fold(const DetectArgs& a, int tid, int b0) {
  const int m = a.spec_m;
  const int per_tile = TB / m > 0 ? TB / m : 1;
  const int ob = b0 / m + tid;
  if (tid >= per_tile || ob >= a.spec_n) return;
  float acc = a.spec_prev_sum[ob];
  for (int t0 = 0; t0 < a.spec_prev_tiles; t0 += 16) {
    float r[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) r[i] = a.spec_prev_partial[(size_t)min(t0 + i, a.spec_prev_tiles - 1) * a.spec_n + ob];
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (t0 + i < a.spec_prev_tiles) acc += r[i];
  }
  a.spec_prev_sum[ob] = acc;
}

constexpr int kLiveLists = 8;        // the most plan workgroups (lists) a stage may have
constexpr int kLiveCopies = 16;      // copies of the count words, kLiveCopyStride ints apart, behind the lists
constexpr int kLiveCopyStride = 1024;
constexpr int kLiveCounts = 8192;    // where the first copy starts
constexpr int kLiveInts = kLiveCounts + kLiveCopies * kLiveCopyStride;  // ints of a DetectArgs::live buffer
constexpr int kLiveHeader = 16;      // header words in front of DetectArgs::live's lists: the list-written flags
constexpr int kLiveCap = 640;        // capacity of a plan workgroup's list: its tile columns x the batch's frame tiles
constexpr int kLiveReady = 1 << 30;  // header word: the list is complete
constexpr int kPlanLdsFloats = 9600; // staging area of a plan workgroup (+ 64 ints of bookkeeping behind it)

// Frame tiles of a batch, and how many tile columns one plan workgroup can take (0: the stage cannot be planned).
__host__ __device__ inline int plan_frame_tiles(int nframes, int shift) { return (nframes + shift + 15) / 16; }
// a column's maxima in a plan wave's LDS: frame f of the batch (f >= -kPlanBefore: the frames before it whose maxima the halo frames
// left) at word F + F / 16, F = f + kPlanBefore (one pad word per frame tile)
constexpr int kHaloSegPitch = 64;
constexpr int kPlanBefore = 48;  // >= kHistRows = 35, a multiple of 16
__host__ __device__ inline int plan_col_floats(int nframes) { return nframes + kPlanBefore + ((nframes + kPlanBefore) >> 4) + 1; }
__host__ __device__ inline int plan_cols_per_wg(int nframes, int shift) {
  const int per_col = plan_col_floats(nframes), nft = plan_frame_tiles(nframes, shift);
  for (int cols = 8; cols >= 4; cols >>= 1)
    if (cols * per_col <= kPlanLdsFloats && cols * nft <= kLiveCap && nft <= 192) return cols;
  return 0;
}

// The plan role (8192-point frames: 32 tile columns). Workgroup `seg` takes `cols` tile columns, wave w the column
// seg * cols + w, lane = frame tile (three rounds at most). Tiles on detect_tile's straight-line path whose sole products are
// mask bits and counts are tested — no learning / warm-up / ring rows, no rel or avg plane wanted, not one of the tiles
// that refresh the ring; all others are evaluated. The wave first copies its column of Fft8192Args::segsum (one float per
// frame) into LDS with coalesced loads — a lane reading its own 36 frames straight from memory touches 36 cache lines
// nobody shares with it: measured, a plan workgroup took 24 us that way and every consumer waited for it — then every lane
// takes the maximum over its 36 frames from there (one pad word per 16 frames: lanes are 16 frames apart). Evaluated
// tiles go to the workgroup's list in (column, frame tile) order, then the header word. A culled tile writes NOTHING: its
// mask words are zero already — the emit stage of the buffer's previous user cleared every word it found set
// (EmitArgs::clear_masks) — where clearing them here, a megabyte of 32-byte writes per call, cost 1.4 us per step.
// `lds` = kPlanLdsFloats floats + 64 ints.
// `first` = false: the call is a consumer's fallback (the plan role's own workgroup has not been heard of): everything is
// written as the plan role writes it, nothing is counted twice.
template <int G, int GX, int TF, int TB_ = 256>
__device__ __forceinline__ void plan_tiles(const DetectArgs& a, int seg, int cols, int tid, float* __restrict__ lds, bool first) {
  using T = DetectTile<G, GX, TF, TB_>;
  constexpr int TB = T::TB, H = T::H;
  static_assert(TF == 16, "one pad word per frame tile");
  const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = a.n, nframes = a.nframes;
  const int tiles_per_row = n / TB;
  const int nft = plan_frame_tiles(nframes, a.shift);
  const int rounds = (nft + 63) >> 6;
  int* book = reinterpret_cast<int*>(lds + kPlanLdsFloats);  // [w * 4 + round]: tiles wave w lists in that round
  const int col = seg * cols + w;
  const bool has_col = w < cols && col < tiles_per_row;
  const bool plannable = a.segsum && !a.rel_out && !a.avg_out;
  float* mine = lds + w * plan_col_floats(nframes);
  const auto at = [](int f) { return f + kPlanBefore + ((f + kPlanBefore) >> 4); };  // frame f's word in `mine`
  // frames before the batch whose maxima are known (the halo frames' — until session 36 of round 5 they left none, and the 64 tiles of
  // a batch's first two frame tiles were evaluated whatever they held: the last workgroups of every launch, profiles/r05/s32_*)
  const int before = a.halo_segsum && a.halo_psd ? min(a.halo_rows, kPlanBefore) : 0;
  float tm = 0.0f;
  if (has_col && plannable) {
    const float* src = a.segsum + (size_t)col * a.seg_pitch;
    tm = a.thr_tilemin[col];
    // (eight loads in flight per trip: one after the other — load, wait, store, sixteen times for a 1024-frame batch — the copy alone
    // took the plan workgroups 8-13 us, and the launch's frame workgroups are through after 12: they wait for this list)
    // (round 6 tried sixteen at a time — ONE round trip for a 1024-frame batch: 23.2 against 22.8-23.1 us per step in alternating runs,
    // profiles/r06/s4_summary.txt: no gain, the frame workgroups do not wait for the plan as a rule)
    constexpr int kPlanCopyLoads = 8;
    float hm = 0.0f;
    if (lane < before) hm = a.halo_segsum[col * kHaloSegPitch + (a.halo_rows - before) + lane];
    for (int fb = 0; fb < nframes; fb += 64 * kPlanCopyLoads) {
      float v[kPlanCopyLoads];
#pragma unroll
      for (int u = 0; u < kPlanCopyLoads; ++u) v[u] = src[min(fb + 64 * u + lane, nframes - 1)];
#pragma unroll
      for (int u = 0; u < kPlanCopyLoads; ++u) {
        const int f = fb + 64 * u + lane;
        if (f < nframes) mine[at(f)] = v[u];
      }
    }
    if (lane < before) mine[at(lane - before)] = hm;
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's column is in LDS (nobody else reads it)
  unsigned long long live_mask[3] = {0ull, 0ull, 0ull}, dead_mask[3] = {0ull, 0ull, 0ull};
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    if (r < rounds) {
      const int ft_seq = r * 64 + lane;
      const bool exists = has_col && ft_seq < nft;
      const int ft = (ft_seq + nft - 1) % nft;
      const int f0 = ft * TF - a.shift;
      // (its 36 frames' maxima are all there — the batch's, and before it the halo frames' —, none of them a learning frame, no ragged end)
      const bool steady = (a.n_learn == 0 ? f0 - (G - 1) >= -before : f0 - (G - 1) >= a.n_learn) && (f0 + TF <= nframes);
      const bool writes_hist = !a.hist_by_fft && f0 + TF > nframes - H;
      bool culled = false;
      if (exists && plannable && steady && !writes_hist) {
        // the 21 x 21 mean that ends at frame f is at most mean(M_{f-20} .. M_f) - tm, M_g = the column's maximum in frame g
        // (round 3; until then max(M) - tm over all 36 frames, which noise alone brings within 1.5 dB of an 8 dB threshold).
        // The sum slides over the tile's 16 frames; a sum that is not a number (a frame of NaNs, -inf leaving the window)
        // decides nothing: evaluated.
        const int b = f0 - (G - 1);
        float sum = 0.0f;
#pragma unroll
        for (int k = 0; k < G; ++k) sum += mine[at(b + k)];
        float best = sum;
        bool unsure = sum != sum;
#pragma unroll
        for (int j = 1; j < TF; ++j) {
          sum -= mine[at(b + j - 1)];
          sum += mine[at(b + j + G - 1)];
          unsure = unsure || (sum != sum);
          best = fmaxf(best, sum);
        }
        culled = !unsure && (best * (1.0f / (float)G) - tm) < a.start_level - kCullMargin;  // (false for NaN)
      }
      live_mask[r] = __ballot(exists && !culled);
      dead_mask[r] = __ballot(culled);
      if (a.stats && first) {  // (wave-uniform)
        const int tested = __popcll(__ballot(exists && plannable && steady && !writes_hist));
        if (lane == 0 && tested) {
          atomicAdd(stat_word(a.stats, kStatTested), (unsigned long long)tested);
          atomicAdd(stat_word(a.stats, kStatCulled), (unsigned long long)__popcll(dead_mask[r]));
        }
      }
      if (lane == 0) book[w * 4 + r] = __popcll(live_mask[r]);
    } else if (lane == 0) {
      book[w * 4 + r] = 0;
    }
  }
  if (lane == 0) book[w * 4 + 3] = 0;
  __syncthreads();
  int base = 0, total = 0;
  for (int k = 0; k < 32; ++k) {  // (wave, round) in order
    const int c = book[k];
    base += k < w * 4 ? c : 0;
    total += c;
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    if (r < rounds) {
      const int ft_seq = r * 64 + lane;
      if ((live_mask[r] >> lane) & 1ull)
        __hip_atomic_store(&a.live[kLiveHeader + seg * kLiveCap + base + __popcll(live_mask[r] & ((1ull << lane) - 1ull))], ft_seq * tiles_per_row + col,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // write-through
      base += __popcll(live_mask[r]);
    }
  }
  // the count at once, in kLiveCopies copies a page apart: a thousand consumers asking one address are a thousand requests to
  // one memory channel (measured: 2 us per step) ...
  if (tid < kLiveCopies) __hip_atomic_store(&a.live[kLiveCounts + tid * kLiveCopyStride + seg], kLiveReady | total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // ... this wave's entries are in memory ...
  __syncthreads();
  if (tid == 0) __hip_atomic_store(&a.live[seg], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ... every wave's: the list may be read
#ifdef SS_DIAG
  if (a.cull_stats > reinterpret_cast<unsigned*>(1) && lane == 0 && has_col) {
    int lv = 0, dd = 0;
    for (int r = 0; r < 3; ++r) {
      lv += __popcll(live_mask[r]);
      dd += __popcll(dead_mask[r]);
    }
    atomicAdd(&a.cull_stats[0], (unsigned)(lv + dd));
    atomicAdd(&a.cull_stats[2], (unsigned)dd);
  }
#endif
}

// Consumer side (scan_step.h), called by every wave of a workgroup with the same arguments. Consumer `p` of `nseg` lists serves
// list p mod nseg, entries 2 (p div nseg) and the next one. All it has to read first is ONE header word, kLiveReady | count:
//   live_wait_count  `word` = the header word as read earlier (the FFT role asks before its pass 3, so the answer usually costs it
//                    nothing); if the list's count was not known by then, poll for it — at most `limit` times. Returns the word
//                    as last seen (kLiveReady missing: gave up);
//   live_wait_list   polls the list-written flag the same way (only consumers that have entries to fetch ask);
//   live_pair        the two tiles (-1: none), once count and entries are known to be there.
// A consumer that gives up makes the plan itself (see the top of this file): nothing waits without bound.
__host__ __device__ __forceinline__ int live_count_word(int p, int nseg) { return kLiveCounts + ((p / nseg) % kLiveCopies) * kLiveCopyStride + p % nseg; }
__device__ __forceinline__ int live_wait_count(const DetectArgs& a, int p, int nseg, int word, int limit) {
  word = __builtin_amdgcn_readfirstlane(word);
  for (int i = 0; i < limit && !(word & kLiveReady); ++i) {
    __builtin_amdgcn_s_sleep(8);
    word = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&a.live[live_count_word(p, nseg)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  }
  return word;
}
__device__ __forceinline__ bool live_wait_list(const DetectArgs& a, int seg, int limit) {
  int flag = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&a.live[seg], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  for (int i = 0; i < limit && !flag; ++i) {
    __builtin_amdgcn_s_sleep(8);
    flag = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&a.live[seg], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  }
  return flag != 0;
}
__device__ __forceinline__ int2 live_pair(const DetectArgs& a, int p, int nseg, int count) {
  const int seg = p % nseg, q = p / nseg;
  int2 t = make_int2(-1, -1);
  if (2 * q < count) {
    const unsigned long long v = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(a.live + kLiveHeader + seg * kLiveCap + 2 * q), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    t.x = __builtin_amdgcn_readfirstlane((int)(unsigned)v);
    if (2 * q + 1 < count) t.y = __builtin_amdgcn_readfirstlane((int)(v >> 32));
    const int n_tiles = (a.n / 256) * plan_frame_tiles(a.nframes, a.shift);
    if ((unsigned)t.x >= (unsigned)n_tiles) t.x = t.y = -1;  // (never: a tile number that is none must not become an address)
    if ((unsigned)t.y >= (unsigned)n_tiles) t.y = -1;
  }
  return t;
}

// min of the noise ceiling over bins [256 c - 32, 256 c + 288), c = blockIdx.x (one wave each): DetectArgs::thr_tilemin,
// refreshed whenever the ceiling changes (learning batches).
__global__ __launch_bounds__(64) void k_thr_tilemin(const float* __restrict__ thr, int n, float* __restrict__ tilemin) {
  const int c = blockIdx.x, lane = threadIdx.x;
  float m = __builtin_inff();
  for (int i = lane; i < 320; i += 64) {
    const int bin = 256 * c - 32 + i;
    if (bin >= 0 && bin < n) m = fminf(m, thr[bin]);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) m = fminf(m, __shfl_xor(m, d));
  if (lane == 0) tilemin[c] = m;
}

// The general path's per-row work, written for the instruction count: a tile that takes this path is evaluated by a workgroup whose
// end the launch waits for, its waves share their SIMDs with six or seven others, and an instruction of theirs is issued every ~5 ns.
// Both parts are block-uniform decisions on the row's frame number fr:
//   the address   fr < 0 at `before_end` + fr rows (clamped to the rows there are), fr >= 0 at psd + min(fr, nframes - 1) rows
//   the value     fr < 0: x - (ceiling or 0.0f);  learning frame: kNoData;  frame of the batch: x - ceiling;  past its end: 0.0f
//                 — as masks on the operands (x - 0.0f is x bit for bit), no branch
// and both are worked out for the 36 rows at once: lane l of a wave works out row l's address and masks with a dozen VECTOR
// instructions, the wave then picks them up row by row with v_readlane (uniform again: the loads keep their scalar base) — three
// instructions per row for the address and load, six for the value.
// (Tried, round 5: row by row on the scalar unit — 21 + 12 instructions per row, each behind the one before; with the expressions as
// they were until session 33, 20 + ~30 with branches, and the two passes cost such a tile 8.4 us each against 1.8 us for a steady
// tile's: profiles/r05/s32_*.)
__device__ __forceinline__ const char* general_row_address(const char* psd, const char* before_end, int before_rows, int nframes, ptrdiff_t row_bytes, int fr) {
  const int idx = min(max(fr, -before_rows), nframes - 1);
  return (fr < 0 ? before_end : psd) + (ptrdiff_t)idx * row_bytes;  // (tried: a 32 x 32 -> 64-bit product by hand — the compiler expands __mulhi on scalars into the same six instructions)
}
struct GeneralRowsOfLane {
  unsigned lo, hi, tm, km, other;
};
__device__ __forceinline__ GeneralRowsOfLane general_rows_of_lane(const char* psd, const char* before_end, int before_rows, int nframes, ptrdiff_t row_bytes, int fr0, int lane,
                                                                   int n_learn, int ring_db_from, bool before_are_psd) {
  const int fr = fr0 + lane;  // (lanes beyond the 36th: a clamped, legal address nobody asks for)
  const unsigned long long at = (unsigned long long)(uintptr_t)general_row_address(psd, before_end, before_rows, nframes, row_bytes, fr);
  GeneralRowsOfLane g;
  g.lo = (unsigned)at;
  g.hi = (unsigned)(at >> 32);
  const bool kept = fr < 0 || (fr < nframes && fr >= n_learn);
  const bool with_t = fr >= 0 || fr >= ring_db_from || before_are_psd;
  g.other = fr < nframes ? __float_as_uint(kNoData) : 0u;
  g.tm = with_t ? 0xffffffffu : 0u;
  g.km = kept ? 0xffffffffu : 0u;
  return g;
}
typedef const __attribute__((address_space(1))) char* global_bytes;  // (global memory, said so: the loads keep a scalar base and a 32-bit lane offset)
template <int R>
__device__ __forceinline__ global_bytes general_row_address_at(const GeneralRowsOfLane& g) {
  // (v_readlane's result is an int: through unsigned, or the low word's sign bit floods the high one)
  const unsigned long long at = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(g.hi, R) << 32) | (unsigned long long)(unsigned)__builtin_amdgcn_readlane(g.lo, R);
  return (global_bytes)at;
}
template <int R>
__device__ __forceinline__ float general_row_value_at(const GeneralRowsOfLane& g, float x, float t) {
  const unsigned tm = __builtin_amdgcn_readlane(g.tm, R), km = __builtin_amdgcn_readlane(g.km, R), other = __builtin_amdgcn_readlane(g.other, R);
  const float v = x - __uint_as_float(__float_as_uint(t) & tm);
  return __uint_as_float((__float_as_uint(v) & km) | (other & ~km));
}
// x[r] = the row's value at byte offset `coff`, r = 0 .. ROWS - 1 (compile-time recursion: v_readlane takes its lane as an immediate)
template <int R, int ROWS>
__device__ __forceinline__ void general_rows_load(const GeneralRowsOfLane& g, uint32_t coff, float (&x)[ROWS]) {
  if constexpr (R < ROWS) {
    x[R] = *(const __attribute__((address_space(1))) float*)(general_row_address_at<R>(g) + coff);
    general_rows_load<R + 1, ROWS>(g, coff, x);
  }
}
template <int R, int ROWS>
__device__ __forceinline__ void general_rows_load2(const GeneralRowsOfLane& g, uint32_t coff0, uint32_t coff1, float (&x)[ROWS], float (&y)[ROWS]) {
  if constexpr (R < ROWS) {
    const global_bytes src = general_row_address_at<R>(g);
    x[R] = *(const __attribute__((address_space(1))) float*)(src + coff0);
    y[R] = *(const __attribute__((address_space(1))) float*)(src + coff1);
    general_rows_load2<R + 1, ROWS>(g, coff0, coff1, x, y);
  }
}
template <int R, int ROWS>
__device__ __forceinline__ void general_rows_settle(const GeneralRowsOfLane& g, float t, float (&x)[ROWS]) {
  if constexpr (R < ROWS) {
    x[R] = general_row_value_at<R>(g, x[R], t);
    general_rows_settle<R + 1, ROWS>(g, t, x);
  }
}

// Which of the tile's 276 columns (256 + 10 either side, in bin order) a thread takes in phase 1. Rows in bin order: thread = column
// (256, then 20 more). The fold's rows (PERM8 = log2 Q, fft65536_dif8.h): a tile's own 256 bins are one block of the row (Q = 8) or
// half of one (Q = 16) with the residues' runs side by side, consecutive BINS 128 bytes apart — so the first 256 threads take the
// tile's own columns in the block's order, thread g * (256 / Q) + j the bin Q j + g: a wave's load is 256 contiguous bytes (four
// runs of 64) instead of sixteen lanes on eight lines — and the 20 columns either side go to the second pass. The tile in LDS stays
// in bin order.
template <int PERM8, int A, int TB>
__device__ __forceinline__ int tile_column_of(int pass_c, int tid) {
  if constexpr (PERM8 == 0) {
    return pass_c * TB + tid;
  } else {
    constexpr int RUN = TB >> PERM8;  // bins of a residue in the tile
    if (pass_c == 0) return A + ((tid & (RUN - 1)) << PERM8) + tid / RUN;
    return tid < A ? tid : TB + tid;  // (tid < 2 A)
  }
}

// One tile of the fused back end. `block` = tile number (what blockIdx.x is for the stand-alone kernel), `tid` = 0..TB-1,
// `tile` / `cnt` = this tile's LDS (TF * P floats, TF ints). `valid` = false: the caller has no tile for these threads (odd
// tile count in a two-tile workgroup) — they only keep the workgroup's barriers company. Every __syncthreads() below is
// reached by all threads of the workgroup whatever `valid`, `steady` or `interior` are.
// PERM8 (0, or log2 of the fold's radix: 3, 4): the rows the tile reads (a.psd, the ring) and writes (the ring) are the radix-Q fold's rows
// of 8192 Q bins in BLOCKS of 32 Q bins — bin Q k' + g at (k' / 32) * 32 Q + 32 g + k' % 32 (fft65536_dif8.h: dif_bin_offset; dB values
// from ring_db_from on) —; calls that hand out no plane only (no rel_out). A tile's thread g * 32 + j takes the bin 8 j + g: a wave's 36
// row loads are 256 contiguous bytes (Q = 8) or four runs of 64 (Q = 16); everything else — the noise ceiling, the pass mask, mask bits,
// sparse averages — stays in bin order.
// ONE_FLIGHT (the fold's rows only; true wherever the scan runs the tile): a thread's two columns in one flight of loads, 124 VGPRs.
// false: the two passes of the paths for rows in bin order, on the fold's addresses — the same arithmetic on the same values in 62 VGPRs,
// for a launch of tiles alone that nothing waits for (track_digest_sparse.h: k_digest_tiles).
template <int G, int GX, int TF, int TB_ = 256, bool SPEC = false, int PERM8 = 0, bool ONE_FLIGHT = true>
__device__ __forceinline__ void detect_tile(const DetectArgs& a, int block, int tid, float* __restrict__ tile, int* __restrict__ cnt, bool valid) {
  using T = DetectTile<G, GX, TF, TB_>;
  constexpr int A = T::A, TB = T::TB, P = T::P, ROWS = T::ROWS, H = T::H, SEGW = T::SEGW, NSEG = T::NSEG, YW = T::YW;
  const int n = a.n, nframes = a.nframes;
  const int tiles_per_row = (n + TB - 1) / TB;
  // Frame tiles are dispatched rotated by one: the ragged last tile and the tiles that read ring rows take the
  // slower general path, so they go first and the straight-line tiles fill in behind them instead of leaving a tail.
  const int nft = (nframes + a.shift + TF - 1) / TF;
  // (Tried for long rows and dropped: an XCD-aware column-major order — each XCD walking the frame tiles of one column
  // group after the other so that a tile finds its predecessor's halo rows in that XCD's L2. 65536 points x 128 frames:
  // the kernel went from 19.6 to 26.7 us.)
  const int ft_seq = block / tiles_per_row, bt = block % tiles_per_row;
  const int ft = (ft_seq + nft - 1) % nft;
  const int f0 = ft * TF - a.shift;  // batch-relative frame of the tile's first row of outputs; may be negative
  const int b0 = bt * TB;
  if (tid < TF) cnt[tid] = 0;
#ifdef SS_DIAG
  if (a.stamp_mid && valid && tid == 0) a.stamp_mid[4 * (size_t)block] = wall_clock64();
#endif
  if constexpr (SPEC) {
    if (valid && a.spec_prev_partial && ft_seq == 0) spectrogram_fold<TB>(a, tid, b0);  // the first-dispatched tile of each bin column
  }
  // block-uniform classification
  const bool interior = (b0 - A >= 0) && (b0 + TB + A <= n);
  const bool steady = (f0 - (G - 1) >= a.n_learn) && (f0 - (G - 1) >= 0) && (f0 + TF <= nframes);
  const int first_hist = a.hist_by_fft ? (1 << 30) : nframes - H;  // batch frames >= first_hist become the ring rows [frame - first_hist]
  const float* before_base = a.halo_psd ? a.halo_psd : a.hist_in;  // rows before the batch: the previous call's last frames, or the ring
  const int before_rows = a.halo_psd ? a.halo_rows : H;
  const bool writes_hist = f0 + TF > first_hist;

  // ---------------- phase 1: time means, thread = column ----------------
  if constexpr (PERM8 != 0 && ONE_FLIGHT) {
    // The fold's rows (KIND 8 / 9 of k_scan_step: 128 registers per thread). A pair of tiles holds a workgroup slot that a residue's
    // transform is waiting for, or ends the launch: what counts is how long ONE wave takes, and a wave issues an instruction every
    // four or five cycles — 1000 instructions are 2 us. Measured per tile, alone on the chip (profiles/r05/s29_*): first pass
    // 1.7 us, the second pass — twenty columns, the same 36 loads and the same latency over again — 1.5, and for the tiles that read
    // rows from before the batch 5-8 + 4-7 us: twenty scalar instructions per row and pass to pick the row's address. So here
    //   * a thread of the first twenty takes its second column's 36 rows in the same flight as its first;
    //   * rows that lie one after the other in memory — a steady tile's, and with the batch's rows right behind the ring's window
    //     (ring_place.h) every tile's but a ragged last one — are addressed as the steady path addresses them.
    // The arithmetic per value is the other paths' own.
    if (valid) {
      const bool two = tid < 2 * A;
      const int c0 = tile_column_of<PERM8, A, TB>(0, tid), c1 = tile_column_of<PERM8, A, TB>(1, tid);
      const int col0 = b0 - A + c0;  // one of the tile's own 256 columns: inside the band
      const int col1 = b0 - A + c1, col1c = min(max(col1, 0), n - 1);
      const bool in1 = col1 == col1c;
      const uint32_t off0 = (uint32_t)dif_bin_offset(col0, PERM8) * 4u, off1 = (uint32_t)dif_bin_offset(two ? col1c : col0, PERM8) * 4u;
      const float t0 = a.thr[col0], t1 = a.thr[two ? col1c : col0];
      const bool in_line = steady || (!a.halo_psd && a.psd == a.hist_in + (size_t)H * n && f0 + TF <= nframes);  // (f0 - 20 >= -H: shift < TF)
      float x[ROWS], y[ROWS];
      // (a non-steady tile's 36 rows on 36 lanes, general_rows_of_lane: every lane of the wave is active here, and the lanes stay together
      // wherever the result is read lane by lane — the second column is the whole first wave's business up to its stores, see the general
      // path below)
      const bool wave0 = tid < 64;
      GeneralRowsOfLane rows_l{};
      if (!steady) {
        rows_l = general_rows_of_lane(reinterpret_cast<const char*>(a.psd), reinterpret_cast<const char*>(before_base) + (ptrdiff_t)before_rows * (ptrdiff_t)n * 4, before_rows, nframes,
                                      (ptrdiff_t)n * 4, f0 - (G - 1), tid & 63, a.n_learn, a.ring_db_from, a.halo_psd != nullptr);
        asm volatile("" : "+v"(rows_l.lo), "+v"(rows_l.hi), "+v"(rows_l.tm), "+v"(rows_l.km), "+v"(rows_l.other));
      }
      if (in_line) {
        const char* p = reinterpret_cast<const char*>(a.psd) + (ptrdiff_t)(f0 - (G - 1)) * (ptrdiff_t)n * 4;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) x[r] = load_row_value(p + (size_t)r * n * 4 + off0);
        if (wave0) {
#pragma unroll
          for (int r = 0; r < ROWS; ++r) y[r] = load_row_value(p + (size_t)r * n * 4 + off1);
        }
      } else {
        general_rows_load2<0, ROWS>(rows_l, off0, off1, x, y);  // (the second column by every thread: a branch per row would cost more than the loads)
      }
      // rel = value - ceiling; learning frames, rows of the ring, frames past a ragged end as the general path below has them
      const auto settle = [&](float (&v)[ROWS], float t) {
        if (steady) {
#pragma unroll
          for (int r = 0; r < ROWS; ++r) v[r] -= t;
        } else {
          general_rows_settle<0, ROWS>(rows_l, t, v);
        }
      };
      settle(x, t0);
      if (wave0) settle(y, t1);
#pragma unroll
      for (int j = 0; j < TF; ++j) {
        const int fr = f0 + j;
        if (fr >= 0 && fr < nframes) {
          if (a.rel_out) store_row(a.rel_out, fr, n, off0, x[G - 1 + j]);
          if (fr >= first_hist) store_row(a.hist_out, fr - first_hist, n, off0, x[G - 1 + j]);
        }
      }
      if (steady) time_means_to_tile<G, TF, P, false>(x, &tile[c0], 0);
      else time_means_to_tile<G, TF, P, true>(x, &tile[c0], a.pushed_before + f0 + 1);
      if (two) {
        if (!in1) {
#pragma unroll
          for (int j = 0; j < TF; ++j) tile[j * P + c1] = 0.0f;  // outside the band: contributes exactly nothing to the clipped window sums
        } else if (steady) {
          time_means_to_tile<G, TF, P, false>(y, &tile[c1], 0);
        } else {
          time_means_to_tile<G, TF, P, true>(y, &tile[c1], a.pushed_before + f0 + 1);
        }
      }
    }
  } else if (!valid) {
    // nothing
  } else if (steady) {
    // straight line: ROWS independent, unconditional loads per column; 276 columns over 256 threads.
    // Columns outside the band (first / last tile of a row) read a clamped address and contribute 0.0f.
#pragma unroll
    for (int pass_c = 0; pass_c < 2; ++pass_c) {
#ifdef SS_DIAG
      if (pass_c == 1 && a.stamp_mid && tid == 0) a.stamp_mid[4 * (size_t)block + 1] = wall_clock64();
#endif
      const int c = tile_column_of<PERM8, A, TB>(pass_c, tid);
      if (pass_c == 0 || tid < 2 * A) {
        const int col = b0 - A + c;
        const int colc = min(max(col, 0), n - 1);
        const bool in_band = col == colc;
        const float t = a.thr[colc];
        // block-uniform row base (scalar registers) + one 32-bit per-thread byte offset
        const char* p = reinterpret_cast<const char*>(a.psd + (size_t)(f0 - (G - 1)) * n);
        const uint32_t coff = (uint32_t)(PERM8 ? dif_bin_offset(colc, PERM8) : colc) * 4u;
        float x[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) x[r] = load_row_value(p + (size_t)r * n * 4 + coff) - t;
        if (!interior) {
#pragma unroll
          for (int r = 0; r < ROWS; ++r) x[r] = in_band ? x[r] : 0.0f;
        }
        time_means_to_tile<G, TF, P, false>(x, &tile[c], 0);
        if (in_band && c >= A && c < A + TB) {
          if (a.rel_out) {
#pragma unroll
            for (int j = 0; j < TF; ++j) store_row(a.rel_out, f0 + j, n, coff, x[G - 1 + j]);
          }
          if (writes_hist) {
#pragma unroll
            for (int j = 0; j < TF; ++j)
              if (f0 + j >= first_hist) store_row(a.hist_out, f0 + j - first_hist, n, coff, x[G - 1 + j]);
          }
        }
      }
    }
  } else {
    // general path: ring rows from before the batch, learning frames, averager warm-up, ragged batch end.
    // Same arithmetic as above on the same values, so a frame's result does not depend on the path.
    // (two straight passes over the 276 columns, not a loop: a loop makes the compiler hoist all 36 row
    // pointers out of it and spill scalar registers)
    // (Tried, round 6: the tiles whose first rows are halo frames — the first two frame tiles of a deep-pipelined 8192-point batch — on a
    // straight-line path of their own: 23.2-23.6 against 23.0-23.1 us per step, no gain, profiles/r06/s16_summary.txt.)
#pragma unroll
    for (int pass_c = 0; pass_c < 2; ++pass_c) {
#ifdef SS_DIAG
      if (pass_c == 1 && a.stamp_mid && tid == 0) a.stamp_mid[4 * (size_t)block + 1] = wall_clock64();
#endif
      // The 36 rows' addresses and masks on 36 lanes (general_rows_of_lane), read back lane by lane. A lane's registers are only safe from
      // the register allocator while the lane runs the same code as its readers (a lane that has branched off "needs them no more" and may
      // find them reused there): so a wave takes part in a pass as a whole or not at all — the second pass is the tile's first wave, its
      // lanes without a column and the lanes outside the band go through the loads on a legal column of their own and part only at the
      // stores.
      if (pass_c == 0 || tid < 64) {
        GeneralRowsOfLane rows_l = general_rows_of_lane(reinterpret_cast<const char*>(a.psd), reinterpret_cast<const char*>(before_base) + (ptrdiff_t)before_rows * (ptrdiff_t)n * 4,
                                                        before_rows, nframes, (ptrdiff_t)n * 4, f0 - (G - 1), tid & 63, a.n_learn, a.ring_db_from, a.halo_psd != nullptr);
        asm volatile("" : "+v"(rows_l.lo), "+v"(rows_l.hi), "+v"(rows_l.tm), "+v"(rows_l.km), "+v"(rows_l.other));
        const bool has_column = pass_c == 0 || tid < 2 * A;  // 276 columns over 256 threads
        const int c = tile_column_of<PERM8, A, TB>(pass_c, has_column ? tid : 0);
        const int col = b0 - A + c, colc = min(max(col, 0), n - 1);
        const bool in_band = col == colc;
        const float t = a.thr[colc];
        const uint32_t coff = (uint32_t)(PERM8 ? dif_bin_offset(colc, PERM8) : colc) * 4u;
        float x[ROWS];
        // all loads first, unconditional, on always-legal addresses: independent and in flight together. Ring rows hold rel values — or dB
        // values, from ring_db_from on —, plane rows (the halo frames) are PSD
        general_rows_load<0, ROWS>(rows_l, coff, x);
        general_rows_settle<0, ROWS>(rows_l, t, x);
        if (has_column) {
          if (!in_band) {
#pragma unroll
            for (int j = 0; j < TF; ++j) tile[j * P + c] = 0.0f;  // outside the band: contributes exactly nothing to the clipped window sums
          } else {
            if (c >= A && c < A + TB) {
#pragma unroll
              for (int j = 0; j < TF; ++j) {
                const int fr = f0 + j;
                if (fr >= 0 && fr < nframes) {
                  if (a.rel_out) store_row(a.rel_out, fr, n, coff, x[G - 1 + j]);
                  if (fr >= first_hist) store_row(a.hist_out, fr - first_hist, n, coff, x[G - 1 + j]);
                }
              }
            }
            time_means_to_tile<G, TF, P, true>(x, &tile[c], a.pushed_before + f0 + 1);
          }
        }
      }
    }
  }
  __syncthreads();
#ifdef SS_DIAG
  if (a.stamp_mid && valid && tid == 0) a.stamp_mid[4 * (size_t)block + 2] = wall_clock64();
#endif

  // ---------------- phase 2: frequency means + threshold, thread = (frame, 16-bin segment) ----------------
#pragma unroll
  for (int q0 = 0; q0 < TF * NSEG; q0 += TB) {
    const int q = q0 + tid;
    const int fj = q % TF;
    const int seg = q / TF;
    const int f = f0 + fj;
    const int i0 = b0 + seg * SEGW;  // first bin of the segment
    const bool live = valid && f >= 0 && f < nframes && i0 < n;
    uint32_t bits = 0;
    if (live) {
      float outv[SEGW];
      const float* row = &tile[fj * P + seg * SEGW];  // row[k] = avgY(f, i0 - A + k)
      float y[YW];
#pragma unroll
      for (int k4 = 0; k4 < YW / 4; ++k4) {
        const float4 v4 = *reinterpret_cast<const float4*>(row + 4 * k4);
        y[4 * k4] = v4.x;
        y[4 * k4 + 1] = v4.y;
        y[4 * k4 + 2] = v4.z;
        y[4 * k4 + 3] = v4.w;
      }
      // Bins outside the band hold 0.0f in the tile, so the same straight-line sums give the reference's
      // edge-clipped window (adding or subtracting 0.0f is exact); only the divisor changes there.
      float sum = 0.0f;
#pragma unroll
      for (int k = 0; k < GX; ++k) sum += y[k];  // lowest bin first
      float sums[SEGW];
      sums[0] = sum;
#pragma unroll
      for (int o = 1; o < SEGW; ++o) {
        sum -= y[o - 1];       // utils.cpp:41  sum -= input[first]
        sum += y[o + GX - 1];  // utils.cpp:45  sum += input[last]
        sums[o] = sum;
      }
      if (interior) {
#pragma unroll
        for (int o = 0; o < SEGW; ++o) outv[o] = div_const<GX>(sums[o]);
      } else {
#pragma unroll
        for (int o = 0; o < SEGW; ++o) {
          const int i = i0 + o;
          const int count = min(n - 1, i + A) - max(0, i - A) + 1;
          outv[o] = sums[o] / (float)count;  // sum / count (float / int), utils.cpp:50
        }
      }
      const uint4 pm = *reinterpret_cast<const uint4*>(a.pass + i0);  // 16 pass bytes (n is a multiple of 64)
      const uint32_t pw[4] = {pm.x, pm.y, pm.z, pm.w};
#pragma unroll
      for (int o = 0; o < SEGW; ++o) {
        const bool ok = ((pw[o >> 2] >> (8 * (o & 3))) & 0xffu) != 0;
        bits |= (a.start_level <= outv[o] && ok) ? (1u << o) : 0u;
      }
      if (a.avg_out) {
        float4* dst = reinterpret_cast<float4*>(a.avg_out + (size_t)f * n + i0);
#pragma unroll
        for (int k4 = 0; k4 < SEGW / 4; ++k4) dst[k4] = make_float4(outv[4 * k4], outv[4 * k4 + 1], outv[4 * k4 + 2], outv[4 * k4 + 3]);
      } else if (bits) {
        float* dst = a.avg_sparse + (size_t)f * n + i0;
#pragma unroll
        for (int o = 0; o < SEGW; ++o)
          if (bits & (1u << o)) dst[o] = outv[o];
      }
    }
    // lanes q and q + TF hold the same frame, segments seg and seg + 1: together one 32-bit mask word
    const uint32_t hi_bits = __shfl_down(bits, TF);
    if ((seg & 1) == 0 && live) {
      const uint32_t word = bits | (hi_bits << 16);
      a.maskbits[((size_t)f * n + i0) >> 5] = word;
      if (word) atomicAdd(&cnt[fj], __popc(word));
    }
  }
  __syncthreads();
#ifdef SS_DIAG
  if (a.stamp_mid && valid && tid == 0) a.stamp_mid[4 * (size_t)block + 3] = wall_clock64();
#endif
  if (valid && tid < TF && cnt[tid] != 0) atomicAdd(&a.counts[f0 + tid], cnt[tid]);
  if constexpr (SPEC) {
    // (the __syncthreads above freed the avgY tile)
    if (valid) spectrogram_tile_means<TF, TB>(a, tile, tid, f0, b0);
    __syncthreads();
    if (valid) spectrogram_tile_sum<TF, TB>(a, tile, tid, ft, f0, b0);
  }
}

// Stand-alone launch: one tile per workgroup of TB threads (FFT sizes other than 8192; the 8192-point chain runs the same
// tile code as a role of k_scan_step, scan_step.h).
template <int G, int GX, int TF, int TB_ = 256, bool SPEC = false>
__global__ __launch_bounds__(TB_) __attribute__((amdgpu_waves_per_eu(8))) void k_detect_fused(DetectArgs a) {
  using T = DetectTile<G, GX, TF, TB_>;
  __shared__ __attribute__((aligned(16))) float tile[TF * T::P];
  __shared__ int cnt[TF];
  detect_tile<G, GX, TF, TB_, SPEC>(a, (int)blockIdx.x, (int)threadIdx.x, tile, cnt, true);
}

// Row copy used when the sliding ring window reaches the end of its buffer and moves back to the front
// (source and destination never overlap: the buffer holds at least three windows).
__global__ void k_hist_shift(const float* __restrict__ hist_in, float* __restrict__ hist_out, int n, int keep_rows, int nframes) {
  const size_t total = (size_t)keep_rows * n;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    hist_out[e] = hist_in[e + (size_t)nframes * n];
  }
}

// Deep pipelining (8192 points): the ring rows a call's detect tiles would have written — rel = dB - thr of its newest `rows`
// frames, the same subtraction on the same values — written when the pipeline is drained instead of by every call: between
// drains nobody reads them (a call's rows from before its batch come from the previous call's frames, transformed once more),
// and the tiles that wrote them, three frame tiles of every call, could not be culled: a third of all evaluated tiles.
struct RingFillArgs {  // up to two calls' rows in one launch (blockIdx.y)
  const float* psd_tail[2];
  const float* thr[2];
  float* hist_out[2];
};
__global__ void k_ring_fill(RingFillArgs a, int n, int rows) {
  const float* __restrict__ src = a.psd_tail[blockIdx.y];
  const float* __restrict__ thr = a.thr[blockIdx.y];
  float* __restrict__ dst = a.hist_out[blockIdx.y];
  const size_t total = (size_t)rows * n;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) dst[e] = src[e] - thr[e % n];
}

// Candidate lists (CSR) from the mask bits: one wave per frame. The frame's offset is the sum of the
// counts of the frames before it (8 counts per lane per trip of 512 frames). The wave pulls 256 mask words
// per trip (one 16-byte load per lane), ranks them with one wave scan, expands the set bits into an LDS
// list at their ranks, then streams the list out with coalesced stores — ascending bins, frames in
// order, deterministic. counts_clear (the counter buffer a later batch will accumulate into, last used by a batch of
// clear_n frames) is zeroed on the way. Everything a trip needs from global memory is requested before anything is
// waited for. The wave synchronises with nobody: its LDS list is private (LDS operations of one wave complete in
// order), so eight frames can share a workgroup (k_scan_step) without a barrier in sight.
struct EmitArgs {
  const uint32_t* maskbits;
  int words_per_row, n, nframes;
  const int* counts;
  int* counts_clear;
  int clear_n;
  const float* avg;  // avg[f * n + bin] for every hit bin (the sparse plane, or the caller's full avg plane)
  int cap;
  int* live_clear;   // DetectArgs::live of the call (or null): its header words go back to zero here
  int clear_masks;   // set every mask word found set back to zero once it has been listed: the next user of the buffer may then
                     // leave the words of tiles it does not evaluate alone (tile culling)
  int* off_int;      // [nframes + 1] the library's own copy of the offsets
  int* off_out;      // caller's cand_off or null
  int* cand_idx;     // null: offsets only
  float* cand_avg;
};

constexpr int kEmitList = 1024;  // ints of LDS per wave

__device__ __forceinline__ void wave_lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// offset of frame f = sum of counts[0..f); lane 0 records it (and the grand total behind the last frame) and zeroes this
// frame's share of the counter buffer a later batch will use. Returns the offset to every lane.
__device__ __forceinline__ int emit_frame_offset(const EmitArgs& a, int f, int lane, int mine) {
  const int nframes = a.nframes;
  int part = 0;
  for (int base = 0; base < f; base += 512) {  // 8 ints per lane per trip, all loads independent
    int v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = a.counts[min(base + k * 64 + lane, nframes - 1)];
#pragma unroll
    for (int k = 0; k < 8; ++k) part += (base + k * 64 + lane) < f ? v[k] : 0;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) part += __shfl_xor(part, d);
  const int begin = part;
  if (f == 0 && a.live_clear) {  // the call's lists are spent: list-written flags and every copy of the count words back to zero
    if (lane < kLiveLists) a.live_clear[lane] = 0;
#pragma unroll
    for (int k = 0; k < kLiveCopies * kLiveLists / 64; ++k) {
      const int e = k * 64 + lane;
      a.live_clear[kLiveCounts + (e / kLiveLists) * kLiveCopyStride + e % kLiveLists] = 0;
    }
  }
  if (lane == 0) {
    a.off_int[f] = begin;
    if (a.off_out) a.off_out[f] = begin;
    if (f == nframes - 1) {
      a.off_int[nframes] = begin + mine;
      if (a.off_out) a.off_out[nframes] = begin + mine;
    }
    for (int g = f; g < a.clear_n; g += nframes) a.counts_clear[g] = 0;
  }
  return begin;
}

// The candidates of mask words [word_lo, word_hi) of frame f, written from list position `carry` on. `w4` holds the first
// trip's words when `preloaded` (requested before the offsets were summed, so the two latencies overlap).
__device__ __forceinline__ void emit_span(const EmitArgs& a, int f, int lane, int* __restrict__ list, int word_lo, int word_hi, int carry, uint4 w4,
                                          bool preloaded) {
  constexpr int LIST = kEmitList;
  const int words_per_row = a.words_per_row, n = a.n;
  const uint32_t* row = a.maskbits + (size_t)f * words_per_row;
  const bool wide = (words_per_row & 3) == 0;
  const float* arow = a.avg + (size_t)f * n;
  const int words_per_trip = wide ? 256 : 64;
  for (int base = word_lo; base < word_hi; base += words_per_trip) {
    if (base > word_lo || !preloaded) {
      w4 = make_uint4(0u, 0u, 0u, 0u);
      if (wide) {
        if (base + 4 * lane < word_hi) w4 = *reinterpret_cast<const uint4*>(row + base + 4 * lane);
      } else if (base + lane < word_hi) {
        w4.x = row[base + lane];
      }
    }
    const uint32_t wv[4] = {w4.x, w4.y, w4.z, w4.w};
    const int c = __popc(wv[0]) + __popc(wv[1]) + __popc(wv[2]) + __popc(wv[3]);
    if (a.clear_masks && c != 0) {  // listed below; the buffer's next user finds them zero (tile culling)
      uint32_t* wrow = const_cast<uint32_t*>(row);
      if (wide) *reinterpret_cast<uint4*>(wrow + base + 4 * lane) = make_uint4(0u, 0u, 0u, 0u);
      else wrow[base + lane] = 0u;
    }
    int incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_up(incl, d);
      if (lane >= d) incl += v;
    }
    const int total = __shfl(incl, 63);
    if (total == 0) continue;  // wave-uniform
    const int first_word = wide ? base + 4 * lane : base + lane;
    // rank of the first candidate of each of this lane's four words inside the trip
    int wstart[4];
    wstart[0] = incl - c;
    wstart[1] = wstart[0] + __popc(wv[0]);
    wstart[2] = wstart[1] + __popc(wv[1]);
    wstart[3] = wstart[2] + __popc(wv[2]);
    // expand in pieces of LIST entries (a whole row of hits does not fit the list at once)
    for (int lo = 0; lo < total; lo += LIST) {
      // Hits cluster in a few words (a transmission is a run of adjacent bins), so the words are expanded
      // one per half-wave, one lane per BIT: the half-wave's 32 lanes test the 32 bits of a broadcast word
      // and write the set ones at their ranks. No per-lane serial loop over bits.
      const int half = lane >> 5, bit = lane & 31;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        unsigned long long nz = __ballot(wv[k] != 0u);
        while (nz) {  // wave-uniform
          const int l0 = __ffsll((long long)nz) - 1;
          nz &= nz - 1;
          int l1 = l0;
          if (nz) {
            l1 = __ffsll((long long)nz) - 1;
            nz &= nz - 1;
          }
          const int src = half ? l1 : l0;
          const uint32_t bits = __shfl(wv[k], src);
          const int start = __shfl(wstart[k], src);
          const int word = __shfl(first_word, src) + k;
          const bool on = ((bits >> bit) & 1u) && !(half && l1 == l0);
          const int pos = start + __popc(bits & ((1u << bit) - 1u)) - lo;
          if (on && pos >= 0 && pos < LIST) list[pos] = word * 32 + bit;
        }
      }
      wave_lds_fence();  // this wave's list writes have landed
      const int cnt = min(LIST, total - lo);
      for (int p0 = 0; p0 < cnt; p0 += 256) {
        int idx[4];
        float av[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int p = p0 + k * 64 + lane;
          idx[k] = p < cnt ? list[p] : 0;
        }
        if (a.cand_avg) {
#pragma unroll
          for (int k = 0; k < 4; ++k) av[k] = arow[idx[k]];  // four independent loads in flight
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int p = p0 + k * 64 + lane;
          const int dst = carry + lo + p;
          if (p < cnt && dst < a.cap && a.cand_idx) {
            a.cand_idx[dst] = idx[k];
            if (a.cand_avg) a.cand_avg[dst] = av[k];
          }
        }
      }
      wave_lds_fence();  // the list has been read before the next piece overwrites it
    }
    carry += total;
  }
}

__device__ __forceinline__ void cand_emit_frame(const EmitArgs& a, int f, int lane, int* __restrict__ list) {
  const int words_per_row = a.words_per_row;
  const uint32_t* row = a.maskbits + (size_t)f * words_per_row;
  // first trip's mask words (words_per_row is a multiple of 2; rows of >= 256 words are 16-byte aligned)
  uint4 w4 = make_uint4(0u, 0u, 0u, 0u);
  if ((words_per_row & 3) == 0) {
    if (4 * lane < words_per_row) w4 = *reinterpret_cast<const uint4*>(row + 4 * lane);
  } else if (lane < words_per_row) {
    w4.x = row[lane];  // N = 64: two words per row, one per lane
  }
  const int mine = a.counts[f];
  const int begin = emit_frame_offset(a, f, lane, mine);
  if (mine == 0 || (!a.cand_idx && !a.clear_masks)) return;
  emit_span(a, f, lane, list, 0, words_per_row, begin, w4, true);
}

// Long rows (n >= 16384: 512 .. 32768 mask words per frame): W waves per frame, each taking a contiguous slice of the row —
// a count pass over its slice (the words come back from L2 for the expansion), a prefix over the W slice counts in LDS,
// then the same expansion from the slice's own start. One wave per frame walks 2^20-point rows in 128 serial trips (38 us
// per 16-frame batch); eight waves take 16 each.
// `lds` = (W * kEmitList + W + 1) ints; one frame per call, 64 * W threads.
template <int W>
__device__ __forceinline__ void cand_emit_frame_wide(const EmitArgs& a, int f, int tid, int* __restrict__ lds) {
  int* slice_cnt = lds + W * kEmitList;
  int* frame_begin = slice_cnt + W;
  const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int words_per_row = a.words_per_row;
  const int per = words_per_row / W;  // a multiple of 256 (the host picks W accordingly)
  const int lo = w * per, hi = lo + per;
  const uint32_t* row = a.maskbits + (size_t)f * words_per_row;
  const int mine = a.counts[f];
  int begin = 0;
  if (w == 0) begin = emit_frame_offset(a, f, lane, mine);
  int cnt = 0;
  const bool walk = mine != 0 && (a.cand_idx || a.clear_masks);  // (offsets only: the words still have to go back to zero)
  if (walk) {
    for (int base = lo; base < hi; base += 256) {
      const uint4 q = *reinterpret_cast<const uint4*>(row + base + 4 * lane);
      cnt += __popc(q.x) + __popc(q.y) + __popc(q.z) + __popc(q.w);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d);
  }
  if (lane == 0) slice_cnt[w] = cnt;
  if (w == 0 && lane == 0) *frame_begin = begin;
  __syncthreads();
  if (!walk) return;
  int carry = *frame_begin;
  for (int k = 0; k < w; ++k) carry += slice_cnt[k];
  if (cnt == 0) return;  // wave-uniform
  emit_span(a, f, lane, lds + w * kEmitList, lo, hi, carry, make_uint4(0u, 0u, 0u, 0u), false);
}

template <int W>
__global__ __launch_bounds__(64 * W) void k_cand_emit_wide(EmitArgs a) {
  __shared__ int lds[W * kEmitList + W + 1];
  cand_emit_frame_wide<W>(a, (int)blockIdx.x, (int)threadIdx.x, lds);
}

// Stand-alone launch: one wave per workgroup (FFT sizes other than 8192).
__global__ __launch_bounds__(64) void k_cand_emit(EmitArgs a) {
  __shared__ int list[kEmitList];
  cand_emit_frame(a, (int)blockIdx.x, (int)threadIdx.x, list);
}

}  // namespace ss

// The long transforms' tile plans (PlanLongArgs, plan_long_run / plan_dif8_run / plan_x256_run, k_plan_long, k_fft_cols1024_plan) live in
// a header of their own that needs everything above; whoever includes this header gets them too, as before they moved.
#include "plan_long.h"
