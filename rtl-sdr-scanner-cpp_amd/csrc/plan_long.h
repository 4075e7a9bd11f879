// plan_long.h — tile culling for the long transforms (N = 256 x N2: 65536 points and up): which 16-frame x 256-bin tiles of a call the
// detect stage must evaluate. Three plans, one per layout of the run maxima the FFT stage leaves (PlanLongArgs::layout), as a launch of
// their own (k_plan_long), as a role of k_scan_step (scan_step.h: step_plan_routine) or at the front of a 2^20-point column launch
// (k_fft_cols1024_plan). What they share is written once: the decision on a tile's sixteen window sums (plan_long_decide), the hand-over
// of the tiles that stay to the detect stage's list and of the counts to ss_get_stats (plan_long_hand_over), and — for the two plans that
// take 32 columns x one frame tile per block — the window sums themselves (plan_cols32_finish). The 8192-point plan (detect_fused.h:
// plan_tiles) is a different protocol: lists per segment, header words, a fallback inside the launch.
// The minimum of the noise ceiling over bins [256 c - 32, 256 c + 288) that the bound subtracts is k_thr_tilemin's (detect_fused.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "detect_fused.h"  // (which includes this header at its end: either one may be included first)
#include "fft1024_kernels.h"
#include "fft256_kernels.h"

namespace ss {

// Tile culling for long transforms (N = 256 x N2: 65536 points and up, 256 and more tile columns). Same idea as plan_tiles — a
// tile that provably holds no candidate is not evaluated — from what the rows kernel of the FFT stage left per frame and 32-bin
// run (RowsExtra::smax, a ring over the frames since the last reset, so that the tile's rows from BEFORE the batch are covered
// too: a 16-frame call of 2^20-point rows has no others). The bound: with M_g the largest dB value of frame g over the tile's 256
// bins and one run on either side, and m the minimum of the noise ceiling over the same bins (thr_tilemin), every rel value of
// frame g in reach of the tile is <= M_g - m, so the 21 x 21 mean that ends at frame f is <= mean(M_{f-20} .. M_f) - m: the tile
// is dropped when that stays below start_level - kCullMargin for each of its frames (the margin covers the fp32 sums on either
// side: < 0.01 dB). A frame of zeros (M = -inf) makes the bound -inf for every window that holds it — those produce no candidate
// either — and a NaN anywhere makes the tile "cannot tell": evaluated. A tile is only tested when all its rows are frames since
// `clean_rel` (batch-relative, <= 0): no learning frame among them, one noise ceiling for all of them, the averager past its
// warm-up. The ring rows such a tile would have written are written by the rows kernel itself (RowsExtra::hist_out), its mask
// words are zero already (EmitArgs::clear_masks). The launch is a stage of its own between the call's rows kernel and the launch
// that carries its detect stage: kernel boundaries order everything, the lists need no hand-over protocol.
// A workgroup takes C tile columns with all their frame tiles: every thread first reduces (column, frame) pairs to M
// (ten ring values each) into LDS, then thread (column, frame tile) slides the 21-frame sum over its 16 frames; the tiles to be
// evaluated — numbers in detect_tile's numbering — are appended to ONE list (list[0] = count, zeroed before the launch; one
// atomic per workgroup), so that the detect role can spread whatever there is evenly over a fixed number of workgroups: a
// workgroup per tile pair, leaving at once when the pair is culled, cost the launch 11 us in DISPATCH alone (1024 workgroups
// of eight waves take the hardware that long to start). The order of the list depends on the scheduling, the
// results do not: tiles touch disjoint mask words, and the per-frame counts are integer sums.
struct PlanLongArgs {
  const float* smax;
  int smax_mask;
  int abs0;       // frames since the last reset before this batch
  int clean_rel;  // first batch-relative frame (<= 0 in a call without learning frames) from which every row qualifies
  int cols;       // C: tile columns per workgroup
  int logn;
  int* list;
  // 0: the ring holds dB values where k_fft_rows256_psd puts them (rows_smax_index); 1: 2^20 points in two passes
  // (fft1024_kernels.h): max_key values at rows1024_smax_index(run) — [k1 group][k2], gathered by atomic maxima;
  // 2: 65536 points by the radix-8 fold (fft65536_dif8.h): value g of tile column c is the largest dB value among the column's bins
  // of residue g, at [g][c] — a column's neighbours then count with all eight of their values, not with their nearest run;
  // 3: 262144 points as 256 columns x 1024-point rows (round 6, fft1024_kernels.h: fft_rows1024_tile<8>): max_key values of the eight
  // 32-bin runs of tile column c at [run][c] (rows1024x256_smax_index), gathered by atomic maxima like layout 1's — planned by
  // plan_x256_run below (a block per 32 columns x one frame tile), not by plan_long_run
  int layout;
};
constexpr int kPlanLongFloats = 8192;  // LDS of a plan workgroup: C x (16 nft + 20) values of M
// max_c: 8, or 32 for the two-pass layout of 2^20 points — there a workgroup's columns are consecutive floats of a frame's row of
// the ring, and 32 of them are a whole 128-byte line (with 8 the four workgroups that share a line each fetched all of it:
// 5.9 against 3.0 MB per launch, 12 against 7 us, profiles/r04/s4_summary.txt)
__host__ __device__ inline int plan_long_cols(int nframes, int shift, int tile_cols, int max_c = 8, int max_floats = 8192) {  // 0: the stage cannot be planned
  const int nft = (nframes + shift + 15) / 16, rows = 16 * nft + 20;
  int c = tile_cols / 256 > 1 ? tile_cols / 256 : 1;  // at least 256 workgroups where there are that many columns
  if (max_c > 8) c = max_c;
  if (c > max_c) c = max_c;
  if (c > max_floats / rows) c = max_floats / rows;
  if (nft > 0 && c > 256 / nft) c = 256 / nft;
  return c;
}

// which tile columns a plan workgroup takes: layout 0 — (wc, d0): the columns whose unshifted number is wc + nsub d, d = d0 .. d0 + C;
// layout 1 — the columns 4 k2 + wc for k2 = d0 .. d0 + C, the 32 / C workgroups whose columns share the 128-byte lines of a frame's row
// of the ring in consecutive slots of ONE XCD (block b runs on XCD b mod 8)
__host__ __device__ inline void plan_long_block(int layout, int block, int C, int lognsub, int* wc, int* d0) {
  if (layout == 2) {  // C consecutive columns (consecutive floats of each of the eight residue rows)
    *wc = 0;
    *d0 = block * C;
  } else if (layout) {
    const int M = (C <= 32 && (32 % C) == 0) ? 32 / C : 1;
    const int xcd = block & 7, slot = block >> 3;
    *wc = xcd & 3;
    *d0 = ((((slot / M) << 1) | (xcd >> 2)) * M + slot % M) * C;
  } else {
    *wc = block & ((1 << lognsub) - 1);
    *d0 = (block >> lognsub) * C;
  }
}
__host__ __device__ inline int plan_long_blocks(int layout, int C, int n) {  // workgroups of the plan launch
  if (!layout || layout == 2) return (n >> 16) * ((256 + C - 1) / C);
  const int line_groups = (C <= 32 && 32 % C == 0) ? 32 / C : 1;
  return 4 * ((((1024 + C - 1) / C + 2 * line_groups - 1) / (2 * line_groups)) * (2 * line_groups));
}

// What the plan needs of the call's DetectArgs (the whole struct is 200 bytes of kernel arguments the column launch of a
// 2^20-point frame — whose first workgroups may run the plan of the call before, k_fft_cols1024_plan — has no use for).
struct PlanLongDet {
  int n, nframes, shift, n_learn;
  int planes_out;  // a rel or avg plane is wanted (or SS_FLAG_NO_CULL on the fold's context, ss_ctx::plan_all): nothing is tested, every tile is listed
  float start_level;
  const float* thr_tilemin;
  unsigned long long* stats;
};
__host__ __device__ inline PlanLongDet plan_long_det(const DetectArgs& d) {
  PlanLongDet a{};
  a.n = d.n;
  a.nframes = d.nframes;
  a.shift = d.shift;
  a.n_learn = d.n_learn;
  a.planes_out = (d.rel_out || d.avg_out) ? 1 : 0;
  a.start_level = d.start_level;
  a.thr_tilemin = d.thr_tilemin;
  a.stats = d.stats;
  return a;
}
constexpr int kPlanLongInts = 16;  // bookkeeping words of a plan block behind its values of M

// The decision on one tile: column `col`, first output frame f0 (batch-relative), window_sum(j) = the sum of M over the 21 frames that
// end at frame f0 + j (j < TF; each sum starts at 0.0f and adds its frames oldest first: the order is part of the result). A tile is
// TESTED only in a call without learning frames whose every row is a frame since clean_rel, and only where no plane is handed out; of a
// tested tile's windows those count that end in a frame of this batch. A sum that is not a number (a NaN run maximum, +inf and -inf in
// one window) decides nothing — the tile stays — and so does a NaN difference. Untested tiles stay.
template <int G, int TF, class WindowSum>
__device__ __forceinline__ void plan_long_decide(const PlanLongDet& a, int clean_rel, int col, int f0, WindowSum&& window_sum, bool* tested, bool* live) {
  *tested = false;
  *live = true;
  if (a.n_learn == 0 && f0 - (G - 1) >= clean_rel && !a.planes_out) {
    *tested = true;
    float best = -__builtin_inff();
    bool unsure = false;
#pragma unroll
    for (int j = 0; j < TF; ++j) {
      const float sum = window_sum(j);
      if (f0 + j >= 0 && f0 + j < a.nframes) {  // the frames of this batch the tile answers for
        unsure = unsure || (sum != sum);
        best = fmaxf(best, sum);
      }
    }
    const float bound = best * (1.0f / (float)G) - a.thr_tilemin[col];
    *live = unsure || !(bound < a.start_level - kCullMargin);  // (a NaN difference: live)
  }
}

// The hand-over of one plan block (256 threads, `tid`): the tiles that stay (`live`; `block` = the tile's number in detect_tile's
// numbering) go to the list in thread order — list[0] = the count, ONE atomic per block —, the block's counts of tested and culled tiles to
// the shard of ss_get_stats' counters that belongs to this workgroup. `book` = kPlanLongInts ints of LDS. Threads without a tile come
// with live = tested = false. The two __syncthreads() are reached by every thread of the WORKGROUP whatever the block finds: several plan
// blocks share a workgroup (k_scan_step: two, k_fft_cols1024_plan: four), and a block past the end of the plan keeps them company.
__device__ __forceinline__ void plan_long_hand_over(const PlanLongDet& a, const PlanLongArgs& p, bool live, bool tested, int block, int tid, int* __restrict__ book) {
  int* wave_cnt = book;             // [4]
  int* stat_cnt = book + 4;         // [4][2]
  int* list_base_p = book + 12;
  const int lane = tid & 63, w = tid >> 6;
  const unsigned long long mask = __ballot(live);
  if (lane == 0) wave_cnt[w] = __popcll(mask);
  if (a.stats) {  // ss_get_stats: one pair of additions per block (below), to the copy of its workgroup's block index
    const int n_tested = __popcll(__ballot(tested)), n_culled = __popcll(__ballot(tested && !live));
    if (lane == 0) {
      stat_cnt[2 * w] = n_tested;
      stat_cnt[2 * w + 1] = n_culled;
    }
  }
  __syncthreads();
  int base = 0, total = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    base += k < w ? wave_cnt[k] : 0;
    total += wave_cnt[k];
  }
  if (tid == 0) *list_base_p = total ? atomicAdd(&p.list[0], total) : 0;
  if (tid == 1 && a.stats) {
    const int nt = stat_cnt[0] + stat_cnt[2] + stat_cnt[4] + stat_cnt[6], nc = stat_cnt[1] + stat_cnt[3] + stat_cnt[5] + stat_cnt[7];
    if (nt) {
      atomicAdd(stat_word(a.stats, kStatTested), (unsigned long long)nt);
      atomicAdd(stat_word(a.stats, kStatCulled), (unsigned long long)nc);
    }
  }
  __syncthreads();
  if (live) p.list[1 + *list_base_p + base + __popcll(mask & ((1ull << lane) - 1ull))] = block;
}

// One plan block: 256 threads (`tid`), `block` = its number (what blockIdx.x is for k_plan_long), `mrow` = room for C x (16 nft + 20)
// floats, `book` = kPlanLongInts ints. Every __syncthreads() below is reached by all threads of the workgroup whatever the block
// finds: several blocks may share a workgroup (k_fft_cols1024_plan: four of them in 1024 threads).
template <int G, int GX, int TF, int TB_ = 256>
__device__ __forceinline__ void plan_long_run(const PlanLongDet& a, const PlanLongArgs& p, int block_no, int tid, float* __restrict__ mrow, int* __restrict__ book) {
  using T = DetectTile<G, GX, TF, TB_>;
  constexpr int TB = T::TB;
  static_assert(TB == 256 && T::A <= 32 && TF == 16 && G == 21, "eight 32-bin runs per tile column, one more on either side");
  const int n = a.n, nframes = a.nframes;
  const int tiles_per_row = n / TB, groups = n >> 5;
  const int nft = (nframes + a.shift + TF - 1) / TF;
  const int rows = TF * nft + (G - 1);  // frames [-shift - 20, 16 nft - shift) of the batch's frame numbering
  // this workgroup's C tile columns: the ones whose run maxima lie side by side in a frame's row of smax (rows_smax_index: the
  // same c, consecutive d) — any C columns would do, these are read with 32-byte requests instead of 4-byte ones
  const int C = p.cols, lognsub = p.logn - 16;
  // layout 0: workgroup (wc, d0) takes the columns whose unshifted number is wc + nsub d; layout 1: the columns 4 k2 + wc of C
  // consecutive k2 — either way the ones whose maxima lie side by side in a frame's row of the ring
  // (layout 1: the 32 / C workgroups whose columns share the 128-byte lines of the ring are consecutive slots of ONE XCD — block b
  // runs on XCD b mod 8 — as they are in layout 0 by construction; spread over two XCDs they fetched every line twice: 12 against
  // 7 us per call, profiles/r04/s4_summary.txt)
  int wc, d0;
  plan_long_block(p.layout, block_no, C, lognsub, &wc, &d0);
  const auto column = [&](int i) {
    if (p.layout == 2) return d0 + i < 256 ? d0 + i : tiles_per_row;
    if (p.layout) return d0 + i < 1024 ? 4 * (d0 + i) + wc : tiles_per_row;
    return d0 + i < 256 ? (wc + ((d0 + i) << lognsub)) ^ (tiles_per_row >> 1) : tiles_per_row;
  };
  for (int e = tid; e < C * rows; e += 256) {
    const int i = e % C, r = e / C, col = column(i);
    float m = -__builtin_inff();
    if (col < tiles_per_row) {
      const int frame = r - a.shift - (G - 1);
      const float* row = p.smax + ((size_t)((p.abs0 + frame) & p.smax_mask) * groups);
      // the column's eight runs, the last run of the column below and the first of the one above (the band's edges: its own once more)
      float v[10];
      if (p.layout == 2) {
        float lo = -__builtin_inff(), hi = -__builtin_inff();  // (this layout's values never hold a NaN: fft8192_v2.h takes the maxima with fmaxf)
#pragma unroll
        for (int g = 0; g < 8; ++g) {
          v[g] = row[256 * g + col];
          lo = fmaxf(lo, row[256 * g + (col > 0 ? col - 1 : col)]);
          hi = fmaxf(hi, row[256 * g + (col + 1 < tiles_per_row ? col + 1 : col)]);
        }
        v[8] = lo;
        v[9] = hi;
      } else if (p.layout) {
        const unsigned* krow = reinterpret_cast<const unsigned*>(row);
#pragma unroll
        for (int g = 0; g < 8; ++g) v[g] = max_key_value(krow[rows1024_smax_index(8 * col + g)]);
        v[8] = max_key_value(krow[rows1024_smax_index(col > 0 ? 8 * col - 1 : 8 * col)]);
        v[9] = max_key_value(krow[rows1024_smax_index(col + 1 < tiles_per_row ? 8 * col + 8 : 8 * col + 7)]);
      } else {
#pragma unroll
      for (int g = 0; g < 8; ++g) v[g] = row[rows_smax_index(col, g, p.logn)];
      v[8] = row[col > 0 ? rows_smax_index(col - 1, 7, p.logn) : rows_smax_index(col, 0, p.logn)];
      v[9] = row[col + 1 < tiles_per_row ? rows_smax_index(col + 1, 0, p.logn) : rows_smax_index(col, 7, p.logn)];
      }
      bool bad = false;
#pragma unroll
      for (int g = 0; g < 10; ++g) {
        bad = bad || (v[g] != v[g]);
        m = fmaxf(m, v[g]);
      }
      if (bad) m = __builtin_nanf("");
    }
    mrow[i * rows + r] = m;
  }
  __syncthreads();
  bool live = false, tested = false;
  int block = 0;
  if (tid < C * nft && column(tid / nft) < tiles_per_row) {
    const int cl = tid / nft, ft_seq = tid % nft;
    const int ft = (ft_seq + nft - 1) % nft;
    const int f0 = ft * TF - a.shift;
    block = ft_seq * tiles_per_row + column(cl);
    const float* mr = mrow + cl * rows + ft * TF;  // mr[k] = M of frame f0 - 20 + k
    plan_long_decide<G, TF>(a, p.clean_rel, column(cl), f0, [mr](int j) {
      float sum = 0.0f;
#pragma unroll
      for (int k = 0; k < G; ++k) sum += mr[j + k];
      return sum;
    }, &tested, &live);
  }
  plan_long_hand_over(a, p, live, tested, block, tid, book);  // this workgroup's list, in thread order
}

// The 32-column decomposition that plan_dif8_run and plan_x256_run share: one block = 32 consecutive tile columns x ONE frame tile, 256
// threads, in three steps with LDS between them —
//   1  R[colx][row] = the largest run maximum of column colx (34 of them: the block's 32 and one either side; the band's edges: the edge
//      column once more) in frame row `row` (36: the tile's 16 frames and the 20 before) — lanes along the columns, so a wave's load is
//      one line, a thread's forty loads in one flight. Each plan's own: floats by fmaxf, or order-preserving keys by integer max;
//   2  M = max(R[col - 1], R[col], R[col + 1]) formed on the fly, S[col][j] = the 21-frame window sum that ends at frame j of the tile
//      (thread per (col, j): 21 x 3 LDS reads);
//   3  thread per tile: plan_long_decide on its sixteen sums, plan_long_hand_over.
// `lds`: kPlanCols32Floats floats (R, then S), kPlanLongInts ints (`book`) behind them.
constexpr int kPlanCols32Rows = 16 + 21 - 1, kPlanCols32Pitch = kPlanCols32Rows + 1;  // 36 frame rows per tile, LDS pitch 37
constexpr int kPlanCols32Floats = 34 * kPlanCols32Pitch + 32 * 16;
constexpr int kPlanDif8Floats = kPlanCols32Floats;
// Which tile a block takes: column group b mod 2^log_groups (32 columns: the groups of a frame tile are consecutive blocks, spread over
// the XCDs), frame tile b >> log_groups in dispatch order (plan_long_run's ft_seq).
struct PlanCols32Block {
  int ft_seq, f0, c0;  // f0: batch-relative frame of the tile's first row of outputs; c0: the block's first column
  bool in_range;       // (a workgroup's second block may lie past the end: it keeps the barriers company)
};
template <int TF>
__device__ __forceinline__ PlanCols32Block plan_cols32_block(const PlanLongDet& a, int block_no, int log_groups) {
  const int nft = (a.nframes + a.shift + TF - 1) / TF;
  PlanCols32Block b;
  b.ft_seq = block_no >> log_groups;
  b.in_range = b.ft_seq < nft;
  const int ft = b.in_range ? (b.ft_seq + nft - 1) % nft : 0;
  b.f0 = ft * TF - a.shift;
  b.c0 = 32 * (block_no & ((1 << log_groups) - 1));
  return b;
}
// Steps 2 and 3, from R as step 1 left it (this function's first barrier is the one behind step 1). Every __syncthreads() is reached by
// all threads of the workgroup whatever the block finds, as plan_long_hand_over wants it.
template <int G, int TF>
__device__ __forceinline__ void plan_cols32_finish(const PlanLongDet& a, const PlanLongArgs& p, const PlanCols32Block& b, int tiles_per_row, int tid, float* __restrict__ lds,
                                                   int* __restrict__ book) {
  static_assert(TF + G - 1 == kPlanCols32Rows, "36 frame rows per tile");
  constexpr int RP = kPlanCols32Pitch;
  const float* R = lds;       // [34][RP]
  float* S = lds + 34 * RP;   // [32][TF]
  __syncthreads();
  if (b.in_range) {
    for (int e = tid; e < 32 * TF; e += 256) {
      const int cl = e >> 4, j = e & 15;
      const float *r0 = R + cl * RP + j, *r1 = r0 + RP, *r2 = r1 + RP;
      float sum = 0.0f;
#pragma unroll
      for (int k = 0; k < G; ++k) sum += fmaxf(fmaxf(r0[k], r1[k]), r2[k]);  // M of frame f0 - 20 + j + k
      S[e] = sum;
    }
  }
  __syncthreads();
  bool live = false, tested = false;
  int block = 0;
  if (b.in_range && tid < 32) {
    const int col = b.c0 + tid;
    block = b.ft_seq * tiles_per_row + col;
    plan_long_decide<G, TF>(a, p.clean_rel, col, b.f0, [S, tid](int j) { return S[tid * TF + j]; }, &tested, &live);
  }
  plan_long_hand_over(a, p, live, tested, block, tid, book);  // this block's share of the list, in thread order
}

// The plan for the radix-8 fold's rows (layout 2): one block = 32 consecutive tile columns x ONE frame tile, 256 threads. What
// plan_long_run does for this layout — a block per tile column with all its frame tiles — fetched every 128-byte line of the run
// maxima thirty-two times over (a column's eight values per frame sit in eight different lines, each shared with 31 other columns:
// 143 MB of L1 fills per 512-frame call) and left all but a few dozen of its threads idle through 336 serial LDS reads; as the first
// 128 workgroups of the fold's launch it cost a 128-frame call 8 us and a 512-frame call 12-16 (profiles/r05/s8_summary.txt). Here: the
// 32-column decomposition above; step 1 takes the maximum over the fold's residues, floats by fmaxf.
// Block b: column group b mod 8 (32 columns: the eight groups of a frame tile are consecutive blocks, one per XCD), frame tile b / 8 in
// dispatch order (plan_long_run's ft_seq). `lds`: kPlanDif8Floats floats + kPlanLongInts ints behind them.
// Radix Q = 1 << logq (logq = p.logn - 13: 3 or 4): 32 Q tile columns, Q column groups per frame tile; a run of a residue's row (32 of
// its bins) spans Q / 8 tile columns.
__host__ __device__ inline int plan_dif8_blocks(int nframes, int shift, int logq = 3) { return ((nframes + shift + 15) / 16) << logq; }
template <int G, int GX, int TF, int TB_ = 256>
__device__ __forceinline__ void plan_dif8_run(const PlanLongDet& a, const PlanLongArgs& p, int block_no, int tid, float* __restrict__ lds, int* __restrict__ book) {
  static_assert(TB_ == 256 && TF == 16 && G == 21, "the fold's rows: tile columns of 256 bins, tiles of 16 frames");
  constexpr int ROWS = kPlanCols32Rows, RP = kPlanCols32Pitch;
  float* R = lds;  // [34][RP]
  const int logq = p.logn - 13, nres = 1 << logq;
  const int tiles_per_row = 32 << logq;
  const PlanCols32Block b = plan_cols32_block<TF>(a, block_no, logq);
  const bool in_range = b.in_range;
  const int f0 = b.f0, c0 = b.c0;
  if (in_range) {
    // (a thread's five entries, eight residues each: forty loads in flight at once. One entry after the other, a residue after the
    // other, this was forty round trips to L2 beside workgroups that keep the memory system busy — a plan workgroup held its slot for
    // 14 us of a 128-frame launch and the 32 fold workgroups that had to wait for those slots ended it 7 us late, profiles/r05/s24_*)
    constexpr int NE = (34 * ROWS + 255) / 256;
    const float* src[NE];
    float m[NE];
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int e = min(tid + 256 * i, 34 * ROWS - 1);
      const int colx = e % 34, r = e / 34;
      const int col = min(max(c0 - 1 + colx, 0), tiles_per_row - 1);  // (the band's edges: the edge column once more)
      src[i] = p.smax + ((size_t)((p.abs0 + f0 - (G - 1) + r) & p.smax_mask) << (8 + logq)) + (col >> (logq - 3));  // (radix 16: a run of a residue's row covers two tile columns)
      m[i] = -__builtin_inff();
    }
    for (int g0 = 0; g0 < nres; g0 += 8) {
      float v[NE][8];
#pragma unroll
      for (int i = 0; i < NE; ++i)
#pragma unroll
        for (int g = 0; g < 8; ++g) v[i][g] = src[i][256 * (g0 + g)];
#pragma unroll
      for (int i = 0; i < NE; ++i)
#pragma unroll
        for (int g = 0; g < 8; ++g) m[i] = fmaxf(m[i], v[i][g]);  // (the fold's maxima hold no NaN: fft8192_v2.h takes them with fmaxf)
    }
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int e = tid + 256 * i;
      if (e < 34 * ROWS) R[(e % 34) * RP + e / 34] = m[i];
    }
  }
  plan_cols32_finish<G, TF>(a, p, b, tiles_per_row, tid, lds, book);
}

// The plan for 262144-point frames (layout 3): the fold's decomposition — one block = 32 consecutive tile columns x ONE frame tile, 256
// threads, a thread's forty loads in one flight — over max_key values at [run g < 8][column < 1024] per frame. Block b: column group
// b mod 32, frame tile b / 32 in dispatch order. A key of "NaN" (a NaN bin in the run: cannot be bounded) counts as +inf: the tile is
// evaluated. `lds`: kPlanDif8Floats floats + kPlanLongInts ints behind them.
__host__ __device__ inline int plan_x256_blocks(int nframes, int shift) { return ((nframes + shift + 15) / 16) << 5; }
template <int G, int GX, int TF, int TB_ = 256>
__device__ __forceinline__ void plan_x256_run(const PlanLongDet& a, const PlanLongArgs& p, int block_no, int tid, float* __restrict__ lds, int* __restrict__ book) {
  static_assert(TB_ == 256 && TF == 16 && G == 21, "tile columns of 256 bins, tiles of 16 frames");
  constexpr int ROWS = kPlanCols32Rows, RP = kPlanCols32Pitch;
  float* R = lds;  // [34][RP]
  constexpr int tiles_per_row = 1024;
  const PlanCols32Block b = plan_cols32_block<TF>(a, block_no, 5);
  const bool in_range = b.in_range;
  const int f0 = b.f0, c0 = b.c0;
  if (in_range) {
    constexpr int NE = (34 * ROWS + 255) / 256;
    const unsigned* src[NE];
    unsigned m[NE];
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int e = min(tid + 256 * i, 34 * ROWS - 1);
      const int colx = e % 34, r = e / 34;
      const int col = min(max(c0 - 1 + colx, 0), tiles_per_row - 1);  // (the band's edges: the edge column once more)
      src[i] = reinterpret_cast<const unsigned*>(p.smax) + ((size_t)((p.abs0 + f0 - (G - 1) + r) & p.smax_mask) << 13) + col;
    }
    unsigned v[NE][8];
#pragma unroll
    for (int i = 0; i < NE; ++i)
#pragma unroll
      for (int g = 0; g < 8; ++g) v[i][g] = src[i][1024 * g];
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      m[i] = 0u;
#pragma unroll
      for (int g = 0; g < 8; ++g) m[i] = max(m[i], v[i][g]);  // (order-preserving keys: the NaN key is the largest)
    }
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int e = tid + 256 * i;
      if (e < 34 * ROWS) R[(e % 34) * RP + e / 34] = m[i] == 0xffffffffu ? __builtin_inff() : max_key_value(m[i]);
    }
  }
  plan_cols32_finish<G, TF>(a, p, b, tiles_per_row, tid, lds, book);  // (no NaN among the values of R: see above; +inf and -inf in one window make a NaN sum)
}
// workgroups (blocks) of a long transform's plan, whatever its layout
__host__ __device__ inline int plan_blocks_of(const PlanLongDet& a, const PlanLongArgs& p, int n) {
  if (p.layout == 3) return plan_x256_blocks(a.nframes, a.shift);
  if (p.layout == 2) return plan_dif8_blocks(a.nframes, a.shift, p.logn - 13);
  return plan_long_blocks(p.layout, p.cols, n);
}

template <int G, int GX, int TF, int TB_ = 256>
__global__ __launch_bounds__(256) void k_plan_long(PlanLongDet a, PlanLongArgs p) {
  __shared__ float mrow[kPlanLongFloats];
  __shared__ int book[kPlanLongInts];
  if (p.layout == 2) return plan_dif8_run<G, GX, TF, TB_>(a, p, (int)blockIdx.x, (int)threadIdx.x, mrow, book);
  if (p.layout == 3) return plan_x256_run<G, GX, TF, TB_>(a, p, (int)blockIdx.x, (int)threadIdx.x, mrow, book);
  plan_long_run<G, GX, TF, TB_>(a, p, (int)blockIdx.x, (int)threadIdx.x, mrow, book);
}

// 2^20 points in two passes: the plan of call k as the FIRST workgroups of the column launch of call k + 1 (fft1024_kernels.h,
// 16-column tiles by 1024 threads). As a launch of its own between the row launch of call k and the column launch of call k + 1
// the plan cost a 16-frame call 11.6 us of a chip that waits for 3 MB of run maxima, plus a launch boundary; here its blocks —
// four to a workgroup of 1024 threads, so that the blocks whose columns share the 128-byte lines of the ring share a workgroup — hold
// `plan_wgs` of the launch's first slots for a few microseconds while the column tiles stream in beside them. What the plan reads
// (the run maxima of frames up to call k's last) was complete before this launch began; the rows of the ring the column tiles clear
// in the same launch are those of call k + 1's frames (the ring holds two batches and the averager's reach: ss_create), which the
// plan touches only where a ragged frame tile reaches past its batch and then ignores. Its consumer — the detect stage of call k —
// rides on the launch AFTER this one (the row half of call k + 1). `plan_wgs` is a multiple of 8: the column tiles keep their XCDs.
constexpr int kPlanFusedFloats = 4096;  // values of M per plan block when four blocks share the column tile's LDS (plan_long_cols: cap)
template <int FMT, bool WCALC>
__global__ __launch_bounds__(1024, 8) void k_fft_cols1024_plan(ColsArgs g, PlanLongDet a, PlanLongArgs p, int plan_wgs) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  static_assert(4 * (kPlanFusedFloats + kPlanLongInts) * 4 <= fft1024_cols_lds_bytes(4), "four plan blocks in a column tile's LDS");
  const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
  if (b < plan_wgs) {  // (workgroup-uniform)
    const int sub = tid >> 8;
    float* mrow = reinterpret_cast<float*>(smem_raw) + sub * (kPlanFusedFloats + kPlanLongInts);
    // plan block number: XCD b mod 8 as k_plan_long's block numbering has it (plan_long_block), the workgroup's four blocks in
    // consecutive slots of that XCD
    plan_long_run<21, 21, 16, 256>(a, p, ((((b >> 3) << 2) + sub) << 3) | (b & 7), tid & 255, mrow, reinterpret_cast<int*>(mrow + kPlanFusedFloats));
    return;
  }
  fft_cols1024_tile<FMT, 4, WCALC>(g, b - plan_wgs, smem_raw, tid);
}
__host__ __device__ inline int plan_fused_wgs(int plan_blocks) { return (((plan_blocks + 3) / 4 + 7) / 8) * 8; }

}  // namespace ss
