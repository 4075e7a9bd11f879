// track_digest_blocked.h — the candidates' kernel of the tracking digest (track_digest.h: per candidate the mode of the window arg-maxes
// of the newest rel rows), by a blocked sliding arg-max: a lane's work per row does not grow with the window, and one row at a time
// sits in LDS, so a window may be thousands of bins wide. (It replaced a bin-by-bin walk of every window, now retired.)
//
// A row is cut into blocks of W = 2 * half + 1 bins, aligned at bin 0 of the row, the last one clipped at n. Two tables per staged bin:
//   P[i]  arg-max of [block start, i]: scanned forward, a bin replaces the running best if it is no NaN and nothing is held yet or its
//         value is strictly greater; all NaN so far: none
//   S[i]  arg-max of [i, block end]: scanned backward, replaces on greater or equal (the lower bin wins a tie); all NaN: none
// Both are "the first maximum of the range, NaNs left out", and so is the join of two adjacent ranges (best_join). The window
// [lo, hi) = [max(0, c - half), min(n, c + half + 1)) of a candidate reaches into two blocks at most, and std::max_element's answer is:
//   row[lo] is NaN: lo. lo is a block start: P[hi - 1]. Otherwise S[lo], displaced by P[hi - 1] if hi - 1 lies in the next block and
//   row[P[hi - 1]] is strictly greater.
// (lo inside a block with hi - 1 inside the same block short of its clipped end cannot happen: an unclipped window is exactly W bins.)
//
// The tables are built by all 256 threads: each scans a contiguous chunk of the staged span, then a segmented scan over the chunks'
// results (segment heads: block starts for P, block ends for S) — shuffles inside a wave, the four waves' totals through LDS — gives
// every chunk what lies before (behind) it in its block, and the chunk's entries up to its first head are joined with that.
// The staged span [s_lo, s_hi] of the tile is enough: P[hi - 1] is never asked for a block that starts below s_lo unless lo is that
// start (and lo >= s_lo), S[lo] never for a block that ends above s_hi unless hi - 1 = n - 1 = s_hi.
//
// A lane keeps the arg-maxes of the rows that qualify in an ascending list in LDS (list_insert) and answers with their mode (list_mode).
//
// The table build, the query and the list functions are plain functions over pointers; tests/host/blocked_argmax_check.cpp compiles them
// for the host.
#pragma once
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#include "track_digest.h"
#define SS_BLOCKED_HD __host__ __device__ __forceinline__
#else
#define SS_BLOCKED_HD inline
#endif

namespace ss {

constexpr int kBlockedLanes = 256;        // threads of k_best_blocked (= kTrackTile)
constexpr uint32_t kBestNone = 0xffffu;   // "none" in P, S and Best::i (offsets from the staged base are below it: the span fits LDS)

struct Best {
  float v;
  uint32_t i;  // offset from the staged base, or kBestNone
};

// the first maximum of two adjacent ranges, a the earlier one
SS_BLOCKED_HD Best best_join(Best a, Best b) { return (a.i == kBestNone || (b.i != kBestNone && b.v > a.v)) ? b : a; }

struct SegBest {
  Best b;
  bool head;  // the range holds a segment head: what b covers ends there
};

SS_BLOCKED_HD SegBest seg_none() { return SegBest{Best{0.0f, kBestNone}, false}; }
// forward (heads are block starts; b covers from the range's last head on): a then b
SS_BLOCKED_HD SegBest seg_join_fwd(SegBest a, SegBest b) { return b.head ? b : SegBest{best_join(a.b, b.b), a.head}; }
// backward (heads are block ends; b covers up to the range's first head): a then b
SS_BLOCKED_HD SegBest seg_join_bwd(SegBest a, SegBest b) { return a.head ? a : SegBest{best_join(a.b, b.b), b.head}; }

// lane's chunk [c0, c1) of a staged span of len bins
SS_BLOCKED_HD void blocked_chunk(int lane, int len, int& c0, int& c1) {
  const int per = (len + kBlockedLanes - 1) / kBlockedLanes;
  c0 = lane * per < len ? lane * per : len;
  c1 = c0 + per < len ? c0 + per : len;
}

// P over the chunk alone (row, P: offset 0 is bin s_lo; blocks of W bins from bin 0; rem = (s_lo + c0) % W, where the chunk's first bin
// lies in its block). Returns the chunk's part behind its last block start.
SS_BLOCKED_HD SegBest blocked_prefix_local(const float* row, uint16_t* P, int W, int rem, int c0, int c1) {
  SegBest r = seg_none();
  for (int o = c0; o < c1; ++o) {
    if (rem == 0) {
      r.b.i = kBestNone;
      r.head = true;
    }
    const float v = row[o];
    if (v == v && (r.b.i == kBestNone || v > r.b.v)) {
      r.b.v = v;
      r.b.i = (uint32_t)o;
    }
    P[o] = (uint16_t)r.b.i;
    if (++rem == W) rem = 0;
  }
  return r;
}

// ... joined with carry, the first maximum of the block's bins in front of the chunk, up to the chunk's first block start
SS_BLOCKED_HD void blocked_prefix_fix(const float* row, uint16_t* P, int W, int rem, int c0, int c1, Best carry) {
  if (carry.i == kBestNone) return;
  for (int o = c0; o < c1 && rem != 0; ++o) {
    const uint32_t p = P[o];
    if (p != kBestNone && row[p] > carry.v) break;  // (the chunk's running maximum only grows from here)
    P[o] = (uint16_t)carry.i;
    if (++rem == W) rem = 0;
  }
}

// S over the chunk alone (rem = (s_lo + c1 - 1) % W: the chunk's last bin). Returns the chunk's part up to its first block end.
SS_BLOCKED_HD SegBest blocked_suffix_local(const float* row, uint16_t* S, int W, int rem, int c0, int c1) {
  SegBest r = seg_none();
  for (int o = c1 - 1; o >= c0; --o) {
    if (rem == W - 1) {
      r.b.i = kBestNone;
      r.head = true;
    }
    const float v = row[o];
    if (v == v && (r.b.i == kBestNone || v >= r.b.v)) {
      r.b.v = v;
      r.b.i = (uint32_t)o;
    }
    S[o] = (uint16_t)r.b.i;
    if (rem-- == 0) rem = W - 1;
  }
  return r;
}

// ... joined with carry, the first maximum of the block's bins behind the chunk, down to the chunk's last block end
SS_BLOCKED_HD void blocked_suffix_fix(const float* row, uint16_t* S, int W, int rem, int c0, int c1, Best carry) {
  if (carry.i == kBestNone) return;
  for (int o = c1 - 1; o >= c0 && rem != W - 1; --o) {
    const uint32_t s = S[o];
    if (s != kBestNone && !(carry.v > row[s])) break;  // (a tie stays with the lower bin)
    S[o] = (uint16_t)carry.i;
    if (rem-- == 0) rem = W - 1;
  }
}

// std::max_element over the bins [lo, hi) of the row (s_lo <= lo < hi, hi - lo <= W; rem = lo % W), from the finished tables
SS_BLOCKED_HD int blocked_query(const float* row, const uint16_t* P, const uint16_t* S, int s_lo, int W, int rem, int lo, int hi) {
  const float head = row[lo - s_lo];
  if (head != head) return lo;
  if (rem == 0) return s_lo + (int)P[hi - 1 - s_lo];
  uint32_t a = S[lo - s_lo];
  if (hi - 1 > lo - rem + W - 1) {
    const uint32_t b = P[hi - 1 - s_lo];
    if (b != kBestNone && row[b] > row[a]) a = b;
  }
  return s_lo + (int)a;
}

// A lane's list: entry k at list[k * stride], ascending. Inserts v into a list of m entries; the caller counts.
SS_BLOCKED_HD void list_insert(int* list, int stride, int m, int v) {
  int k = m;
  while (k > 0 && list[(k - 1) * stride] > v) {
    list[k * stride] = list[(k - 1) * stride];
    --k;
  }
  list[k * stride] = v;
}

// mostFrequentValue over the list's m entries: of the runs of equal values, the longest; of several that long, the one at position
// ties / 2 in ascending order. An empty list gives otherwise.
SS_BLOCKED_HD int list_mode(const int* list, int stride, int m, int otherwise) {
  int result = otherwise;
  if (m > 0) {
    int top = 0, ties = 0;
    for (int i = 0; i < m;) {
      const int v = list[i * stride];
      int e = i + 1;
      while (e < m && list[e * stride] == v) ++e;
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
      const int v = list[i * stride];
      int e = i + 1;
      while (e < m && list[e * stride] == v) ++e;
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
  return result;
}

// dynamic LDS of k_best_blocked: one row's values, P and S, the lanes' lists, the waves' totals
SS_BLOCKED_HD size_t blocked_lds_bytes(int nrows, int half) {
  return (size_t)8 * (size_t)(kBlockedLanes + 2 * half) + sizeof(int) * (size_t)nrows * kBlockedLanes + 64;
}

#ifdef __HIPCC__  // the kernel itself

static_assert(kBlockedLanes == kTrackTile, "one lane per bin of a tile");

// Rows: where the rel rows live — RelRows (k_best_blocked), or track_digest_sparse.h's RingRows; anything with n and a rel_at
template <class Rows>
struct CandBestArgsOf {
  Rows rows;
  const float* avg;         // the batch's avg plane
  const int32_t* cand_off;  // [nframes + 1], clipped to ncand
  const int32_t* cand_idx;  // [ncand], ascending inside a frame
  int32_t* cand_best;       // [ncand]
  float* cand_avg;          // [ncand]
  int nframes;
  int tiles;       // ceil(n / kTrackTile)
  int half;        // group_size / 2
  int nrows;       // ceil(grouping_y / 2) = tail_rows + 1
  int width;       // staged bins of a row: kTrackTile + 2 * half
  float start_level;
};
using CandBestArgs = CandBestArgsOf<RelRows>;

// first candidate of the frame's list [a, b) at or above bin: the lists are ascending
__device__ __forceinline__ int cand_lower_bound(const int32_t* idx, int a, int b, int bin) {
  while (a < b) {
    const int m = (a + b) >> 1;
    if (idx[m] < bin) a = m + 1;
    else b = m;
  }
  return a;
}

__device__ __forceinline__ SegBest seg_shfl_up(SegBest x, int d) {
  const uint32_t k = __shfl_up(x.b.i | (x.head ? 0x10000u : 0u), d, 64);
  return SegBest{Best{__shfl_up(x.b.v, d, 64), k & 0xffffu}, (k & 0x10000u) != 0};
}

__device__ __forceinline__ SegBest seg_shfl_down(SegBest x, int d) {
  const uint32_t k = __shfl_down(x.b.i | (x.head ? 0x10000u : 0u), d, 64);
  return SegBest{Best{__shfl_down(x.b.v, d, 64), k & 0xffffu}, (k & 0x10000u) != 0};
}

// grid nframes * tiles, 256 threads. A workgroup whose tile of its frame holds no candidate returns at once; otherwise it stages, row
// by row, the bins its candidates' windows can touch, and lane t takes the tile's t-th candidate (a tile holds at most 256).
// Dynamic LDS (blocked_lds_bytes): width floats (the row), nrows * 256 ints (the lanes' ascending lists), width + width 16-bit
// offsets (P, S), 16 words (wave totals). The body over the row source; lds_blocked is the kernel's dynamic LDS.
template <class Rows>
__device__ __forceinline__ void best_blocked_tile(const CandBestArgsOf<Rows>& a, float* lds_blocked) {
  const int n = a.rows.n;
  const int f = blockIdx.x / a.tiles;
  const int t0 = (blockIdx.x % a.tiles) * kTrackTile;
  const int list_lo = a.cand_off[f], list_hi = a.cand_off[f + 1];
  if (list_lo >= list_hi) return;
  const int first = cand_lower_bound(a.cand_idx, list_lo, list_hi, t0);
  const int last = cand_lower_bound(a.cand_idx, first, list_hi, t0 + kTrackTile);
  if (first >= last) return;  // (uniform over the workgroup: nobody waits at the barriers below)
  float* row = lds_blocked;                                               // [width], row[0] is bin s_lo
  int* sorted = reinterpret_cast<int*>(row + a.width);                    // [nrows][256]: lane t's qualifying arg-maxes, ascending
  uint16_t* P = reinterpret_cast<uint16_t*>(sorted + a.nrows * kTrackTile);  // [width]
  uint16_t* S = P + a.width;                                              // [width]
  float* tot_v = reinterpret_cast<float*>(S + a.width);                   // [8]: the waves' prefix totals, then their suffix totals
  uint32_t* tot_k = reinterpret_cast<uint32_t*>(tot_v + 8);               // [8]
  const int s_lo = t0 - a.half < 0 ? 0 : t0 - a.half;
  const int s_hi = t0 + kTrackTile - 1 + a.half < n ? t0 + kTrackTile - 1 + a.half : n - 1;  // last staged bin
  const int len = s_hi - s_lo + 1, W = 2 * a.half + 1;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int c0, c1;
  blocked_chunk(tid, len, c0, c1);
  const int rem0 = c0 < c1 ? (s_lo + c0) % W : 0, rem1 = c0 < c1 ? (s_lo + c1 - 1) % W : 0;  // (an empty chunk's loops do not run)
  const int j = first + tid;
  const bool active = j < last;
  int c = 0, lo = 0, hi = 1;
  if (active) {
    c = a.cand_idx[j];
    lo = c - a.half < 0 ? 0 : c - a.half;
    hi = c + a.half + 1 < n ? c + a.half + 1 : n;
  }
  const int rem_lo = lo % W;
  int* mine = sorted + tid;
  int m = 0;
  for (int r = 0; r < a.nrows; ++r) {
    const int frame = f - (a.nrows - 1) + r;
    for (int i = s_lo + tid; i <= s_hi; i += kTrackTile) row[i - s_lo] = rel_at(a.rows, frame, i);
    __syncthreads();
    SegBest p = blocked_prefix_local(row, P, W, rem0, c0, c1);
    SegBest s = blocked_suffix_local(row, S, W, rem1, c0, c1);
    for (int d = 1; d < 64; d <<= 1) {  // inclusive over the wave's chunks: lanes below bring what lies in front, lanes above what lies behind
      const SegBest up = seg_shfl_up(p, d), down = seg_shfl_down(s, d);
      if (lane >= d) p = seg_join_fwd(up, p);
      if (lane + d < 64) s = seg_join_bwd(s, down);
    }
    if (lane == 63) {
      tot_v[wave] = p.b.v;
      tot_k[wave] = p.b.i | (p.head ? 0x10000u : 0u);
    }
    if (lane == 0) {
      tot_v[4 + wave] = s.b.v;
      tot_k[4 + wave] = s.b.i | (s.head ? 0x10000u : 0u);
    }
    __syncthreads();
    SegBest before = seg_shfl_up(p, 1), behind = seg_shfl_down(s, 1);  // exclusive: the neighbour's inclusive result ...
    if (lane == 0) before = seg_none();
    if (lane == 63) behind = seg_none();
    SegBest carry = seg_none();  // ... behind the other waves' totals
    for (int w = 0; w < wave; ++w) carry = seg_join_fwd(carry, SegBest{Best{tot_v[w], tot_k[w] & 0xffffu}, (tot_k[w] & 0x10000u) != 0});
    before = seg_join_fwd(carry, before);
    carry = seg_none();
    for (int w = 3; w > wave; --w) carry = seg_join_bwd(SegBest{Best{tot_v[4 + w], tot_k[4 + w] & 0xffffu}, (tot_k[4 + w] & 0x10000u) != 0}, carry);
    behind = seg_join_bwd(behind, carry);
    blocked_prefix_fix(row, P, W, rem0, c0, c1, before.b);
    blocked_suffix_fix(row, S, W, rem1, c0, c1, behind.b);
    __syncthreads();
    if (active) {
      const int best = blocked_query(row, P, S, s_lo, W, rem_lo, lo, hi);
      if (a.start_level <= row[best - s_lo]) list_insert(mine, kTrackTile, m++, best);
    }
    __syncthreads();  // (the next row overwrites row, P and S)
  }
  if (!active) return;
  a.cand_best[j] = list_mode(mine, kTrackTile, m, c);  // no row qualifies: the candidate itself (signal_tracker.cpp, getBestIndex)
  a.cand_avg[j] = a.avg[(size_t)f * n + c];
}

__global__ __launch_bounds__(kTrackTile) void k_best_blocked(const CandBestArgs a) {
  extern __shared__ float lds_blocked[];
  best_blocked_tile(a, lds_blocked);
}

#endif  // __HIPCC__

}  // namespace ss
