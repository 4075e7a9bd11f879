// track_feed.h — the tracking digest behind the pipelined feed (include/specscan_track_feed.h): the steps of st_digest that ran on the
// host — clipping the offsets, forming the watch list — as kernels, so that a batch is digested in the stream right behind its chain,
// with no host wait in between. The candidates' kernel (k_best_blocked of track_digest_blocked.h; launch_cand_best in host_track.h)
// and k_save_tail of track_digest.h run unchanged between them.
//
//   k_feed_prepare   coff[f] = min(off[f], cand_cap); keymark[key] = seq for the posted keys; the header's flags to zero
//   k_feed_stamp     mark[cand_best[j]] = seq for every candidate of the clipped lists
//   k_feed_count     per 256-bin block: how many bins are watched (mark > p, or keymark == seq)
//   k_feed_scan      exclusive scan of the block counts (one wave, a run of consecutive counts per lane); writes the header
//   k_feed_scatter   the watched bins, ascending, to watch[0 .. min(nwatch, max_watch))
//   k_feed_peaks     k_window_peaks (its window_peak) over a list whose length only the device knows: grid-stride, one wave per (frame, watch key)
//
// The watch list: mark[b] is the sequence number of the newest batch that had b as cand_best of a candidate, keymark[b] the one of the
// newest batch whose submit found b among the posted keys K_p. Batch seq watches {b: mark[b] > p} U {b: keymark[b] == seq}
// = K_p U cand_best(p + 1) U ... U cand_best(seq), a superset of every key the host tracker can hold while it walks the batch.
// Every writer of a word in one launch writes the same value: plain stores, no atomics. Sequence numbers are 32 bits on the device.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "track_digest.h"

namespace ss {

constexpr int kFeedBlock = 256;  // bins per block of the compaction, and its threads

// what the host reads first at collect time (pinned copy); flags: 1 = more than max_watch watch keys, 2 = a cand_best outside [0, n)
struct FeedDigestHeader {
  int32_t ncand_total;  // off[nframes]: what the batch found
  int32_t ncand;        // min(ncand_total, cand_cap): what the lists hold
  int32_t nwatch;       // the true count, also past max_watch
  int32_t flags;
};
constexpr int kFeedOverflow = 1, kFeedBadBest = 2;

struct FeedPrepareArgs {
  const int32_t* off;   // [nframes + 1] as the chain wrote them
  int32_t* coff;        // [nframes + 1] clipped
  const int32_t* keys;  // [nkeys] the posted keys, each inside [0, n): checked by stf_post_keys
  uint32_t* keymark;    // [n]
  FeedDigestHeader* hdr;
  int nframes, cand_cap, nkeys;
  uint32_t seq;
};

__global__ __launch_bounds__(256) void k_feed_prepare(const FeedPrepareArgs a) {
  const int stride = (int)gridDim.x * 256;
  const int t = (int)blockIdx.x * 256 + (int)threadIdx.x;
  for (int f = t; f <= a.nframes; f += stride) {
    const int o = a.off[f];
    a.coff[f] = o < a.cand_cap ? o : a.cand_cap;
  }
  for (int k = t; k < a.nkeys; k += stride) a.keymark[a.keys[k]] = a.seq;
  if (t == 0) a.hdr->flags = 0;
}

// grid-stride over the clipped lists; their length is read on the device
__global__ __launch_bounds__(256) void k_feed_stamp(const int32_t* __restrict__ coff, int nframes, const int32_t* __restrict__ cand_best, uint32_t* __restrict__ mark,
                                                    int n, uint32_t seq, FeedDigestHeader* hdr) {
  const int ncand = coff[nframes];
  for (int j = (int)blockIdx.x * 256 + (int)threadIdx.x; j < ncand; j += (int)gridDim.x * 256) {
    const uint32_t b = (uint32_t)cand_best[j];
    if (b < (uint32_t)n) mark[b] = seq;
    else hdr->flags = kFeedBadBest;
  }
}

__device__ __forceinline__ bool feed_watched(const uint32_t* mark, const uint32_t* keymark, int bin, int n, uint32_t p, uint32_t seq) {
  return bin < n && (mark[bin] > p || keymark[bin] == seq);
}

// grid ceil(n / 256): counts[block]
__global__ __launch_bounds__(kFeedBlock) void k_feed_count(const uint32_t* __restrict__ mark, const uint32_t* __restrict__ keymark, int n, uint32_t p, uint32_t seq,
                                                           int32_t* __restrict__ counts) {
  __shared__ int wave_cnt[kFeedBlock / 64];
  const int bin = (int)blockIdx.x * kFeedBlock + (int)threadIdx.x;
  const unsigned long long m = __ballot(feed_watched(mark, keymark, bin, n, p, seq));
  if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// one wave: lane l owns counts[l * per .. (l + 1) * per), per = ceil(nblocks / 64); counts become their exclusive prefix sums
__global__ __launch_bounds__(64) void k_feed_scan(int32_t* __restrict__ counts, int nblocks, const int32_t* __restrict__ off, const int32_t* __restrict__ coff, int nframes,
                                                  int max_watch, FeedDigestHeader* hdr) {
  const int lane = (int)threadIdx.x;
  const int per = (nblocks + 63) / 64;
  const int lo = lane * per < nblocks ? lane * per : nblocks;
  const int hi = lo + per < nblocks ? lo + per : nblocks;
  int sum = 0;
  for (int i = lo; i < hi; ++i) sum += counts[i];
  int incl = sum;
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  int run = incl - sum;
  for (int i = lo; i < hi; ++i) {
    const int c = counts[i];
    counts[i] = run;
    run += c;
  }
  if (lane == 63) {  // (its inclusive sum is the total)
    hdr->ncand_total = off[nframes];
    hdr->ncand = coff[nframes];
    hdr->nwatch = incl;
    if (incl > max_watch) hdr->flags = hdr->flags | kFeedOverflow;
  }
}

// grid ceil(n / 256), behind k_feed_scan: block_off[block] is the block's first position in the list
__global__ __launch_bounds__(kFeedBlock) void k_feed_scatter(const uint32_t* __restrict__ mark, const uint32_t* __restrict__ keymark, int n, uint32_t p, uint32_t seq,
                                                             const int32_t* __restrict__ block_off, int max_watch, int32_t* __restrict__ watch) {
  __shared__ int wave_cnt[kFeedBlock / 64];
  const int bin = (int)blockIdx.x * kFeedBlock + (int)threadIdx.x;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const bool mine = feed_watched(mark, keymark, bin, n, p, seq);
  const unsigned long long m = __ballot(mine);
  if (lane == 0) wave_cnt[wave] = __popcll(m);
  __syncthreads();
  if (!mine) return;
  int pos = block_off[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) pos += wave_cnt[w];
  if (pos < max_watch) watch[pos] = bin;
}

struct FeedPeaksArgs {
  const float* avg;      // the batch's avg plane
  const int32_t* watch;  // [nwatch]
  const FeedDigestHeader* hdr;
  int32_t* peak_idx;     // [nframes][nwatch]
  float* peak_avg;
  int n, nframes, half;
};

// Grid-stride, one wave per (frame, watch key): window_peak of track_digest.h. The list's length is read from the header; a list that
// overflowed max_watch has no peaks (stf_result::status says so).
__global__ __launch_bounds__(256) void k_feed_peaks(const FeedPeaksArgs a) {
  const int lane = threadIdx.x & 63;
  const int nwatch = (a.hdr->flags & kFeedOverflow) ? 0 : a.hdr->nwatch;
  const long long items = (long long)a.nframes * nwatch;
  for (long long item = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); item < items; item += (long long)gridDim.x * 4) {
    const int f = (int)(item / nwatch), w = (int)(item % nwatch);
    const float* row = a.avg + (size_t)f * a.n;
    const int best = window_peak(row, a.n, a.half, a.watch[w], lane);
    if (lane == 0) {
      a.peak_idx[item] = best;
      a.peak_avg[item] = row[best];
    }
  }
}

}  // namespace ss
