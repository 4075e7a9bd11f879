// chan_ranges.h — host side of sc_process_ranges* (include/specscan_channelizer.h): validation of a call's sc_range list,
// its split into rounds, and the resampler counters that give every range's output count. Plain C++, no HIP: channelizer.hip
// includes it, and tests/host/chan_ranges_check.cpp drives it alone under the sanitizers.
//
// A call is defined as, per channel and in the order given, sc_start(shift) / sc_process of [begin, end) / sc_stop. One launch
// gives a slot one contiguous range (an address offset), so the call is cut into rounds: round r holds the r-th range of every
// channel that has one. Within a round the slots are independent, and rounds run in stream order, so every channel sees
// its ranges in the order given.
#ifndef SPECSCAN_CHAN_RANGES_H
#define SPECSCAN_CHAN_RANGES_H

#include <stdint.h>

#include "../../include/specscan_channelizer.h"

namespace chan_ranges {

// outputs of one resampler for n_in new samples given its (ctr, skip), and the state after them
inline int stage_outputs(int interp, int decim, int ctr, int skip, int n_in, int* ctr_after, int* skip_after) {
  long long nout = 0;
  if (n_in > skip) {
    const long long need = (long long)(n_in - skip) * interp - ctr;  // smallest m with ctr + m*D >= (n_in - skip) * I
    nout = need <= 0 ? 0 : (need + decim - 1) / decim;
  }
  const long long total = (long long)ctr + nout * decim;
  *ctr_after = (int)(total % interp);
  *skip_after = (int)((long long)skip + total / interp - n_in);
  return (int)nout;
}

struct Ratio {
  int interp, decim;
};

// every resampler's polyphase counter and the input samples to pass before its next output, for one slot
struct Counters {
  int ctr[SC_MAX_STAGES];
  int skip[SC_MAX_STAGES];
};

// n_in samples through the cascade: the last stage's output count; the counters advance
inline int cascade_outputs(const Ratio* stages, int nstages, Counters* k, int n_in) {
  int n = n_in;
  for (int s = 0; s < nstages; ++s) n = stage_outputs(stages[s].interp, stages[s].decim, k->ctr[s], k->skip[s], n, &k->ctr[s], &k->skip[s]);
  return n;
}

// What is wrong with the list, or nullptr. Nothing else is looked at before this has passed.
inline const char* validate(const sc_range* ranges, int nranges, int channels, int nsamples) {
  if (nranges < 0 || nranges > SC_MAX_RANGES) return "nranges not in 0..SC_MAX_RANGES";
  if (nranges > 0 && !ranges) return "null ranges";
  int last_end[SC_MAX_CHANNELS];
  for (int ch = 0; ch < SC_MAX_CHANNELS; ++ch) last_end[ch] = 0;
  for (int i = 0; i < nranges; ++i) {
    const sc_range& r = ranges[i];
    if (r.channel < 0 || r.channel >= channels) return "range channel out of range";
    if (r.begin < 0 || r.begin > r.end) return "range with begin < 0 or begin > end";
    if (r.end > nsamples) return "range ends beyond nsamples";
    if (r.begin < last_end[r.channel]) return "ranges of one channel overlap or descend";
    last_end[r.channel] = r.end;
  }
  return nullptr;
}

struct Plan {
  int nrounds;
  int first[SC_MAX_RANGES + 1];  // round r is order[first[r] .. first[r + 1])
  int order[SC_MAX_RANGES];      // indices into the call's list; inside a round in the order given
};

// Round r = the r-th range of every channel that has one. The list must have passed validate().
inline void plan(const sc_range* ranges, int nranges, Plan* p) {
  int seen[SC_MAX_CHANNELS];
  int round_of[SC_MAX_RANGES];
  for (int ch = 0; ch < SC_MAX_CHANNELS; ++ch) seen[ch] = 0;
  p->nrounds = 0;
  for (int i = 0; i < nranges; ++i) {
    round_of[i] = seen[ranges[i].channel]++;
    if (round_of[i] + 1 > p->nrounds) p->nrounds = round_of[i] + 1;
  }
  int n = 0;
  for (int r = 0; r < p->nrounds; ++r) {
    p->first[r] = n;
    for (int i = 0; i < nranges; ++i)
      if (round_of[i] == r) p->order[n++] = i;
  }
  p->first[p->nrounds] = n;
}

// range_counts[i] and counts[channel] of the call, from each channel's counters (k[channel], advanced as the call advances
// them). counts gets all `channels` entries, zero for a channel without ranges.
inline void count_outputs(const sc_range* ranges, int nranges, const Ratio* stages, int nstages, Counters* k, int channels, int32_t* counts,
                          int32_t* range_counts) {
  for (int ch = 0; ch < channels; ++ch) counts[ch] = 0;
  for (int i = 0; i < nranges; ++i) {  // a channel's ranges are in its order already
    const int n = cascade_outputs(stages, nstages, &k[ranges[i].channel], ranges[i].end - ranges[i].begin);
    range_counts[i] = n;
    counts[ranges[i].channel] += n;
  }
}

// sc_process_ranges_upload: the parts of the call's stream that its ranges read, as intervals [begin, end) to copy. The
// non-empty ranges sorted by begin, overlapping and abutting ones merged: at most nranges intervals, ascending, with a gap
// between any two. The list must have passed validate().
struct Interval {
  int begin, end;
};

inline int upload_intervals(const sc_range* ranges, int nranges, Interval* out) {
  int n = 0;
  for (int i = 0; i < nranges; ++i) {  // insertion sort: SC_MAX_RANGES at most, and a channel's ranges ascend already
    if (ranges[i].begin == ranges[i].end) continue;
    int at = n++;
    for (; at > 0 && out[at - 1].begin > ranges[i].begin; --at) out[at] = out[at - 1];
    out[at].begin = ranges[i].begin;
    out[at].end = ranges[i].end;
  }
  int m = 0;
  for (int i = 0; i < n; ++i) {
    if (m > 0 && out[i].begin <= out[m - 1].end) {
      if (out[i].end > out[m - 1].end) out[m - 1].end = out[i].end;
    } else {
      out[m++] = out[i];
    }
  }
  return m;
}

// samples of the largest batch of whole items, max_batch * n * decim; false when that does not fit a call's int32_t nsamples
inline bool item_samples(int max_batch, int n, int decim, int32_t* out) {
  if (max_batch < 0 || n < 0 || decim < 0) return false;
  const unsigned long long frames = (unsigned long long)max_batch * (unsigned long long)n;  // < 2^62
  if (frames > 0x7fffffffULL) return false;
  const unsigned long long total = frames * (unsigned long long)decim;  // < 2^62
  if (total > 0x7fffffffULL) return false;
  *out = (int32_t)total;
  return true;
}

}  // namespace chan_ranges

#endif  // SPECSCAN_CHAN_RANGES_H
