// The host side of sc_process_ranges* (csrc/chan_ranges.h) alone, under the sanitizers: random range sets, valid ones and each
// kind of invalid one, against what the header promises.
//   validate(): accepts exactly the lists that a literal restatement of the rules accepts
//   plan():     every range exactly once; at most one range of a channel per round; a channel's ranges in the order given, one
//               per round from round 0 on without a gap
//   count_outputs(): range_counts sum to counts, and counts equal the cascade's output for the concatenation of the channel's
//               ranges (what a channel produces depends only on how many samples it saw), with the same counters after
// Prints "sets <n> valid <v> invalid <i> bad <b>"; exit status 0 only when bad == 0.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../rtl-sdr-scanner-cpp_amd/csrc/chan_ranges.h"

namespace cr = chan_ranges;

static bool literal_valid(const std::vector<sc_range>& rs, int channels, int nsamples) {
  if ((int)rs.size() > SC_MAX_RANGES) return false;
  for (size_t i = 0; i < rs.size(); ++i) {
    if (rs[i].channel < 0 || rs[i].channel >= channels) return false;
    if (rs[i].begin < 0 || rs[i].begin > rs[i].end || rs[i].end > nsamples) return false;
    for (size_t j = 0; j < i; ++j)
      if (rs[j].channel == rs[i].channel && rs[j].end > rs[i].begin) return false;
  }
  return true;
}

int main() {
  std::mt19937 rng(12345);
  auto uni = [&](int lo, int hi) { return (int)(rng() % (unsigned)(hi - lo + 1)) + lo; };
  const cr::Ratio cascades[][3] = {{{1, 64}}, {{1, 8}, {1, 16}}, {{2, 125}}, {{1, 16}, {5, 16}}, {{1, 75}}, {{3, 2}, {1, 7}, {5, 3}}};
  const int cascade_len[] = {1, 2, 1, 2, 1, 3};
  long long sets = 0, valid = 0, invalid = 0, bad = 0;
  int kinds[6] = {};
  for (int iter = 0; iter < 120000; ++iter) {
    const int channels = uni(1, SC_MAX_CHANNELS);
    const int nsamples = uni(0, 3) == 0 ? uni(0, 40) : uni(1, 300000);
    // a valid set: per channel ascending cuts, then the channels interleaved at random
    std::vector<std::vector<sc_range>> per((size_t)channels);
    int total = 0;
    for (int ch = 0; ch < channels; ++ch) {
      int n = uni(0, 3) == 0 ? 0 : uni(1, 6);
      if (total + n > SC_MAX_RANGES) n = SC_MAX_RANGES - total;
      total += n;
      std::vector<int> cuts;
      for (int k = 0; k < 2 * n; ++k) cuts.push_back(uni(0, nsamples));
      std::sort(cuts.begin(), cuts.end());
      for (int k = 0; k < n; ++k) {
        sc_range r{ch, uni(-500000, 500000), cuts[(size_t)(2 * k)], cuts[(size_t)(2 * k + 1)]};
        if (uni(0, 5) == 0) r.end = r.begin;                                        // empty
        if (k > 0 && uni(0, 3) == 0) r.begin = per[(size_t)ch].back().end;          // abutting
        per[(size_t)ch].push_back(r);
      }
    }
    std::vector<sc_range> rs;
    std::vector<size_t> next((size_t)channels, 0);
    for (int left = total; left > 0;) {
      const int ch = uni(0, channels - 1);
      if (next[(size_t)ch] < per[(size_t)ch].size()) {
        rs.push_back(per[(size_t)ch][next[(size_t)ch]++]);
        --left;
      }
    }
    // two in three stay valid; the rest get one defect of each kind in turn
    const int kind = iter % 3 == 0 ? 1 + (iter / 3) % 5 : 0;
    if (kind == 1 && !rs.empty()) rs[(size_t)uni(0, total - 1)].channel = uni(0, 1) ? channels : -1;
    if (kind == 2 && !rs.empty()) {
      sc_range& r = rs[(size_t)uni(0, total - 1)];
      r.begin = r.end + 1;
    }
    if (kind == 3 && !rs.empty()) rs[(size_t)uni(0, total - 1)].end = nsamples + uni(1, 5);
    if (kind == 4 && rs.size() >= 2) std::swap(rs[0], rs.back());  // may or may not break a channel's order
    if (kind == 5) {
      const sc_range filler{0, 0, nsamples, nsamples};
      while ((int)rs.size() <= SC_MAX_RANGES) rs.push_back(filler);
    }
    ++sets;
    const bool want = literal_valid(rs, channels, nsamples);
    const char* why = cr::validate(rs.data(), (int)rs.size(), channels, nsamples);
    if ((why == nullptr) != want) {
      ++bad;
      printf("iter %d kind %d: validate says %s, the rules say %s\n", iter, kind, why ? why : "ok", want ? "ok" : "invalid");
      continue;
    }
    if (!want) {
      ++invalid;
      ++kinds[kind];
      continue;
    }
    ++valid;
    const int n = (int)rs.size();
    cr::Plan p;
    cr::plan(rs.data(), n, &p);
    std::vector<int> times((size_t)n, 0), rounds_seen((size_t)channels, 0), last_index((size_t)channels, -1);
    bool ok = p.nrounds >= 0 && p.nrounds <= SC_MAX_RANGES && (p.nrounds == 0 || p.first[0] == 0) && p.first[p.nrounds] == n;
    for (int r = 0; ok && r < p.nrounds; ++r) {
      std::vector<int> in_round((size_t)channels, 0);
      ok = ok && p.first[r] < p.first[r + 1];
      for (int i = p.first[r]; ok && i < p.first[r + 1]; ++i) {
        const int idx = p.order[i];
        ok = ok && idx >= 0 && idx < n;
        if (!ok) break;
        const int ch = rs[(size_t)idx].channel;
        ++times[(size_t)idx];
        ok = ok && ++in_round[(size_t)ch] == 1;        // one range of a channel per round
        ok = ok && rounds_seen[(size_t)ch]++ == r;     // its r-th range in round r
        ok = ok && idx > last_index[(size_t)ch];       // in the order given
        last_index[(size_t)ch] = idx;
      }
    }
    for (int i = 0; ok && i < n; ++i) ok = times[(size_t)i] == 1;
    if (!ok) {
      ++bad;
      printf("iter %d: rounds wrong\n", iter);
      continue;
    }
    // counts
    const int which = uni(0, 5), nst = cascade_len[which];
    std::vector<cr::Counters> k0((size_t)channels);
    for (auto& k : k0)
      for (int s = 0; s < SC_MAX_STAGES; ++s) {
        k.ctr[s] = s < nst ? uni(0, cascades[which][s].interp - 1) : 0;
        k.skip[s] = s < nst ? uni(0, cascades[which][s].decim / cascades[which][s].interp + 1) : 0;
      }
    std::vector<cr::Counters> k = k0;
    std::vector<int32_t> counts((size_t)channels, -1), rc((size_t)n + 1, -1);
    cr::count_outputs(rs.data(), n, cascades[which], nst, k.data(), channels, counts.data(), rc.data());
    for (int ch = 0; ok && ch < channels; ++ch) {
      long long seen = 0, sum = 0;
      for (int i = 0; i < n; ++i)
        if (rs[(size_t)i].channel == ch) {
          seen += rs[(size_t)i].end - rs[(size_t)i].begin;
          sum += rc[(size_t)i];
          ok = ok && rc[(size_t)i] >= 0 && (rs[(size_t)i].begin != rs[(size_t)i].end || rc[(size_t)i] == 0);
        }
      cr::Counters whole = k0[(size_t)ch];
      const int want_count = cr::cascade_outputs(cascades[which], nst, &whole, (int)seen);
      ok = ok && sum == counts[(size_t)ch] && counts[(size_t)ch] == want_count;
      for (int s = 0; ok && s < nst; ++s) ok = whole.ctr[s] == k[(size_t)ch].ctr[s] && whole.skip[s] == k[(size_t)ch].skip[s];
    }
    if (!ok) {
      ++bad;
      printf("iter %d: counts wrong\n", iter);
    }
  }
  for (int kind = 1; kind <= 5; ++kind)
    if (kinds[kind] == 0) {
      ++bad;
      printf("no invalid set of kind %d was refused\n", kind);
    }
  printf("sets %lld valid %lld invalid %lld bad %lld\n", sets, valid, invalid, bad);
  return bad == 0 ? 0 : 1;
}
