// Stand-alone check of csrc/spectrogram_gate.h (no HIP, no GPU): built with -fsanitize=address,undefined and run on the CPU by
// tests/test_spectrogram_feed.py. The gate is compared with a restatement of Spectrogram::work / send (spectrogram.cpp:29-75) that
// walks one frame at a time: random clocks, a step onto last + 1000 exactly (no row) and onto last + 1001 (row), a clock that steps
// backwards, the first-frame stamp, two centres alternating with a gate each, and cap smaller than the count.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <vector>

#include "../../rtl-sdr-scanner-cpp_amd/csrc/spectrogram_gate.h"

namespace {

// the restatement: one container per centre, created at its first frame with that frame's time
struct Restated {
  std::map<int, int64_t> last;
  bool frame(int centre, int64_t now) {
    auto it = last.find(centre);
    if (it == last.end()) it = last.emplace(centre, now).first;
    if (it->second + 1000 < now) {
      it->second = now;
      return true;
    }
    return false;
  }
};

struct Gate {
  int64_t last_send = 0;
  int32_t have_last = 0;
};

int failures = 0;

// the stream cut into batches of the given sizes (cycled); the centre alternates per batch between `centres` values
void run(const char* name, const std::vector<int64_t>& t, const std::vector<int>& sizes, int centres, int cap) {
  Restated want;
  std::map<int, Gate> gates;
  size_t at = 0, b = 0;
  long rows = 0;
  while (at < t.size()) {
    const size_t n = std::min(t.size() - at, (size_t)sizes[b % sizes.size()]);
    const int centre = (int)(b % (size_t)centres);
    std::vector<int32_t> expect;
    for (size_t f = 0; f < n; ++f)
      if (want.frame(centre, t[at + f])) expect.push_back((int32_t)f);
    Gate& g = gates[centre];
    std::vector<int32_t> cut((size_t)cap + 1, -7);  // one guard word behind cap
    const int32_t got = ss::spectrogram_gate_plan(&g.last_send, &g.have_last, t.data() + at, (int32_t)n, cap > 0 ? cut.data() : nullptr, cap);
    bool ok = got == (int32_t)expect.size() && cut[(size_t)cap] == -7 && g.have_last == 1 && g.last_send == want.last[centre];
    for (size_t k = 0; ok && k < expect.size() && k < (size_t)cap; ++k) ok = cut[k] == expect[k];
    for (size_t k = expect.size(); ok && k < (size_t)cap; ++k) ok = cut[k] == -7;  // nothing written past the count
    if (!ok) {
      printf("FAIL %s: batch %zu (frames %zu..%zu, centre %d): %d rows, expected %zu\n", name, b, at, at + n, centre, got, expect.size());
      ++failures;
      return;
    }
    rows += got;
    at += n;
    ++b;
  }
  printf("ok %s: %zu frames, %zu batches, %ld rows\n", name, t.size(), b, rows);
}

}  // namespace

int main() {
  std::mt19937_64 rng(7);
  {  // random, mostly forward clocks in several cuttings
    std::vector<int64_t> t;
    int64_t now = 5000;
    for (int k = 0; k < 4000; ++k) t.push_back(now += (int64_t)(rng() % 400));
    run("random/one", t, {4000}, 1, 64);
    run("random/mixed", t, {1, 64, 7, 300, 2}, 1, 64);
    run("random/two centres", t, {33, 5, 64}, 2, 64);
    run("random/cap 1", t, {500}, 1, 1);
    run("random/cap 0", t, {500}, 1, 0);
  }
  {  // exactly last + 1000: no row; last + 1001: row. The first frame stamps (no row at frame 0 whatever its time).
    std::vector<int64_t> t = {777777, 778777, 778778, 779778, 779779, 779779, 780780};
    run("edge/1000 and 1001", t, {7}, 1, 8);
    run("edge/1000 and 1001 by frame", t, {1}, 1, 8);
    Gate g;
    int32_t cut[8];
    const int32_t n = ss::spectrogram_gate_plan(&g.last_send, &g.have_last, t.data(), (int32_t)t.size(), cut, 8);
    if (n != 3 || cut[0] != 2 || cut[1] != 4 || cut[2] != 6 || g.last_send != 780780) {
      printf("FAIL edge: %d rows at %d %d %d\n", n, cut[0], cut[1], cut[2]);
      ++failures;
    }
  }
  {  // a clock that steps backwards: the comparison is against the last send, not the previous frame
    std::vector<int64_t> t;
    int64_t now = 100000;
    for (int k = 0; k < 3000; ++k) {
      now += (int64_t)(rng() % 700) - 200;
      if (k % 500 == 250) now -= 5000;
      t.push_back(now);
    }
    run("backwards/one", t, {3000}, 1, 64);
    run("backwards/mixed, two centres", t, {40, 1, 64, 9}, 2, 64);
    run("negative times", std::vector<int64_t>{-5000, -4001, -3999, -2000, 0, 1001}, {6}, 1, 8);
  }
  if (failures) return 1;
  printf("all ok\n");
  return 0;
}
