// The window -> tile-column arithmetic of csrc/track_sparse.h (watch_col_range, what k_feed_watch_cols marks and k_watch_tiles then
// evaluates) on the host, against a loop over the bins of the window k_feed_peaks reads, [max(0, key - half), min(n - 1, key + half)]:
// a column is marked iff the window holds one of its 256 bins. Then whole random watch lists: the marked set, formed as the kernel
// forms it (flags cleared, every key's range set), against the union of the bins' columns. The flags live in a vector of exactly
// n / 256 entries, so that the address sanitizer sees a column outside the row.
// Plain C++ (g++ -fsanitize=address,undefined), no HIP. Prints "... bad 0" when everything holds.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../rtl-sdr-scanner-cpp_amd/csrc/track_sparse.h"

static long long g_bad = 0, g_windows = 0, g_lists = 0;

static void brute(int key, int half, int n, std::vector<uint8_t>& cols) {
  const int lo = std::max(0, key - half), hi = std::min(n - 1, key + half);
  for (int b = lo; b <= hi; ++b) cols[(size_t)(b / 256)] = 1;
}

static void check_key(int key, int half, int n) {
  const int ncols = n / 256;
  std::vector<uint8_t> want((size_t)ncols, 0), got((size_t)ncols, 0);
  brute(key, half, n, want);
  const ss::WatchColRange r = ss::watch_col_range(key, half, n);
  if (r.lo < 0 || r.hi >= ncols || r.lo > r.hi) {
    if (g_bad++ < 20) printf("RANGE n %d half %d key %d: [%d, %d]\n", n, half, key, r.lo, r.hi);
    return;
  }
  for (int c = r.lo; c <= r.hi; ++c) got[(size_t)c] = 1;
  ++g_windows;
  if (got != want && g_bad++ < 20) printf("MISMATCH n %d half %d key %d: [%d, %d]\n", n, half, key, r.lo, r.hi);
}

int main() {
  std::mt19937 rng(20240607);
  const int sizes[] = {256, 1024, 8192, 32768};
  const int halves[] = {0, 1, 20, 64, 127, 128, 1024, 3260};
  for (int n : sizes)
    for (int half : halves) {
      const int fixed[] = {0, 1, 255, 256, 257, n / 2, n - 257, n - 256, n - 1};
      for (int key : fixed)
        if (key >= 0 && key < n) check_key(key, half, n);
      std::uniform_int_distribution<int> any(0, n - 1);
      for (int k = 0; k < 300; ++k) check_key(any(rng), half, n);
      // whole lists, as k_feed_watch_cols forms the flags
      for (int trial = 0; trial < 20; ++trial) {
        const int ncols = n / 256, nkeys = (int)(rng() % 40);
        std::vector<uint8_t> want((size_t)ncols, 0);
        std::vector<int32_t> flag((size_t)ncols, -1);
        for (int c = 0; c < ncols; ++c) flag[(size_t)c] = 0;
        for (int k = 0; k < nkeys; ++k) {
          const int key = any(rng);
          brute(key, half, n, want);
          const ss::WatchColRange r = ss::watch_col_range(key, half, n);
          for (int c = r.lo; c <= r.hi; ++c) flag[(size_t)c] = 1;
        }
        ++g_lists;
        for (int c = 0; c < ncols; ++c)
          if (flag[(size_t)c] != (int32_t)want[(size_t)c] && g_bad++ < 20) printf("LIST n %d half %d trial %d column %d: %d want %d\n", n, half, trial, c, flag[(size_t)c], want[(size_t)c]);
      }
    }
  printf("watch_cols_check: %lld windows, %lld lists, bad %lld\n", g_windows, g_lists, g_bad);
  return g_bad == 0 ? 0 : 1;
}
