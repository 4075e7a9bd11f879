// The ring-row cell address of csrc/track_digest_sparse.h (ring_cell, ring_bin_offset, ring_db_range: where k_ring_best and k_ring_tail
// find a rel value of a batch whose call left no dB plane, and what they do with it) on the host, against a restatement that walks a row
// position by position. A fold row of 8192 Q bins (Q = 1 << logq) is laid out block by block: block j holds the 32 Q bins
// [32 Q j, 32 Q (j + 1)), residue g's 32 values side by side at [32 g, 32 g + 32) of the block, value m of them being bin Q (32 j + m) + g.
// The check fills a batch of rows that way (every cell a value that names its frame and bin), reads every bin of every row back through
// ring_cell as rel_at does, and compares with the value the host's ss_read_window would give: learning frames among dB rows SS_NO_DATA,
// dB rows minus the ceiling, settled rows as stored. The rows live in a vector of exactly nframes x n floats, so that the address
// sanitizer sees a cell outside them.
// Plain C++ (g++ -fsanitize=address,undefined), no HIP. Prints "... bad 0" when everything holds.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../rtl-sdr-scanner-cpp_amd/csrc/track_digest_sparse.h"

static long long g_bad = 0, g_cells = 0, g_rows = 0;

static float cell_value(int frame, int bin) { return (float)(frame * 7 + 1) + (float)bin * 0.25f; }  // exact in fp32 for the sizes here
static float thr_value(int bin) { return 3.0f + (float)(bin % 97) * 0.5f; }

// a batch of rows as the call's form writes them: position by position, never through ring_bin_offset
static void fill_rows(std::vector<float>& rows, int n, int nframes, int logq) {
  for (int f = 0; f < nframes; ++f) {
    float* row = rows.data() + (size_t)f * (size_t)n;
    if (logq == 0) {
      for (int b = 0; b < n; ++b) row[b] = cell_value(f, b);
      continue;
    }
    const int Q = 1 << logq, block = 32 * Q;
    int pos = 0;
    for (int j = 0; j < n / block; ++j)
      for (int g = 0; g < Q; ++g)
        for (int m = 0; m < 32; ++m) row[pos++] = cell_value(f, Q * (32 * j + m) + g);
  }
}

// db: the call left dB values; [settled_a, settled_b): batch frames settled since
static void check_batch(int n, int logq, int nframes, int n_learn, bool db, long long settled_a, long long settled_b) {
  std::vector<float> rows((size_t)n * (size_t)nframes), thr((size_t)n);
  fill_rows(rows, n, nframes, logq);
  for (int b = 0; b < n; ++b) thr[(size_t)b] = thr_value(b);
  const ss::RingDbRange range = ss::ring_db_range(nframes, db, settled_a, settled_b);
  for (int f = 0; f < nframes; ++f) {
    const bool settled = f >= settled_a && f < settled_b;
    ++g_rows;
    for (int b = 0; b < n; ++b) {
      const ss::RingCell c = ss::ring_cell(n, n_learn, logq, range.from, range.to, f, b);
      if (c.at >= rows.size()) {
        if (g_bad++ < 20) printf("OUTSIDE n %d logq %d frame %d bin %d: %zu\n", n, logq, f, b, c.at);
        continue;
      }
      const float x = rows[c.at];
      const float got = c.kind == ss::kRingNoData ? -100.0f : c.kind == ss::kRingMinusThr ? x - thr[(size_t)b] : x;
      const float want = !db || settled ? cell_value(f, b) : f < n_learn ? -100.0f : cell_value(f, b) - thr_value(b);
      ++g_cells;
      if (got != want && g_bad++ < 20) printf("MISMATCH n %d logq %d frame %d bin %d (db %d settled %d learn %d): %g want %g\n", n, logq, f, b, (int)db, (int)settled, n_learn, got, want);
    }
  }
}

int main() {
  const struct {
    int n, logq;
  } shapes[] = {{65536, 3}, {131072, 4}, {65536, 0}, {8192, 0}, {1 << 20, 0}};
  for (const auto& s : shapes) {
    const int nframes = s.n >= (1 << 20) ? 2 : 5;
    check_batch(s.n, s.logq, nframes, 0, true, 0, 0);              // dB rows, no learning frame
    check_batch(s.n, s.logq, nframes, 2, true, 0, 0);              // ... the first two learn
    check_batch(s.n, s.logq, nframes, 0, false, 0, 0);             // rel rows as stored
    check_batch(s.n, s.logq, nframes, 2, false, 0, 0);             // ... learning frames are whatever was stored
    check_batch(s.n, s.logq, nframes, 0, true, nframes - 1, nframes);  // the newest row settled since
    check_batch(s.n, s.logq, nframes, 1, true, -30, nframes);      // every row settled (the whole window was)
    check_batch(s.n, s.logq, nframes, 0, true, -30, 1);            // the window's rows in front of the batch and the batch's first
    check_batch(s.n, s.logq, nframes, 0, true, -30, -2);           // rows in front of the batch only: none of its own
  }
  printf("ring_rows_check: %lld rows, %lld cells, bad %lld\n", g_rows, g_cells, g_bad);
  return g_bad == 0 ? 0 : 1;
}
