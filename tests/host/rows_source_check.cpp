// rows_source_check.cpp — decide_rows_source (csrc/rows_source.h) without a GPU, as plain C++ under the sanitizers: every combination of
// dB plane / ring rows / fold order / log2 of the fold's radix against the table below, written out by hand from what the digests do
// (host_track.h: st_digest; host_track_feed.h: stf_enqueue). The last line is "rows_source_check: <n> combinations, bad <b>".
#include <cstdio>
#include <cstring>

#include "../../rtl-sdr-scanner-cpp_amd/csrc/rows_source.h"

namespace {

struct Row {
  bool plane, ring, perm8;
  int logq;
  ss::RowsSource source;
  int layout;
  const char* refusal_has;  // a word of the refusal, or null: none
};

// plane ring perm8 logq -> source, layout, refusal
const Row kTable[] = {
    // no plane, no rows: nothing to digest, whatever the order flags say
    {false, false, false, 0, ss::kRowsNone, 0, "no dB plane"},
    {false, false, false, 3, ss::kRowsNone, 0, "no dB plane"},
    {false, false, false, 4, ss::kRowsNone, 0, "no dB plane"},
    {false, false, true, 0, ss::kRowsNone, 0, "no dB plane"},
    {false, false, true, 3, ss::kRowsNone, 0, "no dB plane"},
    {false, false, true, 4, ss::kRowsNone, 0, "no dB plane"},
    // rows in the ring's buffer, bin order: the context's radix does not matter
    {false, true, false, 0, ss::kRowsRing, 0, nullptr},
    {false, true, false, 3, ss::kRowsRing, 0, nullptr},
    {false, true, false, 4, ss::kRowsRing, 0, nullptr},
    // ... in the fold's order: the radix names the tile; a radix no tile reads is refused
    {false, true, true, 0, ss::kRowsNone, 0, "radix"},
    {false, true, true, 3, ss::kRowsRing, 3, nullptr},
    {false, true, true, 4, ss::kRowsRing, 4, nullptr},
    // a dB plane wins: it is in bin order whatever else the call left
    {true, false, false, 0, ss::kRowsPlane, 0, nullptr},
    {true, false, false, 3, ss::kRowsPlane, 0, nullptr},
    {true, false, false, 4, ss::kRowsPlane, 0, nullptr},
    {true, false, true, 0, ss::kRowsPlane, 0, nullptr},
    {true, false, true, 3, ss::kRowsPlane, 0, nullptr},
    {true, false, true, 4, ss::kRowsPlane, 0, nullptr},
    {true, true, false, 0, ss::kRowsPlane, 0, nullptr},
    {true, true, false, 3, ss::kRowsPlane, 0, nullptr},
    {true, true, false, 4, ss::kRowsPlane, 0, nullptr},
    {true, true, true, 0, ss::kRowsPlane, 0, nullptr},
    {true, true, true, 3, ss::kRowsPlane, 0, nullptr},
    {true, true, true, 4, ss::kRowsPlane, 0, nullptr},
};

}  // namespace

int main() {
  long bad = 0, seen = 0;
  bool hit[2][2][2][3] = {};
  for (const Row& r : kTable) {
    const ss::RowsChoice c = ss::decide_rows_source(r.plane, r.ring, r.perm8, r.logq);
    const bool refusal_ok = r.refusal_has ? (c.refusal && strstr(c.refusal, r.refusal_has)) : c.refusal == nullptr;
    if (c.source != r.source || c.layout != r.layout || !refusal_ok) {
      ++bad;
      printf("FAILED plane %d ring %d perm8 %d logq %d: source %d layout %d refusal %s\n", r.plane, r.ring, r.perm8, r.logq, (int)c.source, c.layout, c.refusal ? c.refusal : "-");
    }
    hit[r.plane][r.ring][r.perm8][r.logq == 0 ? 0 : r.logq - 2] = true;
    ++seen;
  }
  for (int p = 0; p < 2; ++p)  // the table names every combination once
    for (int g = 0; g < 2; ++g)
      for (int o = 0; o < 2; ++o)
        for (int q = 0; q < 3; ++q)
          if (!hit[p][g][o][q]) ++bad;
  // a refusal never comes with a source, a source never with a refusal; layouts 3 and 4 only from ring rows in the fold's order
  for (int p = 0; p < 2; ++p)
    for (int g = 0; g < 2; ++g)
      for (int o = 0; o < 2; ++o)
        for (int logq = -1; logq <= 6; ++logq) {
          const ss::RowsChoice c = ss::decide_rows_source(p, g, o, logq);
          if ((c.source == ss::kRowsNone) != (c.refusal != nullptr)) ++bad;
          if (c.layout != 0 && !(c.source == ss::kRowsRing && o && c.layout == logq && (logq == 3 || logq == 4))) ++bad;
          ++seen;
        }
  printf("rows_source_check: %ld combinations, bad %ld\n", seen, bad);
  return bad ? 1 : 0;
}
