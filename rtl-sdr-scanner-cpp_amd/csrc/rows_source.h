// rows_source.h — where a digest finds the rows of the batch it digests, as plain C++ (no HIP include: the stand-alone check
// tests/host/rows_source_check.cpp compiles it with g++, as call_route_check.cpp compiles call_route.h). What a call left decides it:
//
//   a dB plane (ss_ctx::last_psd)                 kRowsPlane  the plane is in bin order whatever the ring's rows are in: RelRows,
//                                                             k_best_blocked / k_save_tail, and the replay is k_watch_tiles (layout 0)
//   no plane, rows in the averager ring's buffer  kRowsRing   RingRows, k_ring_best / k_ring_tail, and the replay is
//   (ss_ctx::last_rel_rows)                                   k_digest_tiles<layout>: 0 = rows in bin order, 3 / 4 = the radix-8 /
//                                                             radix-16 fold's blocked order (scan_step.h: step_detect_layout)
//   neither                                       kRowsNone   a refusal, with the words the digests have always used
//
// st_digest (host_track.h) and stf_enqueue (host_track_feed.h) both ask here, once per batch.
#pragma once

namespace ss {

enum RowsSource { kRowsNone = 0, kRowsPlane = 1, kRowsRing = 2 };

struct RowsChoice {
  RowsSource source;
  int layout;           // the replay's tile layout: 0, 3 or 4 (0 with kRowsPlane and kRowsNone)
  const char* refusal;  // kRowsNone: why; null otherwise
};

// db_plane: the call left a dB plane; ring_rows: it left its rows in the ring's buffer; perm8: those rows (and the window in front of
// them) are in the fold's blocked order; logq: log2 of the fold's radix on this context (3 or 4 where a fold exists, anything else
// where none does — perm8 is false there).
inline RowsChoice decide_rows_source(bool db_plane, bool ring_rows, bool perm8, int logq) {
  if (db_plane) return RowsChoice{kRowsPlane, 0, nullptr};
  if (!ring_rows) return RowsChoice{kRowsNone, 0, "the batch left no dB plane and no rows in the averager ring's buffer"};
  if (!perm8) return RowsChoice{kRowsRing, 0, nullptr};
  if (logq == 3 || logq == 4) return RowsChoice{kRowsRing, logq, nullptr};
  return RowsChoice{kRowsNone, 0, "the batch's rows are in a fold's order no replay tile reads (radix 8 and 16 only)"};
}

}  // namespace ss
