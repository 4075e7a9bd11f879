// spectrogram_gate.h — the reference's per-frame send gate (Spectrogram::send, sources/radio/blocks/spectrogram.cpp:62-75) for one
// centre frequency's container over one batch of frame times. Plain C++, no HIP: sgf_gate_plan (include/specscan_spectrogram_feed.h)
// is this function, and a stand-alone host program can include it (tests/host/spectrogram_gate_check.cpp).
//
//   * the container's first frame stamps last_send (Container's constructor takes getTime(), spectrogram.cpp:9,36);
//   * Spectrogram::work sends after every frame: a row closes at frame f iff last_send + 1000 < t_ms[f], strictly (:65), and then
//     last_send = t_ms[f] (:73);
//   * the clock is whatever the caller hands in: nothing here assumes that it is monotonic.
#pragma once
#include <cstdint>

namespace ss {

constexpr int64_t kSpectrogramSendIntervalMs = 1000;  // SPECTROGRAM_SEND_INTERVAL

// Returns the number of rows the batch closes and writes the first min(that, cap) closing frames to cut_frame (nullable when cap
// is 0). last_send / have_last are the container's gate, read and updated.
inline int32_t spectrogram_gate_plan(int64_t* last_send, int32_t* have_last, const int64_t* t_ms, int32_t nframes, int32_t* cut_frame, int32_t cap) {
  int32_t rows = 0;
  for (int32_t f = 0; f < nframes; ++f) {
    const int64_t now = t_ms[f];
    if (!*have_last) {
      *last_send = now;
      *have_last = 1;
    }
    if (*last_send + kSpectrogramSendIntervalMs < now) {
      if (cut_frame && rows < cap) cut_frame[rows] = f;
      ++rows;
      *last_send = now;
    }
  }
  return rows;
}

}  // namespace ss
