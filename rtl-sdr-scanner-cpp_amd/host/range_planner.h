// range_planner.h — which samples of a batch every recording slot records: SdrDevice::updateRecordings
// (sources/radio/sdr_device.cpp:82-144) walked over the per-frame lists of one batch after another, and its outcome as the
// sc_range list srf_record takes (include/specscan_record_feed.h). recorder.RangePlanner (recorder.py) restated in C++: the
// Python class is the oracle, tests/test_range_planner_host.py holds the two to the same plans.
//
// Per frame, in the reference's order: recorders whose shift is no longer in the list stop (:103-111); then the list is walked
// in order (:113-136) — the slot on that shift flushes if asked, else the first idle slot starts on it, else the shift is
// ignored ("no recorders available"); then the ignored set is pruned to what is still asked for. The frame's samples go to
// every slot that records. Slot state and the ignored set carry from batch to batch; a running recording goes on at sample 0
// of the next batch.
//
// Header-only C++17, no GPU: sc_range and the two limits are all it takes from the ABI.
#pragma once
#include <specscan_channelizer.h>

#include <algorithm>
#include <cstdint>
#include <limits>
#include <set>
#include <string>
#include <vector>

#include "signal_tracker.h"

namespace specscan {

enum class RangeEnd : uint8_t {
  Stop = 0,   // the recording ended: the reference drops what was not flushed (recorder.cpp:75-87)
  Batch = 1,  // the batch ended: the recording goes on at sample 0 of the next
};

struct RangePlan {
  std::vector<sc_range> ranges;  // samples of the batch, frame f being f * stride .. (f + 1) * stride; in the order they end
  std::vector<RangeEnd> ends;    // what closed ranges[i]
  std::vector<uint8_t> flushes;  // ranges[i] ends with a flush: the slot was asked to flush in the range's last frame
  void clear() {
    ranges.clear();
    ends.clear();
    flushes.clear();
  }
};

class RangePlanner {
 public:
  static constexpr int32_t IDLE = std::numeric_limits<int32_t>::max();  // Recorder::getShift while idle
  using Frame = std::vector<FrequencyFlush>;

  // slots: 1..SC_MAX_CHANNELS, stride: samples from one frame of the lists to the next, N * decim. valid() says whether both were.
  RangePlanner(int slots, int64_t stride) : m_stride(stride), m_slots(slots >= 1 && slots <= SC_MAX_CHANNELS && stride > 0 ? (size_t)slots : 0) {}

  bool valid() const { return !m_slots.empty(); }
  int slots() const { return (int)m_slots.size(); }
  int64_t stride() const { return m_stride; }
  bool recording(int slot) const { return m_slots[(size_t)slot].rec; }
  int32_t shift(int slot) const { return m_slots[(size_t)slot].shift; }
  const std::set<int32_t>& ignored() const { return m_ignored; }
  const std::string& error() const { return m_error; }

  // One batch: frames[f] is the tracker's list of frame f. false, with error() set and NOTHING changed (slots, ignored set), when
  // the plan holds more than SC_MAX_RANGES ranges — one srf_record does not take them — or the batch's samples do not fit
  // sc_range's int32_t: plan fewer frames at a time.
  bool plan(const Frame* frames, int nframes, RangePlan* out) {
    out->clear();
    m_error.clear();
    if (!valid()) return fail(out, "RangePlanner: slots not in 1..SC_MAX_CHANNELS or stride <= 0");
    if (nframes < 0 || (int64_t)nframes * m_stride > (int64_t)std::numeric_limits<int32_t>::max())
      return fail(out, "RangePlanner: the batch's samples do not fit int32_t: use a smaller batch");
    const std::vector<Slot> slots_before = m_slots;
    const std::set<int32_t> ignored_before = m_ignored;
    const size_t n = m_slots.size();
    std::vector<int64_t> begin(n, -1), flush_frame(n, -1);  // -1: no open range / never asked to flush in this batch
    for (size_t k = 0; k < n; ++k)
      if (m_slots[k].rec) begin[k] = 0;  // a recording that spans batches goes on at sample 0
    const auto close = [&](size_t k, int64_t at, RangeEnd why) {
      out->ranges.push_back(sc_range{(int32_t)k, m_slots[k].shift, (int32_t)begin[k], (int32_t)at});
      out->ends.push_back(why);
      out->flushes.push_back(at > 0 && flush_frame[k] == at / m_stride - 1 ? 1 : 0);
      begin[k] = -1;
    };
    for (int f = 0; f < nframes; ++f) {
      const Frame& want = frames[f];
      const int64_t at = (int64_t)f * m_stride;
      const auto waiting = [&](int32_t shift) {
        return std::find_if(want.begin(), want.end(), [shift](const FrequencyFlush& x) { return x.shift_hz == shift; }) != want.end();
      };
      for (size_t k = 0; k < n; ++k) {  // sdr_device.cpp:103-111
        if (m_slots[k].rec && !waiting(m_slots[k].shift)) {
          close(k, at, RangeEnd::Stop);
          m_slots[k] = Slot{};
          flush_frame[k] = -1;
        }
      }
      for (const FrequencyFlush& x : want) {  // sdr_device.cpp:113-136
        const auto hit = std::find_if(m_slots.begin(), m_slots.end(), [&](const Slot& s) { return s.shift == x.shift_hz; });
        if (hit != m_slots.end()) {
          if (x.flush) flush_frame[(size_t)(hit - m_slots.begin())] = f;
          continue;
        }
        const auto idle = std::find_if(m_slots.begin(), m_slots.end(), [](const Slot& s) { return !s.rec; });
        if (idle != m_slots.end()) {
          *idle = Slot{true, x.shift_hz};
          begin[(size_t)(idle - m_slots.begin())] = at;
        } else {
          m_ignored.insert(x.shift_hz);  // "no recorders available"
        }
      }
      for (auto it = m_ignored.begin(); it != m_ignored.end();) it = waiting(*it) ? std::next(it) : m_ignored.erase(it);
    }
    for (size_t k = 0; k < n; ++k)
      if (begin[k] >= 0) close(k, (int64_t)nframes * m_stride, RangeEnd::Batch);
    if (out->ranges.size() > (size_t)SC_MAX_RANGES) {
      m_slots = slots_before;
      m_ignored = ignored_before;
      return fail(out, "RangePlanner: " + std::to_string(out->ranges.size()) + " ranges in one batch, more than SC_MAX_RANGES (" +
                           std::to_string(SC_MAX_RANGES) + "): use a smaller batch");
    }
    return true;
  }
  bool plan(const std::vector<Frame>& frames, RangePlan* out) { return plan(frames.data(), (int)frames.size(), out); }

 private:
  struct Slot {
    bool rec = false;
    int32_t shift = IDLE;
  };
  bool fail(RangePlan* out, const std::string& why) {
    out->clear();
    m_error = why;
    return false;
  }
  const int64_t m_stride;
  std::vector<Slot> m_slots;
  std::set<int32_t> m_ignored;
  std::string m_error;
};

}  // namespace specscan

extern "C" {
// C binding (libspecscan_host.so, host/recording_host.cpp). Handles are opaque; arrays are caller-owned.
void* srp_create(int32_t slots, int64_t stride);
void srp_destroy(void* planner);
const char* srp_last_error(const void* planner);
int32_t srp_plan(void* planner, int32_t nframes, const int32_t* frame_off, const int32_t* shifts, const uint8_t* flush, sc_range* ranges,
                 int32_t* ends, int32_t* flushes);
int32_t srp_slots(const void* planner, int32_t* shifts, int32_t* recording);
int32_t srp_ignored(const void* planner, int32_t* out, int32_t cap);
}
