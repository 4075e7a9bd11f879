// feed_recorder.h — recording behind the pipelined feed, above the C ABI: an srf_ctx on a given ss_feed
// (include/specscan_record_feed.h), a RangePlanner (host/range_planner.h) and a RecordingStore (host/recording_store.h). After
// every collect of the feed (ss_feed_collect or stf_collect, which leave the batch held) ONE call takes the batch's per-frame
// tracker lists, plans them, records the planned sample ranges from the feed's own upload and publishes what the flushes release:
// no second upload, and at decim != 1 (a whole-item feed) only the recorded ranges cross PCIe. A batch that records nothing is
// let go with srf_release and uploads nothing.
//
// This is the replay route (host/replay_main.cpp --record-out). RecorderBank (host/recorder_bank.h), the live adapter's route —
// sc_process on the whole stream after a second upload — is a separate class and is not wired to the feed.
// Header-only C++17; links libspecscan.so. One thread records.
#pragma once
#include <specscan.h>
#include <specscan_record_feed.h>

#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "range_planner.h"
#include "recording_store.h"

namespace specscan {

class FeedRecorder {
 public:
  struct Counters {
    uint64_t ranges = 0;         // ranges recorded
    uint64_t samples = 0;        // input samples recorded: the ranges' lengths, summed
    uint64_t h2d_bytes = 0;      // srf_result.h2d_bytes, summed
    uint64_t ignored_max = 0;    // the largest ignored set a batch left behind ("no recorders available")
  };

  // stride = N * decim of the scan context behind the feed; center_frequency its centre. Throws when srf_create refuses.
  FeedRecorder(ss_feed* feed, int32_t bandwidth, int recorders, int64_t stride, int32_t center_frequency, RecordingStore::Publish publish)
      : m_planner(recorders, stride), m_store(recorders, center_frequency, bandwidth, stride, std::move(publish)) {
    srf_config cfg{SRF_ABI_VERSION, bandwidth, 125, recorders, 127.0f, 0};  // RESAMPLER_THRESHOLD, complex_to_interleaved_char's scale
    if (srf_create(feed, &cfg, &m_ctx) != SS_OK) throw std::runtime_error(std::string("srf_create: ") + srf_last_error(nullptr));
  }
  ~FeedRecorder() { srf_destroy(m_ctx); }
  FeedRecorder(const FeedRecorder&) = delete;
  FeedRecorder& operator=(const FeedRecorder&) = delete;

  const RangePlanner& planner() const { return m_planner; }
  const RecordingStore& store() const { return m_store; }
  const Counters& counters() const { return m_counters; }
  uint64_t publishedItems() const { return m_store.published(); }
  uint64_t droppedItems() const { return m_store.dropped(); }
  const std::string& error() const { return m_error; }

  // The batch collected last: frames[f] is the tracker's list of its frame f, first_frame the frame's absolute index in the stream.
  // false with error(): a plan over SC_MAX_RANGES is refused BEFORE srf_record — the batch stays held and nothing has changed, but
  // srf_record lets the batch go after one call, so its frames cannot be recorded in two: use a smaller batch.
  bool record(const std::vector<RangePlanner::Frame>& frames, int64_t first_frame, const RecordingStore::FrameTime& frame_time) {
    if (!m_planner.plan(frames, &m_plan)) return fail(m_planner.error());
    if (m_planner.ignored().size() > m_counters.ignored_max) m_counters.ignored_max = m_planner.ignored().size();
    const int nranges = (int)m_plan.ranges.size();
    if (nranges == 0) {
      if (srf_release(m_ctx) != SS_OK) return fail(std::string("srf_release: ") + srf_last_error(m_ctx));
      return true;
    }
    srf_result r;
    if (srf_record(m_ctx, m_plan.ranges.data(), nranges, &r) != SS_OK) return fail(std::string("srf_record: ") + srf_last_error(m_ctx));
    m_counters.h2d_bytes += r.h2d_bytes;
    int64_t used[SC_MAX_CHANNELS] = {0};  // a channel's outputs lie in its plane in the order of its ranges
    for (int i = 0; i < nranges; ++i) {
      const sc_range& g = m_plan.ranges[(size_t)i];
      const int64_t count = r.range_counts[i];
      if (used[g.channel] + count > (int64_t)r.cap) return fail("srf_record: a channel's outputs exceed the plane's capacity");
      const int8_t* iq = r.out_i8 + ((size_t)g.channel * (size_t)r.cap + (size_t)used[g.channel]) * 2;
      used[g.channel] += count;
      if (!m_store.feed(g, m_plan.ends[(size_t)i], m_plan.flushes[(size_t)i] != 0, iq, count, first_frame, frame_time)) return fail("RecordingStore: bad range");
      ++m_counters.ranges;
      m_counters.samples += (uint64_t)(g.end - g.begin);
    }
    return true;
  }

  // End of the stream: open recordings are dropped like a stop.
  void finish() { m_store.finish(); }

 private:
  bool fail(const std::string& why) {
    m_error = why;
    return false;
  }
  srf_ctx* m_ctx = nullptr;
  RangePlanner m_planner;
  RecordingStore m_store;
  RangePlan m_plan;
  Counters m_counters;
  std::string m_error;
};

}  // namespace specscan
