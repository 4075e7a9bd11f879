// recording_store.h — what the reference's Recorder keeps on the host, fed with the outputs of planned sample ranges
// (host/range_planner.h, srf_record) instead of work() calls: what RecorderBank's Slot (host/recorder_bank.h) does with the int8
// outputs, restated for ranges.
//   stream_to_vector + Buffer        sources/radio/recorder.cpp:35-39, sources/radio/blocks/buffer.h:16-58
//   Recorder::flush / stopRecording  recorder.cpp:75-98
// Per slot: `pending`, less than one item — what sits inside stream_to_vector; it survives stop and start, as in the reference —
// and `items` with `item_times`, the Buffer, cleared by a stop. An item is itemSamples = roundUp(bandwidth * 100 / 1000, 4096)
// int8 (re,im) samples (recorder.cpp:35, config.h:19).
//
// A range that ends with a flush publishes every gathered item of its slot, in order; a range closed by a stop then drops what is
// left in `items`. finish() — the end of the stream — drops open recordings like a stop (the reference's destructor calls
// stopRecording).
//
// Item time: the stream's own clock. The reference stamps an item with the wall clock of the work() call that completed it; here the
// samples of a whole batch arrive at once, so an item gets the time of the frame that held the input sample which completed it,
// by proportion: the item completed by output number q (1-based, counted within the range's `count` outputs) of a range
// [begin, end) is given the frame holding sample
//     p = begin + ceil(q * (end - begin) / count) - 1        (64-bit, clamped into [begin, end - 1])
// of the batch, i.e. the time frame_time(first_frame + p / stride), first_frame being the batch's first absolute frame index and
// stride = N * decim the samples from one frame to the next.
//
// Header-only C++17, no GPU.
#pragma once
#include <specscan_channelizer.h>

#include <cstdint>
#include <functional>
#include <utility>
#include <vector>

#include "range_planner.h"

namespace specscan {

class RecordingStore {
 public:
  // RecorderBank::Publish: time of the item (ms), centre frequency of the recording (device centre + shift), sample rate of the
  // recording, int8 (re,im) samples, their count — DataController::pushTransmission(time, frequency, sampleRate, data, size)
  using Publish = std::function<void(int64_t time_ms, int32_t frequency, int32_t sample_rate, const int8_t* iq, int nsamples)>;
  using FrameTime = std::function<int64_t(int64_t frame)>;  // absolute frame index -> ms

  RecordingStore(int slots, int32_t center_frequency, int32_t bandwidth, int64_t stride, Publish publish)
      : m_center(center_frequency), m_bandwidth(bandwidth), m_stride(stride > 0 ? stride : 1), m_publish(std::move(publish)),
        m_slots(slots >= 1 && slots <= SC_MAX_CHANNELS ? (size_t)slots : 0) {
    const int64_t raw = (int64_t)bandwidth * 100 / 1000;  // roundUp(recordingBandwidth * RECORDER_FLUSH_INTERVAL / 1000, 4096)
    m_itemSamples = raw <= 0 ? 4096 : (int)(raw % 4096 == 0 ? raw : (raw / 4096 + 1) * 4096);
  }

  int slots() const { return (int)m_slots.size(); }
  int itemSamples() const { return m_itemSamples; }
  int pendingSamples(int slot) const { return (int)(m_slots[(size_t)slot].pending.size() / 2); }
  int heldItems(int slot) const { return (int)m_slots[(size_t)slot].item_times.size(); }
  uint64_t published() const { return m_published; }
  uint64_t dropped() const { return m_dropped; }

  // One range of a plan with its outputs: iq = count int8 (re,im) samples, the slice of the channel's plane that
  // srf_result.range_counts gives ranges[i]. false for a channel the store does not have.
  bool feed(const sc_range& r, RangeEnd why, bool flush, const int8_t* iq, int64_t count, int64_t first_frame, const FrameTime& frame_time) {
    if (r.channel < 0 || (size_t)r.channel >= m_slots.size() || count < 0) return false;
    Slot& s = m_slots[(size_t)r.channel];
    const int64_t len = (int64_t)r.end - (int64_t)r.begin, item = m_itemSamples;
    int64_t done = 0;  // outputs of this range already taken
    while (done < count) {
      const int64_t have = (int64_t)(s.pending.size() / 2), take = std::min(item - have, count - done);
      s.pending.insert(s.pending.end(), iq + 2 * done, iq + 2 * (done + take));
      done += take;
      if (have + take < item) break;
      // output number `done` completed an item: stream_to_vector hands it to the Buffer (buffer.h:35-37)
      int64_t p = (int64_t)r.begin + (done * len + count - 1) / count - 1;
      const int64_t last = r.end > r.begin ? (int64_t)r.end - 1 : (int64_t)r.begin;
      p = p < r.begin ? r.begin : p > last ? last : p;
      s.items.insert(s.items.end(), s.pending.begin(), s.pending.end());
      s.item_times.push_back(frame_time(first_frame + p / m_stride));
      s.pending.clear();
    }
    if (flush) {  // Recorder::flush -> Buffer::popSingleSample, one publish per item
      for (size_t i = 0; i < s.item_times.size(); ++i) {
        if (m_publish) m_publish(s.item_times[i], m_center + r.shift_hz, m_bandwidth, s.items.data() + i * (size_t)m_itemSamples * 2, m_itemSamples);
      }
      m_published += s.item_times.size();
      s.items.clear();
      s.item_times.clear();
    }
    if (why == RangeEnd::Stop) drop(s);
    return true;
  }

  // End of the stream: open recordings are dropped like a stop. `pending` stays, as inside stream_to_vector.
  void finish() {
    for (Slot& s : m_slots) drop(s);
  }

 private:
  struct Slot {
    std::vector<int8_t> pending;  // inside stream_to_vector: less than one item
    std::vector<int8_t> items;    // the Buffer: whole items
    std::vector<int64_t> item_times;
  };
  void drop(Slot& s) {  // Recorder::stopRecording: m_buffer->clear()
    m_dropped += s.item_times.size();
    s.items.clear();
    s.item_times.clear();
  }
  const int32_t m_center, m_bandwidth;
  const int64_t m_stride;
  Publish m_publish;
  std::vector<Slot> m_slots;
  int m_itemSamples = 0;
  uint64_t m_published = 0, m_dropped = 0;
};

}  // namespace specscan

extern "C" {
// C binding (libspecscan_host.so, host/recording_host.cpp). Handles are opaque; arrays are caller-owned.
// time ms, frequency, sample rate, int8 (re,im) samples, their count: RecordingStore::Publish
typedef void (*srs_publish_fn)(int64_t time_ms, int32_t frequency, int32_t sample_rate, const int8_t* iq, int32_t nsamples, void* user);
typedef int64_t (*srs_frame_time_fn)(int64_t frame, void* user);
void* srs_create(int32_t slots, int32_t center_frequency, int32_t bandwidth, int64_t stride, srs_publish_fn publish, void* user);
void srs_destroy(void* store);
int32_t srs_item_samples(const void* store);
int32_t srs_feed(void* store, const sc_range* range, int32_t end, int32_t flush, const int8_t* iq, int64_t count, int64_t first_frame,
                 srs_frame_time_fn frame_time, void* user);
void srs_finish(void* store);
uint64_t srs_published(const void* store);
uint64_t srs_dropped(const void* store);
int32_t srs_pending_samples(const void* store, int32_t slot);
int32_t srs_held_items(const void* store, int32_t slot);
}
