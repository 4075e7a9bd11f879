// recording_host.cpp — C entry points of libspecscan_host.so for the two GPU-free recording classes: specscan::RangePlanner
// (host/range_planner.h, srp_*) and specscan::RecordingStore (host/recording_store.h, srs_*). What tests and other hosts bind
// (recorder.py). No exception crosses the binding: failures are return values, srp_last_error has the planner's reason.
#include <new>

#include "range_planner.h"
#include "recording_store.h"

using specscan::RangePlan;
using specscan::RangePlanner;
using specscan::RecordingStore;

extern "C" {

// NULL: slots not in 1..SC_MAX_CHANNELS or stride <= 0
void* srp_create(int32_t slots, int64_t stride) {
  try {
    auto* p = new RangePlanner(slots, stride);
    if (p->valid()) return p;
    delete p;
  } catch (...) {
  }
  return nullptr;
}

void srp_destroy(void* planner) { delete static_cast<RangePlanner*>(planner); }

const char* srp_last_error(const void* planner) { return planner ? static_cast<const RangePlanner*>(planner)->error().c_str() : "null planner"; }

// One batch: frame f's list is entries frame_off[f] .. frame_off[f + 1] of shifts / flush (nonzero: asked to flush). Writes the plan
// to ranges / ends (0 stop, 1 batch) / flushes, each with room for SC_MAX_RANGES entries, and returns the number of ranges; -1 — and
// nothing changed — for a plan the planner refuses (srp_last_error).
int32_t srp_plan(void* planner, int32_t nframes, const int32_t* frame_off, const int32_t* shifts, const uint8_t* flush, sc_range* ranges,
                 int32_t* ends, int32_t* flushes) {
  if (!planner || nframes < 0 || (nframes > 0 && !frame_off)) return -1;
  try {
    auto* p = static_cast<RangePlanner*>(planner);
    std::vector<RangePlanner::Frame> frames((size_t)nframes);
    for (int32_t f = 0; f < nframes; ++f)
      for (int32_t i = frame_off[f]; i < frame_off[f + 1]; ++i) frames[(size_t)f].push_back(specscan::FrequencyFlush{shifts[i], flush[i] != 0});
    RangePlan plan;
    if (!p->plan(frames, &plan)) return -1;
    for (size_t i = 0; i < plan.ranges.size(); ++i) {
      ranges[i] = plan.ranges[i];
      ends[i] = (int32_t)plan.ends[i];
      flushes[i] = plan.flushes[i];
    }
    return (int32_t)plan.ranges.size();
  } catch (...) {
    return -1;
  }
}

// shifts[slot] (INT32_MAX while idle) and recording[slot] for every slot; returns the slot count
int32_t srp_slots(const void* planner, int32_t* shifts, int32_t* recording) {
  const auto* p = static_cast<const RangePlanner*>(planner);
  if (!p) return -1;
  for (int k = 0; k < p->slots(); ++k) {
    if (shifts) shifts[k] = p->shift(k);
    if (recording) recording[k] = p->recording(k) ? 1 : 0;
  }
  return p->slots();
}

// the ignored set, ascending: its size; the first min(size, cap) shifts go to out
int32_t srp_ignored(const void* planner, int32_t* out, int32_t cap) {
  const auto* p = static_cast<const RangePlanner*>(planner);
  if (!p) return -1;
  int32_t n = 0;
  for (int32_t s : p->ignored()) {
    if (out && n < cap) out[n] = s;
    ++n;
  }
  return n;
}

// NULL: slots not in 1..SC_MAX_CHANNELS, bandwidth <= 0 or stride <= 0
void* srs_create(int32_t slots, int32_t center_frequency, int32_t bandwidth, int64_t stride, srs_publish_fn publish, void* user) {
  if (slots < 1 || slots > SC_MAX_CHANNELS || bandwidth <= 0 || stride <= 0) return nullptr;
  try {
    RecordingStore::Publish fn;
    if (publish) fn = [publish, user](int64_t t, int32_t f, int32_t rate, const int8_t* iq, int n) { publish(t, f, rate, iq, (int32_t)n, user); };
    return new RecordingStore(slots, center_frequency, bandwidth, stride, std::move(fn));
  } catch (...) {
    return nullptr;
  }
}

void srs_destroy(void* store) { delete static_cast<RecordingStore*>(store); }

int32_t srs_item_samples(const void* store) { return store ? static_cast<const RecordingStore*>(store)->itemSamples() : -1; }

// RecordingStore::feed: end 0 stop / 1 batch, iq = count int8 (re,im) samples. 0, or -1 for a bad argument.
int32_t srs_feed(void* store, const sc_range* range, int32_t end, int32_t flush, const int8_t* iq, int64_t count, int64_t first_frame,
                 srs_frame_time_fn frame_time, void* user) {
  if (!store || !range || !frame_time || (end != 0 && end != 1) || (count > 0 && !iq)) return -1;
  try {
    const auto ft = [frame_time, user](int64_t frame) { return frame_time(frame, user); };
    return static_cast<RecordingStore*>(store)->feed(*range, end == 0 ? specscan::RangeEnd::Stop : specscan::RangeEnd::Batch, flush != 0, iq, count,
                                                     first_frame, ft)
               ? 0
               : -1;
  } catch (...) {
    return -1;
  }
}

void srs_finish(void* store) {
  if (store) static_cast<RecordingStore*>(store)->finish();
}

uint64_t srs_published(const void* store) { return store ? static_cast<const RecordingStore*>(store)->published() : 0; }
uint64_t srs_dropped(const void* store) { return store ? static_cast<const RecordingStore*>(store)->dropped() : 0; }

int32_t srs_pending_samples(const void* store, int32_t slot) {
  const auto* s = static_cast<const RecordingStore*>(store);
  return s && slot >= 0 && slot < s->slots() ? s->pendingSamples(slot) : -1;
}

int32_t srs_held_items(const void* store, int32_t slot) {
  const auto* s = static_cast<const RecordingStore*>(store);
  return s && slot >= 0 && slot < s->slots() ? s->heldItems(slot) : -1;
}

}  // extern "C"
