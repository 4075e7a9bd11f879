// recording_check.cpp — host/range_planner.h and host/recording_store.h alone, under the sanitizers (tests/test_range_planner_host.py
// builds and runs it): random sessions of per-frame (shift, flush) lists, and for every batch
//   - the plan passes chan_ranges::validate (what srf_record asks of a list) and its ranges lie on frame boundaries;
//   - the plan covers each recording's frames exactly once, with the recording's shift: a plain frame-by-frame walk of
//     SdrDevice::updateRecordings (sdr_device.cpp:82-144), kept here, says which slot records which shift in which frame;
//   - a plan of more than SC_MAX_RANGES ranges is refused and changes nothing, and its frames are taken in smaller pieces;
//   - the store cuts the outputs it is fed into whole items, each a run of its slot's output stream that begins at a multiple of
//     the item size, stamped with a frame of the range that completed it, and every output is pending, held, published or dropped.
// Prints "sessions <n> batches <n> ranges <n> refused <n> items <n> bad <b>"; exit status 1 when bad != 0.
#include <cstdint>
#include <cstdio>
#include <random>
#include <set>
#include <vector>

#include "../../rtl-sdr-scanner-cpp_amd/csrc/chan_ranges.h"
#include "range_planner.h"
#include "recording_store.h"

using specscan::FrequencyFlush;
using specscan::RangeEnd;
using specscan::RangePlan;
using specscan::RangePlanner;
using specscan::RecordingStore;
using Frame = RangePlanner::Frame;

namespace {

long long g_bad = 0;
void expect(bool ok, const char* what, int session) {
  if (ok) return;
  if (++g_bad <= 20) printf("session %d: %s\n", session, what);
}

// updateRecordings frame by frame: rec[k] / shift[k] after the frame's list has been applied = what the frame's samples go to
struct Walk {
  std::vector<char> rec;
  std::vector<int32_t> shift;
  std::set<int32_t> ignored;
  explicit Walk(int slots) : rec((size_t)slots, 0), shift((size_t)slots, RangePlanner::IDLE) {}
  void frame(const Frame& want) {
    const auto waiting = [&](int32_t s) {
      for (const auto& x : want)
        if (x.shift_hz == s) return true;
      return false;
    };
    for (size_t k = 0; k < rec.size(); ++k)
      if (rec[k] && !waiting(shift[k])) rec[k] = 0, shift[k] = RangePlanner::IDLE;
    for (const auto& x : want) {
      bool hit = false;
      for (size_t k = 0; k < rec.size(); ++k) hit = hit || shift[k] == x.shift_hz;
      if (hit) continue;
      size_t k = 0;
      while (k < rec.size() && rec[k]) ++k;
      if (k < rec.size()) rec[k] = 1, shift[k] = x.shift_hz;
      else ignored.insert(x.shift_hz);
    }
    for (auto it = ignored.begin(); it != ignored.end();) it = waiting(*it) ? std::next(it) : ignored.erase(it);
  }
};

const int32_t kPool[8] = {-412500, -270000, -100000, -2500, 0, 57500, 182500, 310000};
const int64_t kStrides[4] = {256, 1024, 1280, 2048};

}  // namespace

int main() {
  long long sessions = 0, batches = 0, ranges = 0, refused = 0, items = 0;
  for (int session = 0; session < 260; ++session) {
    std::mt19937 rng((uint32_t)session * 2654435761u + 17u);
    const auto below = [&](int n) { return (int)(rng() % (uint32_t)n); };
    const int slots = 1 + below(4);
    const int64_t stride = kStrides[below(4)];
    const bool dense = session % 13 == 0;  // recordings of a frame or two: more ranges than one srf_record takes
    const int32_t center = 145000000, bandwidth = 16000;
    const int ratio = 16;  // outputs: about one per `ratio` input samples, and now and then exactly what completes an item

    struct Item {
      int64_t time;
      int32_t frequency;
      std::vector<int8_t> iq;
    };
    std::vector<Item> published;
    RecordingStore store(slots, center, bandwidth, stride, [&](int64_t t, int32_t f, int32_t rate, const int8_t* iq, int n) {
      expect(rate == bandwidth && n == 4096, "publish: sample rate or item size", session);
      published.push_back(Item{t, f, std::vector<int8_t>(iq, iq + 2 * (size_t)n)});
    });
    expect(store.itemSamples() == 4096, "itemSamples", session);
    const auto frame_time = [&](int64_t frame) { return 1000 * frame * stride / 1024000; };

    RangePlanner planner(slots, stride);
    Walk walk(slots);
    std::vector<int64_t> produced((size_t)slots, 0);  // outputs fed per slot so far: the index of the slot's next output
    std::vector<int32_t> live;                        // the shifts asked for, in list order
    std::vector<int> left;
    int64_t first_frame = 0;
    const int nbatches = 3 + below(6);
    for (int b = 0; b < nbatches; ++b) {
      const int nframes = below(8) == 0 ? 0 : 1 + below(dense ? 200 : 70);
      std::vector<Frame> frames((size_t)nframes);
      for (int f = 0; f < nframes; ++f) {
        for (size_t i = live.size(); i-- > 0;)
          if (left[i] <= 0) live.erase(live.begin() + (long)i), left.erase(left.begin() + (long)i);
        if (live.size() < 6 && below(100) < (dense ? 70 : 10)) {
          const int32_t s = kPool[below(8)];
          bool have = false;
          for (int32_t x : live) have = have || x == s;
          if (!have) live.push_back(s), left.push_back(dense ? 1 + below(2) : 3 + below(117));
        }
        for (size_t i = 0; i < live.size(); ++i) frames[(size_t)f].push_back(FrequencyFlush{live[i], below(2) == 1}), --left[i];
      }
      // the plan, in pieces if the planner refuses the whole
      std::vector<std::pair<int, int>> pieces{{0, nframes}};
      RangePlan plan;
      {
        const RangePlanner before = planner;
        if (!planner.plan(frames, &plan)) {
          ++refused;
          expect(planner.error().find("smaller batch") != std::string::npos, "refusal without advice", session);
          bool same = planner.ignored() == before.ignored();
          for (int k = 0; k < slots; ++k) same = same && planner.shift(k) == before.shift(k) && planner.recording(k) == before.recording(k);
          expect(same, "a refused plan changed the planner", session);
          pieces.clear();
          for (int at = 0; at < nframes; at += 16) pieces.push_back({at, at + 16 < nframes ? at + 16 : nframes});
        } else {
          pieces.assign(1, {0, nframes});
        }
      }
      for (size_t piece = 0; piece < pieces.size(); ++piece) {
        const int lo = pieces[piece].first, hi = pieces[piece].second, n = hi - lo;
        if (pieces.size() > 1 || piece > 0) expect(planner.plan(frames.data() + lo, n, &plan), "a piece of 16 frames refused", session);
        ++batches;
        ranges += (long long)plan.ranges.size();
        expect(plan.ranges.size() == plan.ends.size() && plan.ranges.size() == plan.flushes.size(), "plan arrays differ in length", session);
        expect(chan_ranges::validate(plan.ranges.data(), (int)plan.ranges.size(), slots, (int)(n * stride)) == nullptr, "chan_ranges::validate", session);
        // coverage: every (slot, frame) the walk records is in exactly one range with the walk's shift, and nothing else is
        std::vector<int> cover((size_t)slots * (size_t)(n > 0 ? n : 1), 0);
        std::vector<int32_t> cover_shift(cover.size(), RangePlanner::IDLE);
        for (const sc_range& r : plan.ranges) {
          expect(r.begin % stride == 0 && r.end % stride == 0, "a range off the frame boundaries", session);
          for (int64_t f = r.begin / stride; f < r.end / stride; ++f) ++cover[(size_t)r.channel * (size_t)n + (size_t)f], cover_shift[(size_t)r.channel * (size_t)n + (size_t)f] = r.shift_hz;
        }
        for (int f = 0; f < n; ++f) {
          walk.frame(frames[(size_t)(lo + f)]);
          for (int k = 0; k < slots; ++k) {
            const size_t at = (size_t)k * (size_t)n + (size_t)f;
            expect(cover[at] == (walk.rec[(size_t)k] ? 1 : 0), "a frame covered twice, or not as the walk records it", session);
            expect(!walk.rec[(size_t)k] || cover_shift[at] == walk.shift[(size_t)k], "a frame covered with another shift", session);
          }
        }
        bool same = planner.ignored() == walk.ignored;
        for (int k = 0; k < slots; ++k) same = same && planner.shift(k) == walk.shift[(size_t)k] && planner.recording(k) == (walk.rec[(size_t)k] != 0);
        expect(same, "planner state differs from the walk's", session);
        for (size_t i = 0; i < plan.ranges.size(); ++i) {
          expect(plan.ends[i] == RangeEnd::Batch ? plan.ranges[i].end == n * stride : true, "a batch range that ends early", session);
          expect(plan.ends[i] == RangeEnd::Stop ? plan.ranges[i].end < n * stride : true, "a stop at the batch's end", session);
        }
        // the store: outputs numbered along the slot's stream, two bytes of the number per sample
        for (size_t i = 0; i < plan.ranges.size(); ++i) {
          const sc_range& r = plan.ranges[i];
          const int k = r.channel;
          int64_t count = (r.end - r.begin) / ratio;
          if (count > 0 && below(3) == 0) count = 4096 - store.pendingSamples(k) + 4096 * below(2);  // ends on an item's last sample
          std::vector<int8_t> iq((size_t)count * 2);
          for (int64_t j = 0; j < count; ++j) {
            const int64_t idx = produced[(size_t)k] + j;
            iq[(size_t)j * 2] = (int8_t)(uint8_t)(idx & 0xff), iq[(size_t)j * 2 + 1] = (int8_t)(uint8_t)((idx >> 8) & 0xff);
          }
          const size_t had = published.size();
          const uint64_t gone = store.published() + store.dropped();
          const int held = store.heldItems(k);
          expect(store.feed(r, plan.ends[i], plan.flushes[i] != 0, iq.data(), count, first_frame + lo, frame_time), "feed refused", session);
          produced[(size_t)k] += count;
          const int64_t completed = (int64_t)(store.published() + store.dropped() - gone) + store.heldItems(k) - held;
          expect(completed == (produced[(size_t)k] / 4096) - ((produced[(size_t)k] - count) / 4096), "items completed by a range", session);
          expect(store.pendingSamples(k) == (int)(produced[(size_t)k] % 4096), "pending is not the stream's remainder", session);
          expect(plan.flushes[i] || published.size() == had, "published without a flush", session);
          expect(!(plan.flushes[i] || plan.ends[i] == RangeEnd::Stop) || store.heldItems(k) == 0, "items held past a flush or a stop", session);
          for (size_t p = had; p < published.size(); ++p) {
            const Item& it = published[p];
            const int64_t start = (uint8_t)it.iq[0] | ((int64_t)(uint8_t)it.iq[1] << 8);
            bool run = start % 4096 == 0;
            for (int64_t j = 0; run && j < 4096; ++j)
              run = (uint8_t)it.iq[(size_t)j * 2] == (uint8_t)((start + j) & 0xff) && (uint8_t)it.iq[(size_t)j * 2 + 1] == (uint8_t)(((start + j) >> 8) & 0xff);
            expect(run, "an item is not a whole-item run of its slot's stream", session);
            expect(it.frequency == center + r.shift_hz, "item frequency", session);
            expect(it.time <= frame_time(first_frame + lo + (r.end - 1) / stride), "an item stamped after its range", session);
            expect(p == had || published[p - 1].time <= it.time, "item times descend within a flush", session);
          }
        }
        expect(!store.feed(sc_range{slots, 0, 0, 0}, RangeEnd::Stop, false, nullptr, 0, 0, frame_time), "a channel the store lacks was taken", session);
      }
      first_frame += nframes;
    }
    const uint64_t before = store.published() + store.dropped();
    int held = 0;
    for (int k = 0; k < slots; ++k) held += store.heldItems(k);
    store.finish();
    expect(store.published() + store.dropped() == before + (uint64_t)held, "finish did not drop what was held", session);
    uint64_t whole = 0;
    for (int k = 0; k < slots; ++k) whole += (uint64_t)(produced[(size_t)k] / 4096), expect(store.heldItems(k) == 0, "held after finish", session);
    expect(store.published() + store.dropped() == whole && store.published() == published.size(), "outputs lost or made up", session);
    items += (long long)store.published();
    ++sessions;
  }
  printf("sessions %lld batches %lld ranges %lld refused %lld items %lld bad %lld\n", sessions, batches, ranges, refused, items, g_bad);
  return g_bad == 0 ? 0 : 1;
}
