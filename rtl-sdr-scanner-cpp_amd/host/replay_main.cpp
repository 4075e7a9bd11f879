// specscan_replay — a C++ host on the C ABI alone (include/specscan.h + host/raw_file.h), no Python, no GNU Radio:
// streams one of the reference's raw IQ dumps (`full_<date>_<time>_<centre>_<rate>_fc.raw`, or .cs8 / .cu8 / .cs16;
// sources/utils/radio_utils.cpp:78-84, scripts/converter.py:30-38) through the scan chain the way SdrDevice drives
// it (sources/radio/sdr_device.cpp:148-168), with the pipelined feed: a reader thread fills pinned slots while
// earlier batches cross PCIe and run. Optionally writes the raw PSD rows as the reference's DEBUG_SAVE_FULL_POWER
// dump would (`..._power.raw`, sdr_device.cpp:173-176).
//
//   specscan_replay <dump> [--fft N] [--decim D] [--batch B] [--depth K] [--learn-frames L] [--power-dir DIR] [--track | --track-sparse | --track-ring [--bandwidth HZ]]
//                   [--spectrogram-out FILE [--spectrogram-max-rows R] [--spectrogram-ring]] [--record-out FILE [--recorders R]] [--min-time-ms M] [--timeout-ms T]
//                   [--fold-cs16]
// Prints one JSON line: frames, batches, candidates, seconds, MS/s (file + PCIe inclusive).
//
// --track: the feed is a tracked one (include/specscan_track_feed.h) — every batch is digested on the device behind its chain, and
// the consumer thread owns a specscan::SignalTracker (host/signal_tracker.h): after each stf_collect it runs the batch's frames
// through processFrameDigest (frame time 1000 * frame_index * N * D / fs ms, the stream's own clock) and posts its keys. The reader
// thread is unchanged. The JSON line gains `transmissions` (entries of the per-frame lists, summed) and `tracked_frames`.
// --track-sparse: the same tracker and the same JSON, but the context keeps no planes (no SS_FLAG_KEEP_PLANES): the tracked feed is a
// sparse one (include/specscan_track_sparse.h) that re-evaluates the tile columns the watch windows touch behind every batch. The JSON
// line gains `tiles_evaluated` and `tiles_in_batches` (stf_sparse_stats).
// --track-ring: --track-sparse at every transform size (include/specscan_track_feed_ring.h): from 65536 points up the batches take the
// scan's forms that keep no dB plane and are digested from the rows they leave in the averager ring's buffer. The same JSON.
// --spectrogram-out FILE: the feed delivers the spectrogram rows (include/specscan_spectrogram_feed.h; the context gets
// SS_FLAG_SPECTROGRAM). Frame k carries the time nearbyint(k * period), period = 1000 * N * D / fs ms — the clock the reference's
// per-frame send gate runs on — and every row a batch closes is written to FILE as its DataController::pushSpectrogram payload
// (ss_spectrogram_payload) behind its length as a little-endian uint32. The JSON line gains `spectrogram_rows`.
// --spectrogram-ring (with --spectrogram-out): the rows come from sgf_create_ring (include/specscan_spectrogram_feed_ring.h) — the
// context is created WITHOUT SS_FLAG_SPECTROGRAM, so with --track-ring the batches of 65536 points and up keep taking the forms that
// write no dB plane, and the rows are formed from what they leave in the averager ring's buffer. The same payloads; the JSON line
// gains `"spectrogram_ring": true`. Without the switch --spectrogram-out makes every batch keep its plane, as ever.
// --record-out FILE (needs --track, --track-sparse or --track-ring): the transmissions the tracker finds are recorded from the feed's own upload
// (host/feed_recorder.h: RangePlanner -> srf_record -> RecordingStore; --recorders R slots, default 4; the recording bandwidth is
// --bandwidth). After each stf_collect the consumer runs the tracker over the batch's frames, posts the keys and hands the frames'
// lists to the FeedRecorder. With decim != 1 the feed is a whole-item feed (ss_feed_create_items) and the dump is read in whole items
// of N * D samples: only the recorded ranges are uploaded a second time. Every published item is written to FILE as its
// DataController::pushTransmission payload (sc_transmission_payload) behind its length as a little-endian uint32. The JSON line gains
// `recorded_ranges`, `recorded_samples`, `published_items`, `dropped_items`, `record_h2d_bytes` and `ignored_shifts_max`.
// --min-time-ms M / --timeout-ms T: Config::recordingMinTime / recordingTimeout of the tracker (2000 / 2000).
// --fold-cs16: the context gets SS_FLAG_FOLD_CS16 — a .cs16 dump of 65536 / 131072-point frames goes through the work-buffer-free fold
// in the batches that keep no plane, which are those of --track-ring / --spectrogram-ring (every other feed keeps planes, and the flag
// has no effect); results then meet the oracle contract instead of being bit-identical to the CF32 path's. The JSON line gains `"fold": true|false`
// (SS_STATE_FOLD of ss_get_stats).
#include <specscan.h>
#include <specscan_spectrogram_feed.h>
#include <specscan_spectrogram_feed_ring.h>
#include <specscan_track_feed.h>
#include <specscan_track_feed_ring.h>
#include <specscan_track_sparse.h>

#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "feed_recorder.h"
#include "raw_file.h"
#include "signal_tracker.h"

namespace {

struct Options {
  std::string path, power_dir, spectrogram_out, record_out;
  int recorders = 4;
  int min_time_ms = -1, timeout_ms = -1;  // < 0: TrackerConfig's own
  int spectrogram_max_rows = 8;
  int fft = 0, decim = 0, batch = 1024, depth = 3, learn_frames = -1;
  bool track = false, track_sparse = false, track_ring = false, spectrogram_ring = false, fold_cs16 = false;
  int bandwidth = 32000;  // Config::recordingBandwidth: the tracker's windows are ceil(bandwidth / (fs / N)) bins wide
};

bool parse_args(int argc, char** argv, Options* o) {
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    const auto next = [&](int* dst) {
      if (i + 1 >= argc) return false;
      *dst = atoi(argv[++i]);
      return true;
    };
    if (a == "--fft") {
      if (!next(&o->fft)) return false;
    } else if (a == "--decim") {
      if (!next(&o->decim)) return false;
    } else if (a == "--batch") {
      if (!next(&o->batch)) return false;
    } else if (a == "--depth") {
      if (!next(&o->depth)) return false;
    } else if (a == "--learn-frames") {
      if (!next(&o->learn_frames)) return false;
    } else if (a == "--track") {
      o->track = true;
    } else if (a == "--track-sparse") {
      o->track = o->track_sparse = true;
    } else if (a == "--track-ring") {
      o->track = o->track_sparse = o->track_ring = true;
    } else if (a == "--bandwidth") {
      if (!next(&o->bandwidth) || o->bandwidth <= 0) return false;
    } else if (a == "--spectrogram-out") {
      if (i + 1 >= argc) return false;
      o->spectrogram_out = argv[++i];
    } else if (a == "--spectrogram-ring") {
      o->spectrogram_ring = true;
    } else if (a == "--fold-cs16") {
      o->fold_cs16 = true;
    } else if (a == "--spectrogram-max-rows") {
      if (!next(&o->spectrogram_max_rows)) return false;
    } else if (a == "--record-out") {
      if (i + 1 >= argc) return false;
      o->record_out = argv[++i];
    } else if (a == "--recorders") {
      if (!next(&o->recorders)) return false;
    } else if (a == "--min-time-ms") {
      if (!next(&o->min_time_ms) || o->min_time_ms < 0) return false;
    } else if (a == "--timeout-ms") {
      if (!next(&o->timeout_ms) || o->timeout_ms < 0) return false;
    } else if (a == "--power-dir") {
      if (i + 1 >= argc) return false;
      o->power_dir = argv[++i];
    } else if (!a.empty() && a[0] != '-' && o->path.empty()) {
      o->path = a;
    } else {
      return false;
    }
  }
  if (!o->record_out.empty() && !o->track) return false;  // nothing to record without the tracker's lists
  if (o->spectrogram_ring && o->spectrogram_out.empty()) return false;
  return !o->path.empty();
}

}  // namespace

int main(int argc, char** argv) {
  Options opt;
  if (!parse_args(argc, argv, &opt)) {
    fprintf(stderr, "usage: %s <dump> [--fft N] [--decim D] [--batch B] [--depth K] [--learn-frames L] [--power-dir DIR] [--track | --track-sparse | --track-ring [--bandwidth HZ]] [--spectrogram-out FILE [--spectrogram-max-rows R] [--spectrogram-ring]] [--record-out FILE [--recorders R]] [--min-time-ms M] [--timeout-ms T] [--fold-cs16]\n", argv[0]);
    return 2;
  }
  specscan::RawFileInfo info;
  if (!specscan::parseRawFileName(opt.path, &info) || info.kind == specscan::RawKind::F32) {
    fprintf(stderr, "%s: not a raw IQ dump name (<label>_<date>_<time>_<centre>_<rate>_fc.raw | .cs8 | .cu8 | .cs16)\n", opt.path.c_str());
    return 2;
  }
  ss_config cfg;
  ss_default_config(&cfg, info.sample_rate, info.frequency);  // N = getFft(rate, 250), D = max(1, step/50): sdr_device.cpp:149-150
  if (opt.fft > 0) cfg.fft_size = opt.fft;
  if (opt.decim > 0) cfg.decim = opt.decim;
  if (opt.learn_frames >= 0) cfg.learn_frames = opt.learn_frames;
  if (opt.track && !opt.track_sparse) cfg.flags |= SS_FLAG_KEEP_PLANES;  // the digest reads the kept dB and avg planes
  const bool want_rows = !opt.spectrogram_out.empty();
  if (want_rows && !opt.spectrogram_ring) cfg.flags |= SS_FLAG_SPECTROGRAM;  // (sgf_create_ring wants a context without it)
  if (opt.fold_cs16) cfg.flags |= SS_FLAG_FOLD_CS16;  // (without effect where the fold cannot run: specscan.h)
  cfg.max_batch = opt.batch;
  if (info.kind == specscan::RawKind::CS8 || info.kind == specscan::RawKind::CU8) {
    cfg.in_format = info.kind == specscan::RawKind::CS8 ? SS_FMT_CS8 : SS_FMT_CU8;
    cfg.int_scale = 1.0f / 127.5f;  // converter.py:33
  } else if (info.kind == specscan::RawKind::CS16) {
    cfg.in_format = SS_FMT_CS16;
    cfg.int_scale = 1.0f / 32768.0f;
  }
  ss_ctx* ctx = nullptr;
  if (ss_create(&cfg, &ctx) != SS_OK) {
    fprintf(stderr, "ss_create: %s\n", ss_last_error(nullptr));
    return 1;
  }
  const bool want_power = !opt.power_dir.empty();
  const bool want_record = !opt.record_out.empty();
  const bool items = want_record && cfg.decim != 1;  // the slots keep the whole items: the recorder has the stream between the frames
  ss_feed* feed = nullptr;
  if ((items ? ss_feed_create_items : ss_feed_create)(ctx, opt.depth, 1 << 20, want_power ? 1 : 0, &feed) != SS_OK) {
    fprintf(stderr, "%s: %s\n", items ? "ss_feed_create_items" : "ss_feed_create", ss_last_error(ctx));
    ss_destroy(ctx);
    return 1;
  }
  stf_ctx* tracked = nullptr;
  specscan::TrackerConfig tc;
  tc.fft_size = cfg.fft_size;
  tc.sample_rate = info.sample_rate;
  tc.start_level = cfg.start_level;
  tc.grouping_y = cfg.grouping_y;
  tc.group_size = (int)((((long long)opt.bandwidth * cfg.fft_size) + info.sample_rate - 1) / info.sample_rate);  // sdr_device.cpp:151
  if (opt.min_time_ms >= 0) tc.min_time_ms = opt.min_time_ms;
  if (opt.timeout_ms >= 0) tc.timeout_ms = opt.timeout_ms;
  if (opt.track) {
    stf_config tcfg{STF_ABI_VERSION, tc.group_size, cfg.start_level, 4096};
    const auto create = opt.track_ring ? stf_create_ring : opt.track_sparse ? stf_create_sparse : stf_create;
    if (create(feed, &tcfg, &tracked) != SS_OK) {
      fprintf(stderr, "%s: %s\n", opt.track_ring ? "stf_create_ring" : opt.track_sparse ? "stf_create_sparse" : "stf_create", stf_last_error(nullptr));
      ss_feed_destroy(feed);
      ss_destroy(ctx);
      return 1;
    }
  }
  sgf_ctx* rows = nullptr;
  FILE* rows_file = nullptr;
  if (want_rows) {
    sgf_config rcfg{SGF_ABI_VERSION, opt.spectrogram_max_rows, 0};
    if ((opt.spectrogram_ring ? sgf_create_ring : sgf_create)(feed, &rcfg, &rows) != SS_OK)
      fprintf(stderr, "%s: %s\n", opt.spectrogram_ring ? "sgf_create_ring" : "sgf_create", sgf_last_error(nullptr));
    else if (!(rows_file = fopen(opt.spectrogram_out.c_str(), "wb"))) fprintf(stderr, "%s: cannot open for writing\n", opt.spectrogram_out.c_str());
    if (!rows_file) {
      sgf_destroy(rows);
      stf_destroy(tracked);
      ss_feed_destroy(feed);
      ss_destroy(ctx);
      return 1;
    }
  }
  const double frame_period_ms = 1000.0 * cfg.fft_size * cfg.decim / info.sample_rate;
  int rc = 0;
  FILE* record_file = nullptr;
  try {
    // the recorder last: its srf_ctx goes before the feed does
    bool record_failed = false;
    std::vector<uint8_t> record_payload;
    std::unique_ptr<specscan::FeedRecorder> recorder;
    if (want_record) {
      if (!(record_file = fopen(opt.record_out.c_str(), "wb"))) throw std::runtime_error(opt.record_out + ": cannot open for writing");
      recorder = std::make_unique<specscan::FeedRecorder>(
          feed, opt.bandwidth, opt.recorders, (int64_t)cfg.fft_size * cfg.decim, info.frequency,
          [&](int64_t time_ms, int32_t frequency, int32_t sample_rate, const int8_t* iq, int nsamples) {
            const int len = sc_transmission_payload((uint64_t)time_ms, frequency, sample_rate, iq, nsamples, nullptr, 0);
            if (len > 0) record_payload.resize((size_t)len);
            const uint8_t head[4] = {(uint8_t)len, (uint8_t)(len >> 8), (uint8_t)(len >> 16), (uint8_t)(len >> 24)};
            if (len <= 0 || sc_transmission_payload((uint64_t)time_ms, frequency, sample_rate, iq, nsamples, record_payload.data(), len) != len ||
                fwrite(head, 1, 4, record_file) != 4 || fwrite(record_payload.data(), 1, (size_t)len, record_file) != (size_t)len)
              record_failed = true;
          });
    }
    // whole items of N * D samples for a whole-item feed, as replay.replay_file(items=True) reads them
    specscan::RawIqReader reader(opt.path, info.kind, items ? cfg.fft_size * cfg.decim : cfg.fft_size, items ? 1 : cfg.decim);
    specscan::RawFileSink power(sizeof(float) * (size_t)cfg.fft_size);  // FileSink<float>(fftSize, false)
    if (want_power) {
      std::tm tm{};
      tm.tm_year = info.year - 1900, tm.tm_mon = info.month - 1, tm.tm_mday = info.day;
      tm.tm_hour = info.hour, tm.tm_min = info.minute, tm.tm_sec = info.second;
      power.startRecording(opt.power_dir + "/" + specscan::makeRawFileName("full", "power", info.frequency, info.sample_rate, tm).substr(2));
    }
    // slot accounting between the reader thread and this one
    std::mutex mtx;
    std::condition_variable cv;
    int free_slots = opt.depth, submitted = 0;
    bool reader_done = false, failed = false;
    std::string error;

    const auto t0 = std::chrono::steady_clock::now();
    std::thread producer([&] {
      for (;;) {
        {
          std::unique_lock<std::mutex> lock(mtx);
          cv.wait(lock, [&] { return free_slots > 0 || failed; });
          if (failed) break;
          --free_slots;
        }
        void* frames = nullptr;
        int got = 0;
        try {
          if (ss_feed_acquire(feed, &frames) != SS_OK) throw std::runtime_error(ss_last_error(ctx));
          got = reader.readFramesParallel(frames, cfg.max_batch, 4);
          std::vector<int64_t> t_ms;
          if (want_rows)  // (round to even, as numpy's round: replay.replay_file gives the same clock)
            for (int k = 0; k < got; ++k) t_ms.push_back((int64_t)std::nearbyint((double)(reader.position() - got + k) * frame_period_ms));
          if (got > 0 && ss_feed_submit(feed, got, want_rows ? t_ms.data() : nullptr, reader.position() - got) != SS_OK) throw std::runtime_error(ss_last_error(ctx));
        } catch (const std::exception& e) {
          std::lock_guard<std::mutex> lock(mtx);
          failed = true;
          error = e.what();
        }
        std::lock_guard<std::mutex> lock(mtx);
        if (got > 0 && !failed) ++submitted;
        if (got == 0 || failed) {
          reader_done = true;
          cv.notify_all();
          break;
        }
        cv.notify_all();
      }
    });

    long long frames = 0, batches = 0, candidates = 0, transmissions = 0, tracked_frames = 0, spectrogram_rows = 0;
    std::vector<uint8_t> payload;
    specscan::SignalTracker tracker(tc);
    std::vector<specscan::RangePlanner::Frame> lists;  // the tracker's list of every frame of the batch, for the recorder
    const auto frame_time_ms = [&](long long index) { return (int64_t)(1000ll * index * cfg.fft_size * cfg.decim / info.sample_rate); };
    for (;;) {
      {
        std::unique_lock<std::mutex> lock(mtx);
        cv.wait(lock, [&] { return submitted > 0 || reader_done; });
        if (submitted == 0) break;
        --submitted;
      }
      ss_feed_result r;
      stf_result d;
      std::string why;
      if (tracked) {
        if (stf_collect(tracked, &d) != SS_OK) why = stf_last_error(tracked);
        else if (d.status != SS_OK) why = "more watch keys than the tracked feed holds";
        r = d.batch;
        for (int f = 0; why.empty() && f < r.nframes; ++f) {
          const int a = r.cand_off[f] < d.ncand ? r.cand_off[f] : d.ncand, b = r.cand_off[f + 1] < d.ncand ? r.cand_off[f + 1] : d.ncand;
          const auto* tx = tracker.processFrameDigest(frame_time_ms(frames + f), r.cand_idx + a, d.cand_avg + a, d.cand_best + a, b - a, d.watch,
                                                      d.nwatch, d.peak_idx + (size_t)f * d.nwatch, d.peak_avg + (size_t)f * d.nwatch);
          if (!tx) why = "a tracked key is missing from the digest's watch list";
          else transmissions += (long long)tx->size();
          if (tx && recorder) {
            if (lists.size() <= (size_t)f) lists.resize((size_t)f + 1);
            lists[(size_t)f] = *tx;
          }
        }
        if (why.empty()) {
          const std::vector<int> keys = tracker.signalKeys();
          tracked_frames += r.nframes;
          if (stf_post_keys(tracked, d.seq, keys.data(), (int32_t)keys.size()) != SS_OK) why = stf_last_error(tracked);
        }
        if (why.empty() && recorder) {  // plan the lists, record the ranges from the held batch (or let it go), publish what flushed
          lists.resize((size_t)r.nframes);
          if (!recorder->record(lists, frames, frame_time_ms)) why = recorder->error();
          else if (record_failed) why = "writing the transmission payloads failed";
        }
      } else if (ss_feed_collect(feed, &r) != SS_OK) {
        why = ss_last_error(ctx);
      }
      if (why.empty() && rows) {
        sgf_result g;
        if (sgf_rows(rows, &g) != SS_OK) why = sgf_last_error(rows);
        for (int k = 0; why.empty() && k < g.nrows; ++k) {
          const int8_t* row = g.rows + (size_t)k * (size_t)g.size;
          const int len = ss_spectrogram_payload((uint64_t)g.time_ms[k], g.frequency, g.sample_rate, row, g.size, nullptr, 0);
          if (len > 0) payload.resize((size_t)len);
          const uint8_t head[4] = {(uint8_t)len, (uint8_t)(len >> 8), (uint8_t)(len >> 16), (uint8_t)(len >> 24)};
          if (len <= 0 || ss_spectrogram_payload((uint64_t)g.time_ms[k], g.frequency, g.sample_rate, row, g.size, payload.data(), len) != len ||
              fwrite(head, 1, 4, rows_file) != 4 || fwrite(payload.data(), 1, (size_t)len, rows_file) != (size_t)len)
            why = "writing the spectrogram payloads failed";
          else ++spectrogram_rows;
        }
      }
      if (!why.empty()) {
        std::lock_guard<std::mutex> lock(mtx);
        failed = true;
        error = why;
        cv.notify_all();
        break;
      }
      if (want_power) {
        try {
          power.work(r.psd_db, r.nframes);
        } catch (const std::exception& e) {  // the producer thread is still joinable: report, wake it, fall through to the join
          std::lock_guard<std::mutex> lock(mtx);
          failed = true;
          error = e.what();
          cv.notify_all();
          break;
        }
      }
      frames += r.nframes;
      candidates += r.cand_off[r.nframes];
      ++batches;
      std::lock_guard<std::mutex> lock(mtx);
      ++free_slots;
      cv.notify_all();
    }
    producer.join();
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    uint64_t tiles_evaluated = 0, tiles_in_batches = 0;
    if (!failed && opt.track_sparse && stf_sparse_stats(tracked, &tiles_evaluated, &tiles_in_batches) != SS_OK) {
      failed = true;
      error = stf_last_error(tracked);
    }
    if (recorder) recorder->finish();  // the end of the stream stops every recording
    if (failed) {
      fprintf(stderr, "replay failed: %s\n", error.c_str());
      rc = 1;
    } else {
      printf("{\"file\": \"%s\", \"fft_size\": %d, \"decim\": %d, \"items_in_file\": %lld, \"frames\": %lld, \"batches\": %lld, "
             "\"candidates\": %lld, \"seconds\": %.6f, \"msamples_per_sec\": %.1f",
             opt.path.c_str(), cfg.fft_size, cfg.decim, (long long)reader.items(), frames, batches, candidates, seconds,
             seconds > 0 ? (double)frames * cfg.fft_size / seconds / 1e6 : 0.0);
      if (tracked) printf(", \"transmissions\": %lld, \"tracked_frames\": %lld", transmissions, tracked_frames);
      if (opt.track_sparse) printf(", \"tiles_evaluated\": %llu, \"tiles_in_batches\": %llu", (unsigned long long)tiles_evaluated, (unsigned long long)tiles_in_batches);
      if (rows) printf(", \"spectrogram_rows\": %lld", spectrogram_rows);
      if (rows && opt.spectrogram_ring) printf(", \"spectrogram_ring\": true");
      if (opt.fold_cs16) {
        ss_stats st{};
        st.size = sizeof(st);
        printf(", \"fold\": %s", ss_get_stats(ctx, &st) == SS_OK && (st.state & SS_STATE_FOLD) ? "true" : "false");
      }
      if (recorder) {
        const auto& c = recorder->counters();
        printf(", \"recorded_ranges\": %llu, \"recorded_samples\": %llu, \"published_items\": %llu, \"dropped_items\": %llu, "
               "\"record_h2d_bytes\": %llu, \"ignored_shifts_max\": %llu",
               (unsigned long long)c.ranges, (unsigned long long)c.samples, (unsigned long long)recorder->publishedItems(),
               (unsigned long long)recorder->droppedItems(), (unsigned long long)c.h2d_bytes, (unsigned long long)c.ignored_max);
      }
      printf("}\n");
    }
  } catch (const std::exception& e) {
    fprintf(stderr, "%s\n", e.what());
    rc = 1;
  }
  if (record_file && fclose(record_file) != 0) rc = 1;
  if (rows_file && fclose(rows_file) != 0) rc = 1;
  sgf_destroy(rows);
  stf_destroy(tracked);
  ss_feed_destroy(feed);
  ss_destroy(ctx);
  return rc;
}
