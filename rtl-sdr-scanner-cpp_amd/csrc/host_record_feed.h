// host_record_feed.h — the recorder bound to the feed (include/specscan_record_feed.h, srf_*): a channeliser of its own, run on the
// held slot's upload. Part of specscan.hip's translation unit, behind host_feed.h.
// Which slot is held is the feed's ring's (feed_ring.h), under the scan context's mutex; the channeliser, its planes and the pinned
// results are the recorder's, under rec_mtx, which is held for a whole srf_record so that the scan context's mutex is not: a
// producer thread acquires and submits the other slots meanwhile. Lock order: rec_mtx, then the context's.
#pragma once

struct SS_HIDDEN srf_ctx : feed_rider {
  srf_config cfg{};
  std::mutex rec_mtx;
  sc_ctx* chan = nullptr;
  ss::hip_stream stream;  // the copies of the outputs, behind sc_sync
  int cap = 0;
  ss::device_buffer<int8_t> d_i8;
  ss::device_buffer<float> d_cf32;
  ss::pinned_buffer<int8_t> h_i8;
  ss::pinned_buffer<float> h_cf32;
  ss::pinned_buffer<int32_t> h_counts, h_rc;

  ~srf_ctx() {
    if (chan) sc_destroy(chan);
  }
};

extern "C" {

int srf_create(ss_feed* f, const srf_config* cfg, srf_ctx** out) {
  if (create_args_refused(f, cfg, out, SRF_ABI_VERSION)) return SS_ERR_INVALID;
  ss_ctx* c = f->c;
  std::lock_guard<std::mutex> lock(c->mtx);
  if (c->cfg.decim != 1 && !f->items)
    return obj_fail<srf_ctx>(nullptr, SS_ERR_INVALID, "the scan context has decim %d: an ordinary feed takes only the frames the scan reads, there is no stream to record from (ss_feed_create_items keeps the whole items)", c->cfg.decim);
  if (feed_already_has<srf_ctx>(f->recorder, "a recorder") || feed_busy<srf_ctx>(f)) return SS_ERR_INVALID;
  int32_t max_samples = 0;  // of the recorded stream: whole items (decim is 1 on the device route)
  if (!chan_ranges::item_samples(c->cfg.max_batch, c->n, c->cfg.decim, &max_samples))
    return obj_fail<srf_ctx>(nullptr, SS_ERR_INVALID, "max_batch * N * decim = %lld samples do not fit one channeliser call", (long long)c->cfg.max_batch * c->n * c->cfg.decim);
  srf_ctx* t = new (std::nothrow) srf_ctx();
  if (!t) return obj_fail<srf_ctx>(nullptr, SS_ERR_NOMEM, "out of memory");
  t->scan = c;
  t->feed = f;
  t->cfg = *cfg;
  sc_config sc;
  sc_default_config(&sc, c->cfg.sample_rate, cfg->bandwidth);
  sc.threshold = cfg->threshold;
  sc.channels = cfg->channels;
  sc.max_samples = max_samples;
  sc.pack_scale = cfg->pack_scale;
  sc.device_id = c->cfg.device_id;
  int st = sc_create(&sc, &t->chan);
  if (st != SS_OK) {
    obj_fail<srf_ctx>(nullptr, st, "sc_create: %s", sc_last_error(nullptr));
    delete t;
    return st;
  }
  st = sc_set_input_format(t->chan, c->cfg.in_format, c->cfg.int_scale);
  if (st != SS_OK) {
    obj_fail<srf_ctx>(nullptr, st, "sc_set_input_format: %s", sc_last_error(t->chan));
    delete t;
    return st;
  }
  t->cap = sc_output_capacity(t->chan, max_samples);
  const size_t plane = (size_t)2 * (size_t)t->cap * (size_t)cfg->channels;
  ss::hip_steps made;
  made.then([&] { return hipSetDevice(c->cfg.device_id); }).stream(t->stream);
  made.alloc(t->d_i8, plane).alloc(t->h_i8, plane);
  if (cfg->want_cf32) made.alloc(t->d_cf32, plane).alloc(t->h_cf32, plane);
  made.alloc(t->h_counts, SC_MAX_CHANNELS).alloc(t->h_rc, SC_MAX_RANGES);
  if (!made.ok()) {
    delete t;
    return obj_fail<srf_ctx>(nullptr, SS_ERR_NOMEM, "allocating the recorder's buffers failed: %s", hipGetErrorString(made.error()));
  }
  f->recorder = t;
  *out = t;
  return SS_OK;
}

void srf_destroy(srf_ctx* t) {
  if (!t) return;
  {
    std::lock_guard<std::mutex> rec(t->rec_mtx);
    std::lock_guard<std::mutex> lock(t->scan->mtx);
    if (t->feed) {
      (void)t->feed->ring.let_go();  // the held slot, if there is one, goes back to the producer (without a recorder nothing is held)
      t->feed->recorder = nullptr;
    }
    (void)hipSetDevice(t->scan->cfg.device_id);
    if (t->stream) (void)hipStreamSynchronize(t->stream);
  }
  delete t;
}

const char* srf_last_error(const srf_ctx* t) { return t ? t->err : create_err<srf_ctx>(); }

int srf_release(srf_ctx* t) {
  if (!t) return SS_ERR_INVALID;
  std::lock_guard<std::mutex> rec(t->rec_mtx);
  std::lock_guard<std::mutex> lock(t->scan->mtx);
  if (feed_destroyed(t)) return SS_ERR_INVALID;
  if (t->feed->ring.let_go() != ss::ring_refusal::none) return obj_fail(t, SS_ERR_INVALID, "no batch is held: collect one first");
  return SS_OK;
}

int srf_record(srf_ctx* t, const sc_range* ranges, int32_t nranges, srf_result* out) {
  if (!t) return SS_ERR_INVALID;
  if (!out || nranges < 0 || (nranges > 0 && !ranges)) return obj_fail(t, SS_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> rec(t->rec_mtx);
  const void* d_in = nullptr;
  const void* h_items = nullptr;  // an items feed: the held slot's pinned items, uploaded as far as the ranges read them
  int nsamples = 0;
  {
    std::lock_guard<std::mutex> lock(t->scan->mtx);
    if (feed_destroyed(t)) return SS_ERR_INVALID;
    ss_feed* f = t->feed;
    if (f->ring.held() < 0) return obj_fail(t, SS_ERR_INVALID, "no batch is held: collect one first");
    const ss_feed_slot& s = f->slots[(size_t)f->ring.held()];
    d_in = s.d_in.get();  // the collect has waited for the batch's chain, which waited for the upload
    if (f->items) h_items = s.h_in.get();
    nsamples = s.nframes * t->scan->n * (f->items ? t->scan->cfg.decim : 1);  // (srf_create: fits)
  }
  const int nch = t->cfg.channels;
  int8_t *const d_i8 = t->d_i8.get(), *const h_i8 = t->h_i8.get();
  float *const d_cf32 = t->d_cf32.get(), *const h_cf32 = t->h_cf32.get();
  int32_t* const h_counts = t->h_counts.get();
  out->nsamples = nsamples;
  out->cap = t->cap;
  out->counts = h_counts;
  out->range_counts = t->h_rc.get();
  out->out_i8 = h_i8;
  out->out_cf32 = t->cfg.want_cf32 ? h_cf32 : nullptr;
  out->h2d_bytes = 0;
  for (int ch = 0; ch < nch; ++ch) h_counts[ch] = 0;
  if (nranges > 0) {
    // the held slot is not acquired and not submitted to while it is held, so its d_in and its pinned items stand still without
    // the context's lock
    uint64_t uploaded = 0;
    int st = h_items ? sc_process_ranges_upload(t->chan, h_items, nsamples, ranges, nranges, d_i8, d_cf32, h_counts, t->h_rc.get(), t->cap, &uploaded)
                     : sc_process_ranges_device(t->chan, d_in, nsamples, ranges, nranges, d_i8, d_cf32, h_counts, t->h_rc.get(), t->cap);
    if (st != SS_OK) return obj_fail(t, st, "%s", sc_last_error(t->chan));
    st = sc_sync(t->chan);  // (the uploads have read the pinned items by now: the slot may go)
    if (st != SS_OK) return obj_fail(t, st, "%s", sc_last_error(t->chan));
    out->h2d_bytes = uploaded;
    hipError_t e = hipSetDevice(t->scan->cfg.device_id);
    for (int ch = 0; ch < nch && e == hipSuccess; ++ch) {
      const size_t n = (size_t)(h_counts[ch] < t->cap ? h_counts[ch] : t->cap), at = (size_t)2 * (size_t)t->cap * (size_t)ch;
      if (n == 0) continue;
      e = hipMemcpyAsync(h_i8 + at, d_i8 + at, 2 * n, hipMemcpyDeviceToHost, t->stream);
      if (e == hipSuccess && t->cfg.want_cf32) e = hipMemcpyAsync(h_cf32 + at, d_cf32 + at, sizeof(float) * 2 * n, hipMemcpyDeviceToHost, t->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
    if (e != hipSuccess) return obj_fail(t, SS_ERR_HIP, "copying the recorded samples failed: %s", hipGetErrorString(e));
  }
  std::lock_guard<std::mutex> lock(t->scan->mtx);
  if (t->feed) (void)t->feed->ring.let_go();
  return SS_OK;
}

}  // extern "C"
