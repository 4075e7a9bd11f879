// host_track.h — the tracking digest (include/specscan_track.h, st_*; kernels: track_digest.h, track_digest_blocked.h): what the
// host-side signal tracker reads of the last batch's rel and avg planes, computed next to them. digest_rows and its launch helpers
// are shared with the tracked feed (host_track_feed.h). Part of specscan.hip's translation unit.
#pragma once

namespace {

// What st_ctx and stf_ctx share: the rel rows getBestIndex looks at, and the ones among them that lie before a batch.
struct digest_rows {
  int group_size = 0;
  float start_level = 0.0f;
  int nrows = 1;      // ceil(grouping_y / 2): the rel rows getBestIndex looks at
  int tail_rows = 0;  // nrows - 1: how many of them can lie before a batch
  ss::device_buffer<float> d_tail[2];  // [tail_rows][n] each; [tail_cur] holds the rows before the next batch, the other one is written by the digest
  int tail_cur = 0;
};

// create time: the row count, and whether a tile of the candidates' kernel (track_digest_blocked.h) fits LDS; the message goes to err
int digest_rows_plan(digest_rows& r, const ss_ctx* scan, int group_size, float start_level, char* err) {
  r.group_size = group_size;
  r.start_level = start_level;
  r.nrows = (scan->cfg.grouping_y + 1) / 2;
  r.tail_rows = r.nrows - 1;
  const size_t lds = ss::blocked_lds_bytes(r.nrows, group_size / 2);
  if (lds > 65536) return fail_to(err, SS_ERR_INVALID, "group_size %d with %d rows needs %zu bytes of LDS per tile (64 KiB at most)", group_size, r.nrows, lds);
  return SS_OK;
}

size_t tail_floats(const digest_rows& r, const ss_ctx* scan) { return (size_t)std::max(1, r.tail_rows) * (size_t)scan->n; }

hipError_t tails_alloc(digest_rows& r, const ss_ctx* scan) { return ss::hip_steps().alloc(r.d_tail[0], tail_floats(r, scan)).alloc(r.d_tail[1], tail_floats(r, scan)).error(); }

// both tails to zero on the context's stream (the caller waits for it)
hipError_t tails_zero(const digest_rows& r, const ss_ctx* scan) {
  hipError_t e = hipSuccess;
  for (int k = 0; k < 2 && e == hipSuccess; ++k) e = hipMemsetAsync(r.d_tail[k].get(), 0, sizeof(float) * tail_floats(r, scan), scan->stream);
  return e;
}

// the rel rows of the last batch and in front of it
ss::RelRows rel_rows(const ss_ctx* c, const digest_rows& r) {
  ss::RelRows rows{};
  rows.n = c->n;
  rows.n_learn = c->last_n_learn;
  rows.tail_rows = r.tail_rows;
  rows.tail = r.d_tail[r.tail_cur].get();
  if (c->fused) {
    rows.psd = c->last_psd;
    rows.thr = c->last_thr;
  } else {
    rows.rel = c->d_rel + (size_t)(c->cfg.grouping_y - 1) * c->n;
  }
  return rows;
}

// the candidates' kernel over the last batch: lists on the device in, cand_best and cand_avg out
void launch_cand_best(const ss_ctx* c, const digest_rows& r, const ss::RelRows& rows, int nframes, const int32_t* cand_off, const int32_t* cand_idx, int32_t* cand_best,
                      float* cand_avg) {
  ss::CandBestArgs a{};
  a.rows = rows;
  a.avg = c->last_avg;
  a.cand_off = cand_off;
  a.cand_idx = cand_idx;
  a.cand_best = cand_best;
  a.cand_avg = cand_avg;
  a.nframes = nframes;
  a.tiles = (c->n + ss::kTrackTile - 1) / ss::kTrackTile;
  a.half = r.group_size / 2;
  a.nrows = r.nrows;
  a.width = ss::kTrackTile + 2 * a.half;
  a.start_level = r.start_level;
  hipLaunchKernelGGL(ss::k_best_blocked, dim3((unsigned)((size_t)nframes * a.tiles)), dim3(ss::kTrackTile), ss::blocked_lds_bytes(r.nrows, a.half), c->stream, a);
}

// the batch's last rows into the other tail; flip_tail makes it the current one
void launch_save_tail(const ss_ctx* c, const digest_rows& r, const ss::RelRows& rows, int nframes) {
  if (r.tail_rows == 0) return;
  const size_t total = (size_t)r.tail_rows * (size_t)c->n;
  hipLaunchKernelGGL(ss::k_save_tail, dim3((unsigned)std::min<size_t>((total + 255) / 256, 1024)), dim3(256), 0, c->stream, rows, nframes, r.d_tail[r.tail_cur ^ 1].get());
}

void flip_tail(digest_rows& r) {
  if (r.tail_rows > 0) r.tail_cur ^= 1;
}

}  // namespace

struct SS_HIDDEN st_ctx {
  ss_ctx* scan = nullptr;
  st_config cfg{};
  digest_rows rows;
  unsigned long long seen_batch = 0;  // ss_ctx::batch_no of the last batch digested (or at st_create / st_reset)
  ss::device_buffer<int32_t> d_off, d_idx, d_best, d_watch, d_pidx;
  ss::device_buffer<float> d_cavg, d_pavg;
  ss::pinned_buffer<int32_t> h_off, h_idx, h_best, h_watch, h_pidx;
  ss::pinned_buffer<float> h_cavg, h_pavg;
  size_t peak_cap = 0;  // elements of d_pidx / d_pavg / h_pidx / h_pavg (grown to nframes x nwatch as needed)
  size_t cand_alloc = 0;  // elements of d_idx / d_best / d_cavg and their host twins (grown as needed, cfg.cand_cap at most)
  std::vector<int32_t> merged;  // the watch list being formed
  std::vector<uint8_t> mark;    // [n], all zero between digests
  char err[512] = "";
};

namespace {

#define ST_HIP(ctx, call)                                                                                  \
  do {                                                                                                     \
    hipError_t e_ = (call);                                                                                \
    if (e_ != hipSuccess) return obj_fail(ctx, SS_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
  } while (0)

// (cfg.cand_cap is a limit, not an allocation: an adapter that cannot know its traffic states fft_size x max_batch and pays for what comes)
int st_grow_cands(st_ctx* t, size_t need) {
  if (need <= t->cand_alloc) return SS_OK;
  const size_t cap = std::min((size_t)t->cfg.cand_cap, std::max({need, t->cand_alloc * 2, (size_t)4096}));
  t->cand_alloc = 0;  // (and stays 0 if an allocation fails: the next digest grows again)
  ss::reset_all(t->d_idx, t->d_best, t->d_cavg, t->h_idx, t->h_best, t->h_cavg);
  ss::hip_steps grown;
  grown.alloc(t->d_idx, cap).alloc(t->d_best, cap).alloc(t->d_cavg, cap).alloc(t->h_idx, cap).alloc(t->h_best, cap).alloc(t->h_cavg, cap);
  if (!grown.ok()) return obj_fail(t, SS_ERR_HIP, "%s failed: %s", grown.what(), hipGetErrorString(grown.error()));
  t->cand_alloc = cap;
  return SS_OK;
}

int st_grow_peaks(st_ctx* t, size_t need) {
  if (need <= t->peak_cap) return SS_OK;
  const size_t cap = std::max(need, t->peak_cap * 2);
  t->peak_cap = 0;
  ss::reset_all(t->d_pidx, t->d_pavg, t->h_pidx, t->h_pavg);
  ss::hip_steps grown;
  grown.alloc(t->d_pidx, cap).alloc(t->d_pavg, cap).alloc(t->h_pidx, cap).alloc(t->h_pavg, cap);
  if (!grown.ok()) return obj_fail(t, SS_ERR_HIP, "%s failed: %s", grown.what(), hipGetErrorString(grown.error()));
  t->peak_cap = cap;
  return SS_OK;
}

}  // namespace

extern "C" {

int st_create(ss_ctx* scan, const st_config* cfg, st_ctx** out) {
  if (create_args_refused(scan, cfg, out, ST_ABI_VERSION)) return SS_ERR_INVALID;
  if (cfg->group_size < 0 || cfg->max_watch <= 0 || cfg->cand_cap <= 0) return obj_fail<st_ctx>(nullptr, SS_ERR_INVALID, "group_size >= 0, max_watch > 0 and cand_cap > 0 required");
  std::lock_guard<std::mutex> lock(scan->mtx);
  if (!(scan->cfg.flags & SS_FLAG_KEEP_PLANES)) return obj_fail<st_ctx>(nullptr, SS_ERR_INVALID, "the scan context needs SS_FLAG_KEEP_PLANES (the digest reads the kept dB and avg planes)");
  digest_rows rows;
  if (const int st = digest_rows_plan(rows, scan, cfg->group_size, cfg->start_level, create_err<st_ctx>()); st != SS_OK) return st;
  st_ctx* t = new (std::nothrow) st_ctx();
  if (!t) return obj_fail<st_ctx>(nullptr, SS_ERR_NOMEM, "out of memory");
  t->scan = scan;
  t->cfg = *cfg;
  t->rows = std::move(rows);
  t->seen_batch = scan->batch_no;
  const size_t frames = (size_t)scan->cfg.max_batch, mw = (size_t)cfg->max_watch;
  ss::hip_steps made;
  made.then([&] { return hipSetDevice(scan->cfg.device_id); }).then([&] { return tails_alloc(t->rows, scan); }).then([&] { return tails_zero(t->rows, scan); });
  made.alloc(t->d_off, frames + 1).alloc(t->h_off, frames + 1).alloc(t->d_watch, mw).alloc(t->h_watch, mw).then([&] { return hipStreamSynchronize(scan->stream); });
  if (!made.ok()) {
    delete t;
    return obj_fail<st_ctx>(nullptr, SS_ERR_NOMEM, "allocating the digest's buffers failed: %s", hipGetErrorString(made.error()));
  }
  *out = t;
  return SS_OK;
}

void st_destroy(st_ctx* t) {
  if (!t) return;
  {
    std::lock_guard<std::mutex> lock(t->scan->mtx);
    (void)hipSetDevice(t->scan->cfg.device_id);
    (void)hipStreamSynchronize(t->scan->stream);
  }
  delete t;
}

const char* st_last_error(const st_ctx* t) { return t ? t->err : create_err<st_ctx>(); }

int st_reset(st_ctx* t) {
  if (!t) return SS_ERR_INVALID;
  ss_ctx* c = t->scan;
  std::lock_guard<std::mutex> lock(c->mtx);
  ST_HIP(t, hipSetDevice(c->cfg.device_id));
  ST_HIP(t, hipMemsetAsync(t->rows.d_tail[t->rows.tail_cur].get(), 0, sizeof(float) * tail_floats(t->rows, c), c->stream));
  ST_HIP(t, hipStreamSynchronize(c->stream));
  t->seen_batch = c->batch_no;
  return SS_OK;
}

int st_digest(st_ctx* t, const int32_t* cand_off, const int32_t* cand_idx, const int32_t* keys, int32_t nkeys, st_result* out) {
  if (!t) return SS_ERR_INVALID;
  if (!cand_off || !out || nkeys < 0 || (nkeys > 0 && !keys)) return obj_fail(t, SS_ERR_INVALID, "null argument");
  ss_ctx* c = t->scan;
  std::lock_guard<std::mutex> lock(c->mtx);
  const int n = c->n, nframes = c->last_n;
  if (nframes <= 0) return obj_fail(t, SS_ERR_INVALID, "no batch processed since ss_create / ss_reset / ss_reset_noise");
  if (c->batch_no == t->seen_batch) return obj_fail(t, SS_ERR_INVALID, "the last batch has been digested already (or none has run since st_create / st_reset)");
  if (c->batch_no != t->seen_batch + 1)
    return obj_fail(t, SS_ERR_INVALID, "%llu batches went by without st_digest: the kept rel rows are stale until st_reset", c->batch_no - t->seen_batch - 1);
  if (c->last_retunes != c->retunes) return obj_fail(t, SS_ERR_INVALID, "ss_set_frequency_range since the last batch: its noise ceiling is not the current one");
  if (!c->last_avg || (c->fused && (!c->last_psd || !c->last_thr))) return obj_fail(t, SS_ERR_INVALID, "the last batch left no dB plane, avg plane or noise ceiling to digest");
  // the lists: offsets clipped to what the batch's call could write (SS_ERR_CAND_OVERFLOW leaves truncated lists), bins checked
  int32_t* const h_off = t->h_off.get();
  const int64_t cap = c->last_cand_cap > 0 ? c->last_cand_cap : 0;
  int64_t prev = 0;
  for (int f = 0; f <= nframes; ++f) {
    int64_t o = cand_off[f];
    if (o < prev || (f == 0 && o != 0)) return obj_fail(t, SS_ERR_INVALID, "cand_off is not a list of offsets (frame %d)", f);
    prev = o;
    if (o > cap) o = cap;
    h_off[f] = (int32_t)o;
  }
  const int ncand = h_off[nframes];
  if (ncand > t->cfg.cand_cap) return obj_fail(t, SS_ERR_INVALID, "%d candidates > cand_cap %d", ncand, t->cfg.cand_cap);
  if (ncand > 0 && !cand_idx) return obj_fail(t, SS_ERR_INVALID, "null argument");
  ST_HIP(t, hipSetDevice(c->cfg.device_id));
  if (const int st = st_grow_cands(t, (size_t)ncand); st != SS_OK) return st;
  for (int j = 0; j < ncand; ++j) {
    const int32_t b = cand_idx[j];
    if (b < 0 || b >= n) return obj_fail(t, SS_ERR_INVALID, "candidate %d: bin %d outside [0, %d)", j, b, n);
    t->h_idx.get()[j] = b;
  }
  if (nkeys > t->cfg.max_watch) return obj_fail(t, SS_ERR_INVALID, "%d keys > max_watch %d", nkeys, t->cfg.max_watch);
  for (int k = 0; k < nkeys; ++k)
    if (keys[k] < 0 || keys[k] >= n) return obj_fail(t, SS_ERR_INVALID, "key %d: bin %d outside [0, %d)", k, keys[k], n);
  flush_stages(c);
  const ss::RelRows rows = rel_rows(c, t->rows);
  uint64_t d2h = 0;
  if (ncand > 0) {
    ST_HIP(t, hipMemcpyAsync(t->d_off.get(), h_off, sizeof(int32_t) * ((size_t)nframes + 1), hipMemcpyHostToDevice, c->stream));
    ST_HIP(t, hipMemcpyAsync(t->d_idx.get(), t->h_idx.get(), sizeof(int32_t) * (size_t)ncand, hipMemcpyHostToDevice, c->stream));
    launch_cand_best(c, t->rows, rows, nframes, t->d_off.get(), t->d_idx.get(), t->d_best.get(), t->d_cavg.get());
    ST_HIP(t, hipGetLastError());
    ST_HIP(t, hipMemcpyAsync(t->h_best.get(), t->d_best.get(), sizeof(int32_t) * (size_t)ncand, hipMemcpyDeviceToHost, c->stream));
    ST_HIP(t, hipMemcpyAsync(t->h_cavg.get(), t->d_cavg.get(), sizeof(float) * (size_t)ncand, hipMemcpyDeviceToHost, c->stream));
    ST_HIP(t, stream_wait(c->stream));
    d2h += 8ull * (uint64_t)ncand;
  }
  // the watch list: every key the tracker can hold while it walks the batch
  // (one flag per bin and a walk over the bins: a batch brings hundreds of thousands of candidates and a handful of distinct keys)
  std::vector<int32_t>& w = t->merged;
  w.clear();
  t->mark.resize((size_t)n, 0);
  for (int k = 0; k < nkeys; ++k) t->mark[(size_t)keys[k]] = 1;
  bool sane = true;
  for (int j = 0; j < ncand; ++j) {
    const uint32_t b = (uint32_t)t->h_best.get()[j];
    if (b < (uint32_t)n) t->mark[b] = 1;
    else sane = false;
  }
  for (int b = 0; b < n; ++b)
    if (t->mark[(size_t)b]) {
      w.push_back(b);
      t->mark[(size_t)b] = 0;
    }
  if (!sane) return obj_fail(t, SS_ERR_HIP, "the candidates' kernel returned a bin outside [0, %d)", n);
  const int nwatch = (int)w.size();
  if (nwatch > t->cfg.max_watch) return obj_fail(t, SS_ERR_INVALID, "%d watch keys > max_watch %d", nwatch, t->cfg.max_watch);
  if (nwatch > 0) {
    const int st = st_grow_peaks(t, (size_t)nframes * (size_t)nwatch);
    if (st != SS_OK) return st;
    memcpy(t->h_watch.get(), w.data(), sizeof(int32_t) * (size_t)nwatch);
    ST_HIP(t, hipMemcpyAsync(t->d_watch.get(), t->h_watch.get(), sizeof(int32_t) * (size_t)nwatch, hipMemcpyHostToDevice, c->stream));
    ss::WindowPeaksArgs p{};
    p.avg = c->last_avg;
    p.watch = t->d_watch.get();
    p.peak_idx = t->d_pidx.get();
    p.peak_avg = t->d_pavg.get();
    p.n = n;
    p.nframes = nframes;
    p.nwatch = nwatch;
    p.half = t->rows.group_size / 2;
    const size_t items = (size_t)nframes * (size_t)nwatch;
    hipLaunchKernelGGL(ss::k_window_peaks, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, c->stream, p);
    ST_HIP(t, hipGetLastError());
    ST_HIP(t, hipMemcpyAsync(t->h_pidx.get(), t->d_pidx.get(), sizeof(int32_t) * items, hipMemcpyDeviceToHost, c->stream));
    ST_HIP(t, hipMemcpyAsync(t->h_pavg.get(), t->d_pavg.get(), sizeof(float) * items, hipMemcpyDeviceToHost, c->stream));
    d2h += 8ull * (uint64_t)items;
  }
  launch_save_tail(c, t->rows, rows, nframes);
  ST_HIP(t, hipGetLastError());
  ST_HIP(t, stream_wait(c->stream));
  flip_tail(t->rows);
  t->seen_batch = c->batch_no;
  out->nframes = nframes;
  out->ncand = ncand;
  out->nwatch = nwatch;
  out->cand_best = t->h_best.get();
  out->cand_avg = t->h_cavg.get();
  out->watch = t->h_watch.get();
  out->peak_idx = t->h_pidx.get();
  out->peak_avg = t->h_pavg.get();
  out->d2h_bytes = d2h;
  return SS_OK;
}

}  // extern "C"
