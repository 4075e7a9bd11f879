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

// ... of a batch whose call left no dB plane (st_create_sparse): ss_ctx::last_rel_rows, in the averager ring's buffer (track_digest_sparse.h)
ss::RingRows ring_rows(const ss_ctx* c, const digest_rows& r, int nframes) {
  ss::RingRows rows{};
  rows.rows = c->last_rel_rows;
  rows.thr = c->last_thr;
  rows.tail = r.d_tail[r.tail_cur].get();
  rows.n = c->n;
  rows.n_learn = c->last_n_learn;
  rows.tail_rows = r.tail_rows;
  rows.logq = c->last_rows_perm8 ? c->dif_logq : 0;
  // Defence only: rows settled since the call (settle_ring_db, ss_read_window's last_settled_lo / hi) follow a retune or ss_reset_noise,
  // and st_digest refuses both before it gets here (last_retunes; last_n = 0) — as things stand the range is empty and db_from / db_to
  // say last_rows_db for the whole batch. Kept so that the kernels read the rows by ss_read_window's rule whatever settles them one day.
  long long a = 0, b = 0;
  if (c->last_settled_lo) {
    a = (c->last_settled_lo - c->last_rel_rows) / (ptrdiff_t)c->n;
    b = (c->last_settled_hi - c->last_rel_rows) / (ptrdiff_t)c->n;
  }
  const ss::RingDbRange db = ss::ring_db_range(nframes, c->last_rows_db, a, b);
  rows.db_from = db.from;
  rows.db_to = db.to;
  return rows;
}

// the candidates' kernel over the last batch: lists on the device in, cand_best and cand_avg out
template <class Rows, class Kernel>
void launch_cand_best_of(Kernel kernel, const ss_ctx* c, const digest_rows& r, const Rows& rows, int nframes, const int32_t* cand_off, const int32_t* cand_idx,
                         int32_t* cand_best, float* cand_avg) {
  ss::CandBestArgsOf<Rows> a{};
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
  hipLaunchKernelGGL(kernel, dim3((unsigned)((size_t)nframes * a.tiles)), dim3(ss::kTrackTile), ss::blocked_lds_bytes(r.nrows, a.half), c->stream, a);
}
void launch_cand_best(const ss_ctx* c, const digest_rows& r, const ss::RelRows& rows, int nframes, const int32_t* cand_off, const int32_t* cand_idx, int32_t* cand_best,
                      float* cand_avg) {
  launch_cand_best_of(ss::k_best_blocked, c, r, rows, nframes, cand_off, cand_idx, cand_best, cand_avg);
}
void launch_cand_best(const ss_ctx* c, const digest_rows& r, const ss::RingRows& rows, int nframes, const int32_t* cand_off, const int32_t* cand_idx, int32_t* cand_best,
                      float* cand_avg) {
  launch_cand_best_of(ss::k_ring_best, c, r, rows, nframes, cand_off, cand_idx, cand_best, cand_avg);
}

// the batch's last rows into the other tail; flip_tail makes it the current one
unsigned save_tail_grid(const ss_ctx* c, const digest_rows& r) { return (unsigned)std::min<size_t>(((size_t)r.tail_rows * (size_t)c->n + 255) / 256, 1024); }
void launch_save_tail(const ss_ctx* c, const digest_rows& r, const ss::RelRows& rows, int nframes) {
  if (r.tail_rows == 0) return;
  hipLaunchKernelGGL(ss::k_save_tail, dim3(save_tail_grid(c, r)), dim3(256), 0, c->stream, rows, nframes, r.d_tail[r.tail_cur ^ 1].get());
}
void launch_save_tail(const ss_ctx* c, const digest_rows& r, const ss::RingRows& rows, int nframes) {
  if (r.tail_rows == 0) return;
  hipLaunchKernelGGL(ss::k_ring_tail, dim3(save_tail_grid(c, r)), dim3(256), 0, c->stream, rows, nframes, r.d_tail[r.tail_cur ^ 1].get());
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
  // st_create_sparse on a context that keeps no planes (include/specscan_track_digest_sparse.h, kernels: track_digest_sparse.h)
  bool sparse = false;
  int ncols = 0;                                         // ceil(n / 256): the tile columns
  ss::device_buffer<uint32_t> d_sp_mask;                 // [(n / 32) x max_batch] the replayed tiles' mask words: never read
  ss::device_buffer<int> d_sp_counts;                    // [max_batch] ... and their counts
  ss::device_buffer<int32_t> d_col_flag;                 // [ncols] the tile columns the batch's watch windows touch
  ss::device_buffer<unsigned long long> d_sp_evaluated;  // tiles the replay ran, since st_create_sparse / st_reset
  uint64_t sp_tiles_in_batches = 0;
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

// A sparse object, between the watch list and the peaks: avg in the tile columns the watch windows touch, by the batch's own detect
// stage once more — stf_replay_watch_tiles' recipe (host_track_feed.h has the list of what is switched off and why) on ss_ctx::last_det,
// with the tile of the form the batch took: its rows in bin order, or in the fold's order (scan_step.h: step_detect_layout).
// What the replay reads, and why it is all still there: st_digest holds the context's lock and has run flush_stages — no stage waits,
// nothing is in flight on the library's queues, and the next call, which is what moves the ring's window (place_ring), settles dB
// rows in place (settle_ring_db), rewrites the window in the other order (set_ring_form), raises the ceiling or rotates the planes,
// cannot start before the lock is released. So last_det's psd (the dB plane, or the rows a no-plane call left in the ring's buffer),
// hist_in / halo_psd (the rows before the batch), thr and pass are as the batch's own tiles saw them. A retune or ss_reset_noise
// since the batch settles rows too: st_digest has refused those already.
bool last_det_is_the_batch(const ss_ctx* c, int nframes) {
  const float* batch_rows = c->last_psd ? c->last_psd : c->last_rel_rows;
  return c->last_det_ok && c->last_det.psd == batch_rows && c->last_det.nframes == nframes && c->last_det.n == c->n && c->last_det.avg_sparse == c->last_avg;
}

int st_replay_watch_tiles(st_ctx* t, int nframes, int nwatch, int layout) {
  ss_ctx* c = t->scan;
  const int n = c->n;
  // (st_digest has checked last_det_is_the_batch before its first launch)
  hipLaunchKernelGGL(ss::k_digest_cols, dim3(1), dim3(256), 0, c->stream, (const int32_t*)t->d_watch.get(), nwatch, n, t->rows.group_size / 2, t->d_col_flag.get());
  ss::WatchTilesArgs wa{};
  wa.det = c->last_det;
  wa.det.maskbits = t->d_sp_mask.get();
  wa.det.counts = t->d_sp_counts.get();
  wa.det.rel_out = nullptr;
  wa.det.avg_out = const_cast<float*>(c->last_avg);
  wa.det.hist_out = nullptr;
  wa.det.hist_by_fft = 1;
  wa.det.segsum = nullptr;
  wa.det.halo_segsum = nullptr;
  wa.det.live = nullptr;
  wa.det.tile_list = nullptr;
  wa.det.stats = nullptr;
  wa.det.spec_partial = nullptr;
  wa.det.spec_prev_partial = nullptr;
  wa.det.spec_prev_sum = nullptr;
  wa.det.spec_prev_tiles = 0;
  wa.det.spec_m = wa.det.spec_n = 0;
#ifdef SS_DIAG
  wa.det.stamp_mid = nullptr;
  wa.det.cull_stats = nullptr;
#endif
  wa.col_flag = t->d_col_flag.get();
  wa.evaluated = t->d_sp_evaluated.get();
  const int frame_tiles = (nframes + wa.det.shift + kFusedTF - 1) / kFusedTF;
  const dim3 grid((unsigned)(frame_tiles * t->ncols));
  if (layout == 4) hipLaunchKernelGGL(ss::k_digest_tiles<4>, grid, dim3(256), 0, c->stream, wa);
  else if (layout == 3) hipLaunchKernelGGL(ss::k_digest_tiles<3>, grid, dim3(256), 0, c->stream, wa);
  else hipLaunchKernelGGL(ss::k_digest_tiles<0>, grid, dim3(256), 0, c->stream, wa);
  return SS_OK;
}

// st_create and st_create_sparse: allow_sparse = the context may lack SS_FLAG_KEEP_PLANES (the object is a sparse one if it does)
int st_create_any(ss_ctx* scan, const st_config* cfg, st_ctx** out, bool allow_sparse) {
  if (create_args_refused(scan, cfg, out, ST_ABI_VERSION)) return SS_ERR_INVALID;
  if (cfg->group_size < 0 || cfg->max_watch <= 0 || cfg->cand_cap <= 0) return obj_fail<st_ctx>(nullptr, SS_ERR_INVALID, "group_size >= 0, max_watch > 0 and cand_cap > 0 required");
  std::lock_guard<std::mutex> lock(scan->mtx);
  const bool sparse = allow_sparse && !(scan->cfg.flags & SS_FLAG_KEEP_PLANES);
  if (!allow_sparse && !(scan->cfg.flags & SS_FLAG_KEEP_PLANES)) return obj_fail<st_ctx>(nullptr, SS_ERR_INVALID, "the scan context needs SS_FLAG_KEEP_PLANES (the digest reads the kept dB and avg planes)");
  if (sparse && !scan->fused)
    return obj_fail<st_ctx>(nullptr, SS_ERR_INVALID, "sparse tracking needs the fused back end (grouping 21 x 21; this context has %d x %d): the unfused back end keeps no sparse avg plane",
                            scan->cfg.grouping_x, scan->cfg.grouping_y);
  if (sparse && scan->ref_nan) return obj_fail<st_ctx>(nullptr, SS_ERR_INVALID, "sparse tracking on a SS_FLAG_REFERENCE_NAN context: its NaN stage patches the planes behind the tiles");
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
  made.alloc(t->d_off, frames + 1).alloc(t->h_off, frames + 1).alloc(t->d_watch, mw).alloc(t->h_watch, mw);
  if (sparse) {
    t->sparse = true;
    t->ncols = (scan->n + ss::kWatchCol - 1) / ss::kWatchCol;
    const size_t words = ((size_t)scan->n / 32) * frames, plane = sizeof(float) * (size_t)scan->n * frames, ncols = (size_t)t->ncols;
    made.alloc(t->d_sp_mask, words).alloc(t->d_sp_counts, frames).alloc(t->d_col_flag, ncols).alloc(t->d_sp_evaluated, 1);
    made.then([&] { return hipMemsetAsync(t->d_sp_mask.get(), 0, sizeof(uint32_t) * words, scan->stream); });
    made.then([&] { return hipMemsetAsync(t->d_sp_counts.get(), 0, sizeof(int) * frames, scan->stream); });
    made.then([&] { return hipMemsetAsync(t->d_col_flag.get(), 0, sizeof(int32_t) * ncols, scan->stream); });
    made.then([&] { return hipMemsetAsync(t->d_sp_evaluated.get(), 0, sizeof(unsigned long long), scan->stream); });
    // every sparse plane to NaN, once (all bytes 0xff), as stf_create_sparse does: a cell of a watch window the replay failed to write
    // would be a NaN peak, not a plausible value some earlier batch left there
    made.then([&] {
      flush_stages(scan);
      return hipSuccess;
    });
    for (int k = 0; k < scan->nbuf; ++k) made.then([&] { return hipMemsetAsync(scan->d_avg2[k], 0xff, plane, scan->stream); });
  }
  made.then([&] { return hipStreamSynchronize(scan->stream); });
  if (!made.ok()) {
    delete t;
    return obj_fail<st_ctx>(nullptr, SS_ERR_NOMEM, "allocating the digest's buffers failed: %s", hipGetErrorString(made.error()));
  }
  *out = t;
  return SS_OK;
}

}  // namespace

extern "C" {

int st_create(ss_ctx* scan, const st_config* cfg, st_ctx** out) { return st_create_any(scan, cfg, out, false); }

int st_create_sparse(ss_ctx* scan, const st_config* cfg, st_ctx** out) { return st_create_any(scan, cfg, out, true); }

int st_sparse_stats(st_ctx* t, uint64_t* tiles_evaluated, uint64_t* tiles_in_batches) {
  if (!t) return SS_ERR_INVALID;
  if (!tiles_evaluated || !tiles_in_batches) return obj_fail(t, SS_ERR_INVALID, "null argument");
  ss_ctx* c = t->scan;
  std::lock_guard<std::mutex> lock(c->mtx);
  if (!t->sparse) return obj_fail(t, SS_ERR_INVALID, "not a sparse object: the scan context keeps its planes (st_create, or st_create_sparse with SS_FLAG_KEEP_PLANES), nothing is replayed");
  unsigned long long ev = 0;
  ST_HIP(t, hipSetDevice(c->cfg.device_id));
  ST_HIP(t, hipMemcpyAsync(&ev, t->d_sp_evaluated.get(), sizeof(ev), hipMemcpyDeviceToHost, c->stream));
  ST_HIP(t, hipStreamSynchronize(c->stream));
  *tiles_evaluated = ev;
  *tiles_in_batches = t->sp_tiles_in_batches;
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
  if (t->sparse) ST_HIP(t, hipMemsetAsync(t->d_sp_evaluated.get(), 0, sizeof(unsigned long long), c->stream));
  ST_HIP(t, hipStreamSynchronize(c->stream));
  t->sp_tiles_in_batches = 0;
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
  // (a sparse object also digests a call that left no dB plane: its rows are in the averager ring's buffer, track_digest_sparse.h)
  const ss::RowsChoice src = ss::decide_rows_source(c->last_psd != nullptr, c->last_rel_rows != nullptr, c->last_rows_perm8, c->dif_logq);  // (rows_source.h)
  const bool ring_call = t->sparse && c->fused && src.source == ss::kRowsRing;
  if (!c->last_avg || (c->fused && ((!c->last_psd && !ring_call) || !c->last_thr))) return obj_fail(t, SS_ERR_INVALID, "the last batch left no dB plane, avg plane or noise ceiling to digest");
  // (defence only, see ring_rows: nothing settles rows between a call and its digest that is not refused above)
  if (ring_call && c->last_settled_lo && c->last_settled_lo > c->last_rel_rows && c->last_settled_hi < c->last_rel_rows + (size_t)nframes * (size_t)n)
    return obj_fail(t, SS_ERR_INVALID, "rows in the middle of the last batch were settled since it ran: nothing a call leaves looks like that");
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
  if (t->sparse && !last_det_is_the_batch(c, nframes)) return obj_fail(t, SS_ERR_INVALID, "sparse digest: the detect stage launched last is not this batch's");
  const ss::RelRows rows = ring_call ? ss::RelRows{} : rel_rows(c, t->rows);  // one of the two sources
  const ss::RingRows ring = ring_call ? ring_rows(c, t->rows, nframes) : ss::RingRows{};
  uint64_t d2h = 0;
  if (ncand > 0) {
    ST_HIP(t, hipMemcpyAsync(t->d_off.get(), h_off, sizeof(int32_t) * ((size_t)nframes + 1), hipMemcpyHostToDevice, c->stream));
    ST_HIP(t, hipMemcpyAsync(t->d_idx.get(), t->h_idx.get(), sizeof(int32_t) * (size_t)ncand, hipMemcpyHostToDevice, c->stream));
    if (ring_call) launch_cand_best(c, t->rows, ring, nframes, t->d_off.get(), t->d_idx.get(), t->d_best.get(), t->d_cavg.get());
    else launch_cand_best(c, t->rows, rows, nframes, t->d_off.get(), t->d_idx.get(), t->d_best.get(), t->d_cavg.get());
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
    if (t->sparse) {  // avg where the windows lie: nothing but the tiles with hits has written the sparse plane
      const int st_replay = st_replay_watch_tiles(t, nframes, nwatch, src.layout);
      if (st_replay != SS_OK) return st_replay;
    }
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
  if (ring_call) launch_save_tail(c, t->rows, ring, nframes);
  else launch_save_tail(c, t->rows, rows, nframes);
  ST_HIP(t, hipGetLastError());
  ST_HIP(t, stream_wait(c->stream));
  flip_tail(t->rows);
  t->seen_batch = c->batch_no;
  if (t->sparse) t->sp_tiles_in_batches += (uint64_t)((nframes + c->last_det.shift + kFusedTF - 1) / kFusedTF) * (uint64_t)t->ncols;
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
