// host_spectrogram_feed.h — the spectrogram rows of the feed (include/specscan_spectrogram_feed.h, sgf_*): the reference's per-frame
// send gate on the host (spectrogram_gate.h) and its arithmetic, in its order, in one kernel behind every batch (spectrogram_rows.h).
// Everything here is the scan context's, under its mutex. The kernel is on the context's stream behind flush_stages, like the tracked
// feed's digest (host_track_feed.h says why the next batch's chain cannot overtake it): it reads c->last_psd before the next batch
// rotates the planes. Part of specscan.hip's translation unit, behind host_feed.h.
//
// sgf_create_ring (include/specscan_spectrogram_feed_ring.h): the same object on a context without SS_FLAG_SPECTROGRAM, whose batches
// may keep no dB plane (stf_wants_no_plane_calls). sgf_enqueue asks rows_source.h where the batch left its dB values: the plane, the
// ring's buffer in bin order (k_spec_rows over last_rel_rows, the same pitch) or in the fold's order (spectrogram_rows_ring.h). The
// kernel is then one more reader of a no-plane batch's rows on the context's stream: host_track_feed.h has the ordering argument.
#pragma once

namespace {
struct sgf_container {  // Spectrogram::Container (spectrogram.h:10-16), one per centre frequency: the sum on the device, the rest here
  int32_t center = 0;
  ss::device_buffer<float> d_sum;
  int64_t last_send = 0;
  int32_t have_last = 0;  // the container's first frame stamps last_send
  int32_t count = 0;      // m_counter
};

struct sgf_slot {
  ss::device_buffer<int8_t> d_rows;
  ss::device_buffer<float> d_mean;
  ss::pinned_buffer<int8_t> h_rows;
  ss::pinned_buffer<float> h_mean;
  ss::pinned_buffer<int64_t> h_time;
  ss::pinned_buffer<int32_t> h_frame, h_count;
  int32_t nrows = 0, frequency = 0, open_count = 0;
};
}  // namespace

struct SS_HIDDEN sgf_ctx : feed_rider {
  sgf_config cfg{};
  int size = 0, log2_m = 0;
  bool ring = false;  // sgf_create_ring: a batch's rows may come from the averager ring's buffer
  std::vector<sgf_container> containers;
  std::vector<sgf_slot> slots;
};

namespace {

bool sgf_reads_ring_rows(const ss_feed* f) { return static_cast<const sgf_ctx*>(f->spectrogram)->ring; }

sgf_container* sgf_container_for(sgf_ctx* t, int32_t center) {
  for (auto& g : t->containers)
    if (g.center == center) return &g;
  return nullptr;
}

// ss_feed_submit, under the context's lock, in front of the upload: the gate of the centre in force over the batch's clock, on
// copies. A refusal leaves every state as it was.
int sgf_plan_batch(ss_feed* f, int nframes, const int64_t* t_ms, sgf_plan* plan) {
  sgf_ctx* t = static_cast<sgf_ctx*>(f->spectrogram);
  ss_ctx* c = f->c;
  if (!t_ms) return fail(c, SS_ERR_INVALID, "ss_feed_submit without t_ms: the feed's spectrogram rows close on the frames' clock");
  plan->center = (c->range_lo + c->range_hi) / 2;
  if (const sgf_container* g = sgf_container_for(t, plan->center)) {
    plan->last_send = g->last_send;
    plan->have_last = g->have_last;
  }
  const int rows = ss::spectrogram_gate_plan(&plan->last_send, &plan->have_last, t_ms, nframes, plan->cut, t->cfg.max_rows);
  if (rows > t->cfg.max_rows) return fail(c, SS_ERR_INVALID, "the batch's clock closes %d spectrogram rows, max_rows is %d: submit fewer frames at a time", rows, t->cfg.max_rows);
  plan->ncuts = rows;
  for (int k = 0; k < rows; ++k) plan->time[k] = t_ms[plan->cut[k]];
  return SS_OK;
}

// ss_feed_submit, behind flush_stages and the result copies, in front of ev_done: the batch's rows, and the plan taken over.
int sgf_enqueue(ss_feed* f, int slot_no, int nframes, const sgf_plan& plan) {
  sgf_ctx* t = static_cast<sgf_ctx*>(f->spectrogram);
  ss_ctx* c = f->c;
  sgf_slot& s = t->slots[(size_t)slot_no];
  // Where the batch's dB values are (rows_source.h), from the state run_batch left a moment ago under this lock, as stf_enqueue asks.
  const ss::RowsChoice src = ss::decide_rows_source(c->last_psd != nullptr, c->last_rel_rows != nullptr, c->last_rows_perm8, c->dif_logq);
  if (t->ring && src.source == ss::kRowsNone) return fail(c, SS_ERR_INVALID, "spectrogram rows (ring): %s", src.refusal);
  const bool ring_batch = t->ring && src.source == ss::kRowsRing;
  const float* db_rows = ring_batch ? c->last_rel_rows : c->last_psd;
  if (!db_rows || ((uintptr_t)db_rows & 15u)) return fail(c, SS_ERR_INVALID, "spectrogram rows: the batch left no (16-byte aligned) dB plane");
  if (ring_batch) {  // (defence only, as in stf_enqueue: run_batch has just cleared the settled pair, and a ring-only call leaves dB values)
    long long sa = 0, sb = 0;
    if (c->last_settled_lo) {
      sa = (c->last_settled_lo - c->last_rel_rows) / (ptrdiff_t)c->n;
      sb = (c->last_settled_hi - c->last_rel_rows) / (ptrdiff_t)c->n;
    }
    const ss::RingDbRange db = ss::ring_db_range(nframes, c->last_rows_db, sa, sb);
    if (db.from != 0 || db.to != nframes) return fail(c, SS_ERR_INVALID, "spectrogram rows (ring): the batch's rows in the ring's buffer are not dB values from its first frame to its last");
  }
  sgf_container* g = sgf_container_for(t, plan.center);
  if (!g) {  // first use of a centre: a zeroed sum row (Container's constructor)
    sgf_container fresh;
    fresh.center = plan.center;
    ss::hip_steps made;
    made.alloc(fresh.d_sum, (size_t)t->size).then([&] { return hipMemsetAsync(fresh.d_sum.get(), 0, sizeof(float) * (size_t)t->size, c->stream); }, "hipMemsetAsync");
    if (!made.ok()) return fail(c, SS_ERR_HIP, "%s failed: %s", made.what(), hipGetErrorString(made.error()));
    t->containers.push_back(std::move(fresh));
    g = &t->containers.back();
  }
  ss::SpecRowsArgs a{};
  a.psd = db_rows;
  a.sum = g->d_sum.get();
  a.rows = s.d_rows.get();
  a.mean = t->cfg.want_mean ? s.d_mean.get() : nullptr;
  a.n = c->n;
  a.nframes = nframes;
  a.size = t->size;
  a.log2_m = t->log2_m;
  a.count0 = g->count;
  a.ncuts = plan.ncuts;
  for (int k = 0; k < plan.ncuts; ++k) a.cut[k] = plan.cut[k];
  if (ring_batch && src.layout != 0) {  // the fold's order: the same arithmetic through the fold's addresses
    const ss::SpecRowsRingArgs ra{a, src.layout};
    const dim3 grid((unsigned)(c->n >> ss::spec_ring_geom(t->log2_m, src.layout).lcol));
    hipLaunchKernelGGL(ss::k_spec_rows_ring, grid, dim3(256), 0, c->stream, ra);
  } else {
    const dim3 grid((unsigned)(c->n >> std::max(t->log2_m, 6)));
    if (t->log2_m <= 2) hipLaunchKernelGGL(ss::k_spec_rows<false>, grid, dim3(256), 0, c->stream, a);
    else hipLaunchKernelGGL(ss::k_spec_rows<true>, grid, dim3(256), 0, c->stream, a);
  }
  SS_HIP(c, hipGetLastError());
  if (plan.ncuts > 0) {
    const size_t cells = (size_t)plan.ncuts * (size_t)t->size;
    SS_HIP(c, hipMemcpyAsync(s.h_rows.get(), s.d_rows.get(), cells, hipMemcpyDeviceToHost, c->stream));
    if (t->cfg.want_mean) SS_HIP(c, hipMemcpyAsync(s.h_mean.get(), s.d_mean.get(), sizeof(float) * cells, hipMemcpyDeviceToHost, c->stream));
  }
  int32_t count = g->count, prev = -1;
  for (int k = 0; k < plan.ncuts; ++k) {  // m_counter at each send: the closing frame is part of its row
    s.h_time.get()[k] = plan.time[k];
    s.h_frame.get()[k] = plan.cut[k];
    s.h_count.get()[k] = count + (plan.cut[k] - prev);
    count = 0;
    prev = plan.cut[k];
  }
  g->count = count + (nframes - 1 - prev);
  g->last_send = plan.last_send;
  g->have_last = plan.have_last;
  s.nrows = plan.ncuts;
  s.frequency = plan.center;
  s.open_count = g->count;
  return SS_OK;
}

// sgf_create and sgf_create_ring: ring = the context has no SS_FLAG_SPECTROGRAM, the row size is the flag's rule (scan_form.h) applied
// here, and a batch's rows may come from the averager ring's buffer
int sgf_create_any(ss_feed* f, const sgf_config* cfg, sgf_ctx** out, bool ring) {
  if (create_args_refused(f, cfg, out, SGF_ABI_VERSION)) return SS_ERR_INVALID;
  if (cfg->max_rows < 1 || cfg->max_rows > SGF_MAX_ROWS) return obj_fail<sgf_ctx>(nullptr, SS_ERR_INVALID, "max_rows %d outside 1..%d", cfg->max_rows, SGF_MAX_ROWS);
  ss_ctx* c = f->c;
  std::lock_guard<std::mutex> lock(c->mtx);
  if (!ring && c->spec_n <= 0) return obj_fail<sgf_ctx>(nullptr, SS_ERR_INVALID, "the scan context needs SS_FLAG_SPECTROGRAM (it fixes the row size and keeps every batch's dB plane)");
  if (ring && c->spec_n > 0)
    return obj_fail<sgf_ctx>(nullptr, SS_ERR_INVALID, "the scan context has SS_FLAG_SPECTROGRAM, which makes every batch keep its dB plane: sgf_create serves it (sgf_create_ring is for a context without the flag)");
  if (feed_already_has<sgf_ctx>(f->spectrogram, "a spectrogram object") || feed_busy<sgf_ctx>(f)) return SS_ERR_INVALID;
  const int size = ring ? std::min(std::min(get_fft(c->cfg.sample_rate, 1000), 16384), c->n) : c->spec_n;  // (scan_form.h: spec_n)
  int log2_m = 0;
  while (log2_m < 30 && ((long long)size << log2_m) < c->n) ++log2_m;
  if (((long long)size << log2_m) != c->n || (!ring && c->spec_m != (1 << log2_m)) || c->n % 64 != 0)
    return obj_fail<sgf_ctx>(nullptr, SS_ERR_INVALID, "%d points into %d spectrogram bins: the rows need a power-of-two ratio and a multiple of 64 points", c->n, size);
  sgf_ctx* t = new (std::nothrow) sgf_ctx();
  if (!t) return obj_fail<sgf_ctx>(nullptr, SS_ERR_NOMEM, "out of memory");
  t->scan = c;
  t->feed = f;
  t->cfg = *cfg;
  t->size = size;
  t->ring = ring;
  t->log2_m = log2_m;
  t->slots.resize((size_t)f->ring.depth());
  const size_t cells = (size_t)cfg->max_rows * (size_t)t->size, rows = (size_t)cfg->max_rows;
  ss::hip_steps made;
  made.then([&] { return hipSetDevice(c->cfg.device_id); });
  for (auto& s : t->slots) {
    made.alloc(s.d_rows, cells).alloc(s.h_rows, cells);
    if (cfg->want_mean) made.alloc(s.d_mean, cells).alloc(s.h_mean, cells);
    made.alloc(s.h_time, rows).alloc(s.h_frame, rows).alloc(s.h_count, rows);
  }
  if (!made.ok()) {
    delete t;
    return obj_fail<sgf_ctx>(nullptr, SS_ERR_NOMEM, "allocating the spectrogram rows' buffers failed: %s", hipGetErrorString(made.error()));
  }
  f->spectrogram = t;
  f->ring.forget_last_collected();
  *out = t;
  return SS_OK;
}

}  // namespace

extern "C" {

int32_t sgf_gate_plan(int64_t* last_send, int32_t* have_last, const int64_t* t_ms, int32_t nframes, int32_t* cut_frame, int32_t cap) {
  if (!last_send || !have_last || nframes < 0 || (nframes > 0 && !t_ms) || cap < 0 || (cap > 0 && !cut_frame)) return SS_ERR_INVALID;
  return ss::spectrogram_gate_plan(last_send, have_last, t_ms, nframes, cut_frame, cap);
}

int sgf_create(ss_feed* f, const sgf_config* cfg, sgf_ctx** out) { return sgf_create_any(f, cfg, out, false); }

int sgf_create_ring(ss_feed* f, const sgf_config* cfg, sgf_ctx** out) { return sgf_create_any(f, cfg, out, true); }

void sgf_destroy(sgf_ctx* t) {
  if (!t) return;
  {
    std::lock_guard<std::mutex> lock(t->scan->mtx);
    (void)hipSetDevice(t->scan->cfg.device_id);
    if (t->feed) {  // (a destroyed feed has waited for its streams already)
      (void)hipStreamSynchronize(t->scan->stream);
      t->feed->spectrogram = nullptr;
    }
  }
  delete t;
}

const char* sgf_last_error(const sgf_ctx* t) { return t ? t->err : create_err<sgf_ctx>(); }

int sgf_rows(sgf_ctx* t, sgf_result* out) {
  if (!t) return SS_ERR_INVALID;
  if (!out) return obj_fail(t, SS_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(t->scan->mtx);
  if (feed_destroyed(t)) return SS_ERR_INVALID;
  const int last = t->feed->ring.last_collected();
  if (last < 0) return obj_fail(t, SS_ERR_INVALID, "no batch has been collected since sgf_create");
  const sgf_slot& s = t->slots[(size_t)last];
  out->nrows = s.nrows;
  out->size = t->size;
  out->frequency = s.frequency;
  out->sample_rate = t->scan->cfg.sample_rate;
  out->open_count = s.open_count;
  out->time_ms = s.h_time.get();
  out->frame = s.h_frame.get();
  out->count = s.h_count.get();
  out->rows = s.h_rows.get();
  out->mean = t->cfg.want_mean ? s.h_mean.get() : nullptr;
  return SS_OK;
}

int sgf_batch_db_rows(sgf_ctx* t, int32_t frame0, int32_t nframes, float* out) {
  if (!t) return SS_ERR_INVALID;
  if (!out) return obj_fail(t, SS_ERR_INVALID, "null argument");
  ss_ctx* c = t->scan;
  std::lock_guard<std::mutex> lock(c->mtx);
  if (feed_destroyed(t)) return SS_ERR_INVALID;
  const int n = c->n;
  if (c->last_n <= 0) return obj_fail(t, SS_ERR_INVALID, "no batch whose rows still hold dB values (none submitted yet, or a retune or ss_reset_noise since)");
  if (frame0 < 0 || nframes < 0 || (long long)frame0 + nframes > c->last_n) return obj_fail(t, SS_ERR_INVALID, "frames [%d, %d + %d) outside the batch's %d", frame0, frame0, nframes, c->last_n);
  const ss::RowsChoice src = ss::decide_rows_source(c->last_psd != nullptr, c->last_rel_rows != nullptr, c->last_rows_perm8, c->dif_logq);
  if (src.source == ss::kRowsNone) return obj_fail(t, SS_ERR_INVALID, "%s", src.refusal);
  if (src.source == ss::kRowsRing) {  // which of the rows still hold dB values: ss_read_window's rule (ring_db_range)
    long long sa = 0, sb = 0;
    if (c->last_settled_lo) {
      sa = (c->last_settled_lo - c->last_rel_rows) / (ptrdiff_t)n;
      sb = (c->last_settled_hi - c->last_rel_rows) / (ptrdiff_t)n;
    }
    const ss::RingDbRange db = ss::ring_db_range(c->last_n, c->last_rows_db, sa, sb);
    if (frame0 < db.from || frame0 + nframes > db.to) return obj_fail(t, SS_ERR_INVALID, "the batch's rows in the ring's buffer are no longer dB values (settled since the submit)");
  }
  if (nframes == 0) return SS_OK;
  const float* rows = (src.source == ss::kRowsPlane ? c->last_psd : c->last_rel_rows) + (size_t)frame0 * (size_t)n;
  if (hipSetDevice(c->cfg.device_id) != hipSuccess) return obj_fail(t, SS_ERR_HIP, "hipSetDevice failed: %s", hipGetErrorString(hipGetLastError()));
  flush_stages(c);
  if (src.layout == 0) {
    if (hipMemcpyAsync(out, rows, sizeof(float) * (size_t)nframes * (size_t)n, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
      return obj_fail(t, SS_ERR_HIP, "reading the batch's rows failed: %s", hipGetErrorString(hipGetLastError()));
    return SS_OK;
  }
  // the fold's order undone, as read_perm8_row does: a row comes over whole, the host picks. One row of scratch, no exception across the ABI.
  float* folded = new (std::nothrow) float[(size_t)n];
  if (!folded) return obj_fail(t, SS_ERR_NOMEM, "out of memory");
  int st = SS_OK;
  for (size_t f = 0; f < (size_t)nframes && st == SS_OK; ++f) {
    if (hipMemcpyAsync(folded, rows + f * (size_t)n, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
      st = obj_fail(t, SS_ERR_HIP, "reading the batch's rows failed: %s", hipGetErrorString(hipGetLastError()));
    else
      for (int i = 0; i < n; ++i) out[f * (size_t)n + (size_t)i] = folded[(size_t)ss::dif_bin_offset(i, src.layout)];
  }
  delete[] folded;
  return st;
}

}  // extern "C"
