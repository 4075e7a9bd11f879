// host_feed.h — pipelined host feeding (include/specscan.h, ss_feed_*): pinned staging slots, H2D on a copy stream, the chain on
// the context's stream, exact-size candidate read-back on a third stream at collect time. Which slot is whose is feed_ring.h's.
// Part of specscan.hip's translation unit, included behind the scan engine.
//
// Three objects can ride on a feed: the tracked feed's digest (host_track_feed.h), the recorder (host_record_feed.h) and the
// spectrogram rows (host_spectrogram_feed.h). What the feed calls of them is declared here; what they share stands below ss_feed.
#pragma once

struct ss_feed;

// What a batch's clock decides for the spectrogram rows, worked out on copies before anything is enqueued (sgf_plan_batch) and
// taken over once the batch's chain is in the stream (sgf_enqueue).
struct sgf_plan {
  int32_t center = 0;
  int64_t last_send = 0;  // the centre's gate behind the batch
  int32_t have_last = 0;
  int32_t ncuts = 0;
  int32_t cut[SGF_MAX_ROWS];   // the closing frames
  int64_t time[SGF_MAX_ROWS];  // and their t_ms
};

namespace {
// the riders' hooks, under the context's lock
int stf_enqueue(ss_feed* f, int slot, int nframes);  // ss_feed_submit, behind the result copies
bool stf_wants_no_plane_calls(const ss_feed* f);     // ss_feed_submit, in front of the batch: a ring tracker or ring spectrogram object is bound and nothing reads the plane
bool sgf_reads_ring_rows(const ss_feed* f);          // the bound spectrogram object is sgf_create_ring's (f->spectrogram != nullptr)
// feed_collect on a tracked feed: the slot's digest, its read-back enqueued on the feed's read-back stream (*copies: something was)
int stf_collect_digest(ss_feed* f, int slot, int nframes, int ncopy, stf_result* digest, bool* copies);
int sgf_plan_batch(ss_feed* f, int nframes, const int64_t* t_ms, sgf_plan* plan);  // ss_feed_submit, in front of the upload
int sgf_enqueue(ss_feed* f, int slot, int nframes, const sgf_plan& plan);          // ss_feed_submit, behind stf_enqueue

// What stf_ctx, srf_ctx and sgf_ctx start with.
struct feed_rider {
  ss_ctx* scan = nullptr;
  ss_feed* feed = nullptr;  // null once the feed has been destroyed: only the rider's destroy and last_error from then on
  char err[512] = "";
};

struct ss_feed_slot {
  ss::pinned_buffer<unsigned char> h_in;
  ss::device_buffer<unsigned char> d_in;
  ss::pinned_buffer<int32_t> h_off, h_idx;
  ss::pinned_buffer<float> h_avg, h_psd;
  ss::device_buffer<int32_t> d_off, d_idx;
  ss::device_buffer<float> d_avg;
  ss::hip_event ev_h2d, ev_done;
  int nframes = 0;
  int64_t tag = 0;
};
}  // namespace

struct SS_HIDDEN ss_feed {
  ss_ctx* c = nullptr;
  int cand_cap = 0;
  bool want_psd = false;
  bool items = false;  // ss_feed_create_items on a decimated context: h_in holds whole items of n * decim samples, d_in their first n
  ss::feed_ring ring;
  std::vector<ss_feed_slot> slots;
  ss::hip_stream copy_stream, d2h_stream;
  feed_rider* tracker = nullptr;      // stf_create: every batch is digested behind its chain (include/specscan_track_feed.h)
  feed_rider* recorder = nullptr;     // srf_create: a collected slot stays held until its samples are recorded or let go (include/specscan_record_feed.h)
  feed_rider* spectrogram = nullptr;  // sgf_create: every batch leaves the spectrogram rows it closes (include/specscan_spectrogram_feed.h); sgf_rows reads ring.last_collected()

  explicit ss_feed(int depth) : ring(depth), slots((size_t)depth) {}
};

namespace {

// ---- what the riders share -------------------------------------------------------------------------------------------------
// The refusals every rider makes, with the text every rider gives. Each writes its message (obj_fail: into the object, or into its
// API's own create-time text) and returns true: the caller returns SS_ERR_INVALID.
template <class T, class Cfg>
bool create_args_refused(const void* on, const Cfg* cfg, T** out, uint32_t abi) {
  if (!on || !cfg || !out) return obj_fail<T>(nullptr, SS_ERR_INVALID, "null argument") != SS_OK;
  *out = nullptr;
  if (cfg->abi_version != abi) return obj_fail<T>(nullptr, SS_ERR_INVALID, "abi_version %u, library has %u", cfg->abi_version, abi) != SS_OK;
  return false;
}

template <class T>
bool feed_already_has(const feed_rider* rider, const char* what) {
  return rider && obj_fail<T>(nullptr, SS_ERR_INVALID, "the feed already has %s", what) != SS_OK;
}

template <class T>
bool feed_busy(const ss_feed* f) {
  return !f->ring.idle() && obj_fail<T>(nullptr, SS_ERR_INVALID, "the feed has batches pending: collect them first") != SS_OK;
}

template <class T>
bool feed_destroyed(T* t) {
  return !t->feed && obj_fail(t, SS_ERR_INVALID, "the feed has been destroyed") != SS_OK;
}

// ss_feed_destroy, under the context's lock: the riders outlive the feed
void feed_gone(feed_rider* t) {
  if (t) t->feed = nullptr;
}

int feed_create(ss_ctx* c, int32_t depth, int32_t cand_cap, int32_t want_psd, bool items, ss_feed** out) {
  if (!c || !out) return SS_ERR_INVALID;
  std::lock_guard<std::mutex> lock(c->mtx);
  if (depth < 2 || depth > ss::feed_ring::kMaxDepth || cand_cap < 0) return fail(c, SS_ERR_INVALID, "feed depth %d (2..8) / cand_cap %d", depth, cand_cap);
  SS_HIP(c, hipSetDevice(c->cfg.device_id));
  ss_feed* f = new ss_feed(depth);
  f->c = c;
  f->cand_cap = cand_cap;
  f->want_psd = want_psd != 0;
  f->items = items && c->cfg.decim != 1;  // with decim == 1 the items are the frames: an ordinary feed
  const size_t frames = (size_t)c->cfg.max_batch;
  const size_t in_bytes = in_bytes_per_sample(c->cfg.in_format) * (size_t)c->n * frames;
  const size_t host_bytes = f->items ? in_bytes * (size_t)c->cfg.decim : in_bytes;
  const size_t ncand = (size_t)(cand_cap > 0 ? cand_cap : 1);
  ss::hip_steps made;
  made.stream(f->copy_stream).stream(f->d2h_stream);
  for (auto& s : f->slots) {
    made.alloc(s.h_in, host_bytes).alloc(s.d_in, in_bytes).alloc(s.h_off, frames + 1).alloc(s.h_idx, ncand).alloc(s.h_avg, ncand);
    if (f->want_psd) made.alloc(s.h_psd, (size_t)c->n * frames);
    made.alloc(s.d_off, frames + 1).alloc(s.d_idx, ncand).alloc(s.d_avg, ncand);
    made.event(s.ev_h2d).event(s.ev_done);
  }
  if (!made.ok()) {
    delete f;
    return fail(c, SS_ERR_HIP, "%s failed: %s", made.what(), hipGetErrorString(made.error()));
  }
  *out = f;
  return SS_OK;
}

// ss_feed_collect and stf_collect: the oldest pending batch, and — digest != nullptr — its digest, read back in exact sizes on the
// feed's read-back stream next to the candidate lists.
int feed_collect(ss_feed* f, ss_feed_result* out, stf_result* digest) {
  ss_ctx* c = f->c;
  ss_feed_slot* s = nullptr;
  int slot_no = 0;
  {
    std::lock_guard<std::mutex> lock(c->mtx);
    if (f->tracker && !digest) return fail(c, SS_ERR_INVALID, "ss_feed_collect on a tracked feed: collect through stf_collect");
    const ss::ring_refusal r = f->ring.oldest_pending(&slot_no);
    if (r == ss::ring_refusal::slot_held) return fail(c, SS_ERR_INVALID, "the batch collected last is held for the recorder: srf_record or srf_release first");
    if (r != ss::ring_refusal::none) return fail(c, SS_ERR_INVALID, "ss_feed_collect: nothing pending");
    s = &f->slots[(size_t)slot_no];
  }
  // wait outside the lock: a producer thread may acquire / submit the next slots meanwhile
  hipError_t e = hipEventSynchronize(s->ev_done);
  std::lock_guard<std::mutex> lock(c->mtx);
  if (e != hipSuccess) return fail(c, SS_ERR_HIP, "hipEventSynchronize failed: %s", hipGetErrorString(e));
  SS_HIP(c, hipSetDevice(c->cfg.device_id));
  const int total = s->h_off.get()[s->nframes];
  const int ncopy = total < f->cand_cap ? total : f->cand_cap;
  bool copies = false;
  if (ncopy > 0) {
    SS_HIP(c, hipMemcpyAsync(s->h_idx.get(), s->d_idx.get(), sizeof(int32_t) * (size_t)ncopy, hipMemcpyDeviceToHost, f->d2h_stream));
    SS_HIP(c, hipMemcpyAsync(s->h_avg.get(), s->d_avg.get(), sizeof(float) * (size_t)ncopy, hipMemcpyDeviceToHost, f->d2h_stream));
    copies = true;
  }
  if (digest) {
    const int st = stf_collect_digest(f, slot_no, s->nframes, ncopy, digest, &copies);
    if (st != SS_OK) return st;
  }
  if (copies) SS_HIP(c, hipStreamSynchronize(f->d2h_stream));
  out->nframes = s->nframes;
  out->status = (f->cand_cap > 0 && total > f->cand_cap) ? SS_ERR_CAND_OVERFLOW : SS_OK;
  out->user_tag = s->tag;
  out->cand_off = s->h_off.get();
  out->cand_idx = s->h_idx.get();
  out->cand_avg = s->h_avg.get();
  out->psd_db = f->want_psd ? s->h_psd.get() : nullptr;
  // held: its d_in is what srf_record reads
  if (f->ring.collected(slot_no, f->recorder != nullptr) != ss::ring_refusal::none) return fail(c, SS_ERR_INVALID, "ss_feed_collect: another collect took the batch meanwhile");
  return SS_OK;
}

}  // namespace

extern "C" {

int ss_feed_create(ss_ctx* c, int32_t depth, int32_t cand_cap, int32_t want_psd, ss_feed** out) { return feed_create(c, depth, cand_cap, want_psd, false, out); }

int ss_feed_create_items(ss_ctx* c, int32_t depth, int32_t cand_cap, int32_t want_psd, ss_feed** out) { return feed_create(c, depth, cand_cap, want_psd, true, out); }

void ss_feed_destroy(ss_feed* f) {
  if (!f) return;
  {
    std::lock_guard<std::mutex> lock(f->c->mtx);
    (void)hipSetDevice(f->c->cfg.device_id);
    (void)hipStreamSynchronize(f->copy_stream);
    (void)hipStreamSynchronize(f->c->stream);
    (void)hipStreamSynchronize(f->d2h_stream);
    feed_gone(f->tracker);
    feed_gone(f->recorder);
    feed_gone(f->spectrogram);
  }
  delete f;
}

int ss_feed_pending(const ss_feed* f) {
  if (!f) return 0;
  std::lock_guard<std::mutex> lock(f->c->mtx);
  return f->ring.pending();
}

int ss_feed_acquire(ss_feed* f, void** frames) {
  if (!f || !frames) return SS_ERR_INVALID;
  ss_ctx* c = f->c;
  std::lock_guard<std::mutex> lock(c->mtx);
  int slot = 0;  // acquiring twice without a submit hands out the same buffer
  if (f->ring.acquire(&slot) != ss::ring_refusal::none) return fail(c, SS_ERR_INVALID, "no free feed slot: collect a batch first");
  *frames = f->slots[(size_t)slot].h_in.get();
  return SS_OK;
}

int ss_feed_submit(ss_feed* f, int32_t nframes, const int64_t* t_ms, int64_t user_tag) {
  if (!f) return SS_ERR_INVALID;
  ss_ctx* c = f->c;
  std::lock_guard<std::mutex> lock(c->mtx);
  const int slot = f->ring.acquired();
  if (slot < 0) return fail(c, SS_ERR_INVALID, "ss_feed_submit without ss_feed_acquire");
  if (nframes <= 0) return fail(c, SS_ERR_INVALID, "nframes %d", nframes);
  if (nframes > c->cfg.max_batch) return fail(c, SS_ERR_BATCH, "nframes %d > max_batch %d", nframes, c->cfg.max_batch);
  sgf_plan rows_plan;
  if (f->spectrogram) {  // refusals of the spectrogram rows come before anything is enqueued: the slot stays acquired
    const int planned = sgf_plan_batch(f, nframes, t_ms, &rows_plan);
    if (planned != SS_OK) return planned;
  }
  SS_HIP(c, hipSetDevice(c->cfg.device_id));
  ss_feed_slot& s = f->slots[(size_t)slot];
  const int n = c->n;
  const size_t row_bytes = in_bytes_per_sample(c->cfg.in_format) * (size_t)n;
  if (f->items)  // the first n samples of every item: d_in stays compact, and everything behind the copy is an ordinary feed's
    SS_HIP(c, hipMemcpy2DAsync(s.d_in.get(), row_bytes, s.h_in.get(), row_bytes * (size_t)c->cfg.decim, row_bytes, (size_t)nframes, hipMemcpyHostToDevice, f->copy_stream));
  else
    SS_HIP(c, hipMemcpyAsync(s.d_in.get(), s.h_in.get(), row_bytes * (size_t)nframes, hipMemcpyHostToDevice, f->copy_stream));
  SS_HIP(c, hipEventRecord(s.ev_h2d, f->copy_stream));
  SS_HIP(c, hipStreamWaitEvent(c->stream, s.ev_h2d, 0));
  NoiseState* z = nullptr;
  int st = get_noise(c, &z);
  if (st != SS_OK) return st;
  const int n_learn = plan_learning(c, z, nframes, t_ms);
  const bool want_cands = f->cand_cap > 0;
  st = run_batch(c, s.d_in.get(), (long long)n, nframes, n_learn, z,
                 CallOut{nullptr, nullptr, nullptr, s.d_off.get(), want_cands ? s.d_idx.get() : nullptr, want_cands ? s.d_avg.get() : nullptr, f->cand_cap},
                 stf_wants_no_plane_calls(f));  // (false on every feed without a ring tracker or ring spectrogram object: the call is what it has always been)
  if (st != SS_OK) return st;
  flush_stages(c);  // the slot's results are copied out right behind the batch
  SS_HIP(c, hipMemcpyAsync(s.h_off.get(), s.d_off.get(), sizeof(int32_t) * ((size_t)nframes + 1), hipMemcpyDeviceToHost, c->stream));
  if (f->want_psd) SS_HIP(c, hipMemcpyAsync(s.h_psd.get(), c->last_psd, sizeof(float) * (size_t)n * (size_t)nframes, hipMemcpyDeviceToHost, c->stream));
  if (f->tracker) {  // the digest: behind the chain and the result copies, in front of ev_done; nothing in it waits on the host
    st = stf_enqueue(f, slot, nframes);
    if (st != SS_OK) return st;
  }
  if (f->spectrogram) {  // the rows this batch closes: one kernel on the dB plane (or the rows in the ring's buffer), then exactly their bytes to the slot's pinned memory
    st = sgf_enqueue(f, slot, nframes, rows_plan);
    if (st != SS_OK) return st;
  }
  SS_HIP(c, hipEventRecord(s.ev_done, c->stream));
  s.nframes = nframes;
  s.tag = user_tag;
  (void)f->ring.submit();
  return SS_OK;
}

int ss_feed_collect(ss_feed* f, ss_feed_result* out) {
  if (!f || !out) return SS_ERR_INVALID;
  return feed_collect(f, out, nullptr);
}

}  // extern "C"
