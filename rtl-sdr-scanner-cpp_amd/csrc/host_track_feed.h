// host_track_feed.h — the tracking digest behind the pipelined feed (include/specscan_track_feed.h, stf_*, and its sparse form,
// include/specscan_track_sparse.h; kernels: track_feed.h + track_digest.h, track_sparse.h): every batch submitted through a tracked
// feed is digested on the context's stream right behind its chain; the watch list is formed on the device from sequence-number
// marks, so no step waits for the host. Part of specscan.hip's translation unit, behind host_feed.h and host_track.h.
//
// Ordering against the next batch's chain, which may run on the library's own queues and rotates the PSD / avg / mask / offset
// buffers (and raises the noise ceiling in place while it learns): the digest is on the context's stream, and whatever that stream
// holds comes before a batch — an in-order call is on that stream itself, and an overlapped call's first launch waits for an event
// recorded behind it (run_call_deep: "whatever the public stream holds ... comes first"; the want_psd copy of ss_feed_submit
// rests on the same lines). ss_feed_submit has drained the deferred stages (flush_stages joins the queues into the stream) before
// the digest is enqueued, so the digest in turn sees the whole batch.
//
// ---- stf_create_ring (include/specscan_track_feed_ring.h): batches that keep no dB plane -------------------------------------------
// How such a batch comes about. A batch goes through the feed as an ordinary call (run_batch: device_call = false), and an ordinary
// call keeps its dB plane at every size (call_route.h: keeps_no_plane wants CallAsk::device). The fold, the culled chains' ring-only
// calls and the 2^20-point ring-only calls are therefore forms no feed took before; while a ring tracker is bound, ss_feed_submit
// hands run_batch device_call = true at 65536 points and up (stf_wants_no_plane_calls; not on a feed with want_psd or sgf_create's
// spectrogram rows, which read the plane; sgf_create_ring's rows read the ring's buffer: below). What CallAsk::device promises — the input stays untouched until the stages have run — the slot
// gives: d_in is written again only after the batch has been collected, and ss_feed_submit drains the stages right behind the call.
// Nothing else reads the flag at these sizes: decide_call's deep branch (the only other reader) is 8192 points.
//
// What the digest of batch k reads that a plane batch's does not: the batch's rows in the averager ring's buffer (last_rel_rows: dB
// values, in the fold's order after a fold), through RingRows in k_ring_best / k_ring_tail and through last_det.psd in the replay;
// the window in front of them (last_det.hist_in, 35 rows, some of them dB rows: ring_db_from); the noise ceiling (thr). It runs on
// the context's stream while the host submits batches k + 1 and k + 2. The rule that orders everything: AT THESE SIZES THE LIBRARY
// HAS NO QUEUE OF ITS OWN, AND A FEED DRAINS EVERY BATCH. The second half first: ss_feed_submit runs flush_stages behind every run_batch,
// so through a feed the no-plane forms run drained per batch — the fold's, the merged chain's and the ring-only calls' kernels, but
// never their overlapped shape: the merged chain's row half runs in the drain's launch instead of beside the next call's columns,
// and the plan, detect and emit stages never ride on a later call's launch. That is what puts the whole of batch k — its rows in the
// ring, its mask bits, its lists — in the stream in front of its digest, and it is why last_det is batch k's own detect stage.
// The first half: ScanForm::deep is 8192 points only (scan_form.h), and the side streams belong to it alone (run_call_deep,
// drain_deep, fold_spectrogram_slots); every launch run_batch, launch_step, launch_chunks, plan_call, place_ring, settle_ring_db,
// set_ring_form and flush_stages make on a context of 65536 points and up names c->stream (launch_step's default; SS_LAUNCH_SLOT).
// One in-order stream: what is enqueued behind the digest runs behind it. So no event wait had to be added on the scan side, and
// the untracked scan is untouched. Route by route, everything that can write what the digest of batch k reads is enqueued by a LATER
// host call, under the context's lock, and therefore behind the digest (stf_enqueue runs in the same ss_feed_submit as the batch,
// under the same lock acquisition, before the lock is released once):
//   * the fold, KIND 8 / 9 of k_scan_step (65536 / 131072 points, int8: launch_fold) — one launch of k_scan_step per call on c->stream whose FFT role
//     writes the call's rows to the region place_ring gave it; the plan, detect and emit stages of the calls before ride on it. Batch
//     k + 1's launch is enqueued by batch k + 1's ss_feed_submit: behind digest k. Its rows go where ring_place_decide puts them —
//     never on the window or the batch rows that hist_prev / hist_prev2 protect — but stream order alone already suffices.
//   * the merged chain, KIND 7 / 12 (65536 / 262144 points, one launch per call: launch_merged + rows_for_next_launch) — the row half
//     of batch k waits for the next launch; ss_feed_submit's flush_stages runs it (Waiting::rows) before the digest is enqueued, so
//     the rows are in the ring when the digest reads them, and batch k + 1's column launch, on c->stream, is behind the digest.
//   * the two-launch forms, KIND 6 and KIND 10 (65536 / 262144 points: CALL_ROWS256_STEP, CALL_ROWS1024X256, launch_chunks) — column launch and
//     row launch per chunk, both on c->stream, all enqueued inside batch k's run_batch; the deferred stages by the same flush.
//   * the 2^20-point column / row pair, KIND 4 / 5 (CALL_TWO_PASS: launch_cols1024, then k_scan_step's row role; its drain) — both on c->stream; a batch
//     shorter than the ring writes its rows right behind the window it reads (ring_rows = rp.in + 35 rows), a longer one to a region
//     of its own (rp.batch): batch k + 1 places its rows behind those, in a launch behind digest k.
//   * k_ring_fill — drain_deep's, 8192 points only: never launched here.
//   * place_ring's k_hist_shift — the wrap of the 1024-row ring: when batch k + j finds no room behind the window, place_ring drains
//     what waits (nothing, through a feed) and copies the window to the front of the buffer, on c->stream, in batch k + j's
//     ss_feed_submit: behind digest k, which has read the old place by then. The rows of batch k itself are not moved (only the
//     35-row window is), and the RingRows / DetectArgs the digest was launched with hold pointers taken before the move.
//     tests/test_gpu_track_feed_ring.py::test_ring_wrap_with_two_batches_in_flight runs 1120 rows through it.
//   * settle_ring_db's k_rows_sub_thr — run_batch calls it when a call of another kind, or under another ceiling, finds dB rows in the
//     window (a learning batch behind ring batches), ss_set_frequency_range and ss_reset_noise call it too: each under the lock, on
//     c->stream, behind every digest enqueued so far. The host side of it — last_settled_lo / hi, which say which rows no longer
//     hold dB values — is read by ring_rows() inside stf_enqueue, that is right behind the batch's own run_batch, which has just
//     cleared the pair: the digest is launched with db_from / db_to = the whole batch, the truth at the point of the stream where
//     it runs. A later settle changes the rows behind it and the host state behind the launch: neither reaches the digest.
//   * set_ring_form's k_rows_perm8 + k_copy_rows — a change between the fold's order and bin order (a learning batch on a fold
//     context): on c->stream, in the later batch's run_batch; it rewrites the window at the front of the buffer and leaves batch
//     k's rows where they are. RingRows::logq and the replay's layout were fixed when digest k was launched.
//   * the noise ceiling — raised in place only by learning frames (launch_learning, on c->stream, in a later batch's run_batch);
//     ss_reset_noise waits for the stream before it frees a ceiling.
//   * the sparse avg plane d_avg2[b] and the scratch of the replay — as for the 8192-point replay below.
// The host-side state the digest is built from — last_psd, last_rel_rows, last_rows_perm8, last_rows_db, last_settled_*, last_n_learn,
// last_thr, last_avg, last_det — is read once, in stf_enqueue, under the lock the batch's run_batch ran under; RelRows / RingRows /
// WatchTilesArgs go into the launches by value. No form had to be refused.
//
// ---- the second reader: sgf_create_ring (include/specscan_spectrogram_feed_ring.h, host_spectrogram_feed.h) -----------------------
// A ring spectrogram object's kernel (k_spec_rows over bin-order ring rows, k_spec_rows_ring over the fold's) reads batch k's rows in
// the ring's buffer — last_rel_rows, nothing in front of them, no ceiling — once, on the context's stream, enqueued by sgf_enqueue in
// batch k's own ss_feed_submit behind stf_enqueue, under the same lock acquisition. It is a reader of a subset of what digest k reads,
// at the same point of the same stream, so every line above holds for it with "digest" read as "rows kernel": a later batch's fold,
// merged or two-launch chain places its rows elsewhere and in a launch behind it; settle_ring_db (k_rows_sub_thr), place_ring's window
// move (k_hist_shift) and set_ring_form's reorder are enqueued by later host calls on c->stream; and because ss_feed_submit runs
// flush_stages behind every run_batch, the whole of batch k's rows — the merged chain's row half included — is in the stream in front
// of it. The object also switches the feed to device-style calls with NO tracker bound (stf_wants_no_plane_calls): nothing in the
// argument needs the digest to be there. What the kernel writes — the centre's sum row, the slot's rows — is its own, ordered by the
// stream against the next batch's kernel and by ev_done against the collect. The host state it is built from (last_psd, last_rel_rows,
// last_rows_perm8, last_rows_db, last_settled_*) is read once in sgf_enqueue and goes into the launch by value.
#pragma once

namespace {
struct stf_slot {
  ss::device_buffer<int32_t> d_coff, d_best, d_watch, d_pidx, d_keys;
  ss::device_buffer<float> d_cavg, d_pavg;
  ss::device_buffer<ss::FeedDigestHeader> d_hdr;
  ss::pinned_buffer<int32_t> h_best, h_watch, h_pidx, h_keys;
  ss::pinned_buffer<float> h_cavg, h_pavg;
  ss::pinned_buffer<ss::FeedDigestHeader> h_hdr;
  uint64_t seq = 0, keys_seq = 0;
};
}  // namespace

struct SS_HIDDEN stf_ctx : feed_rider {
  stf_config cfg{};
  digest_rows rows;
  ss::device_buffer<uint32_t> d_mark, d_keymark;  // [n] each: sequence number of the newest batch that had the bin as cand_best / as a posted key
  ss::device_buffer<int32_t> d_counts;            // [ceil(n / 256)] block counts, then their prefix sums
  int nblocks = 0;
  std::vector<stf_slot> slots;
  uint64_t next_seq = 1, collected = 0;  // the next batch's sequence number; the newest collected one
  uint64_t post_seq = 0;                 // p and K_p as last posted
  std::vector<int32_t> post_keys;
  // stf_create_sparse on a context that keeps no planes (include/specscan_track_sparse.h, kernels: track_sparse.h)
  bool sparse = false;
  ss::device_buffer<uint32_t> d_sp_mask;                 // [(n / 32) x max_batch] the replayed tiles' mask words: never read
  ss::device_buffer<int> d_sp_counts;                    // [max_batch] ... and their counts
  ss::device_buffer<int32_t> d_col_flag;                 // [nblocks] the tile columns the batch's watch windows touch
  ss::device_buffer<unsigned long long> d_sp_evaluated;  // tiles the replay ran, since stf_create_sparse / stf_reset
  uint64_t sp_tiles_in_batches = 0;
  // stf_create_ring on such a context (include/specscan_track_feed_ring.h): batches go through the feed as calls that may keep no dB
  // plane, and a batch that kept none is digested from the rows it left in the averager ring's buffer (track_digest_sparse.h)
  bool ring = false;
};

namespace {

// (under the context's lock) rows, marks and post back to zero, on the context's stream
hipError_t stf_clear(stf_ctx* t) {
  ss_ctx* c = t->scan;
  hipError_t e = tails_zero(t->rows, c);
  if (e == hipSuccess) e = hipMemsetAsync(t->d_mark.get(), 0, sizeof(uint32_t) * (size_t)c->n, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(t->d_keymark.get(), 0, sizeof(uint32_t) * (size_t)c->n, c->stream);
  if (e == hipSuccess && t->sparse) e = hipMemsetAsync(t->d_sp_evaluated.get(), 0, sizeof(unsigned long long), c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  t->sp_tiles_in_batches = 0;
  t->next_seq = 1;
  t->collected = 0;
  t->post_seq = 0;
  t->post_keys.clear();
  return e;
}

// A sparse object, between the watch list and the peaks: avg in the tile columns the watch windows touch, by the batch's own detect
// stage once more (track_sparse.h) — its arguments as they were launched (ss_ctx::last_det), with everything but avg switched off:
//   maskbits, counts  scratch of the tracker's. The scan's mask buffers are all zero between uses (EmitArgs::clear_masks: culled tiles
//                     write nothing and rely on it) and its count buffers are zeroed on a schedule of their own: words written there
//                     now would be a later batch's candidates.
//   avg_out           the batch's sparse plane (ss_ctx::last_avg = DetectArgs::avg_sparse): every cell of a marked column, hit or not
//   rel_out, hist_out nothing: hist_by_fft = 1 — the ring has this batch's rows already (its own tiles, its FFT stage or the drain's
//                     k_ring_fill wrote them: flush_stages has run)
//   segsum, halo_segsum, live, tile_list, stats   nothing is culled, waited for or counted: ss_get_stats does not move
//   spec_*            zero, and the SPEC = false tile: a SS_FLAG_SPECTROGRAM context does not accumulate the batch twice
// The rows in front of the batch are read where the detect stage read them, hist_in or halo_psd as launched (the same bits either way,
// detect_fused.h: DetectArgs::halo_psd). Both are intact here, and stay so until the replay has read them:
//   * the ring window [hist_in, hist_in + 35 rows): a call's own rows never land on its own window (ring_place.h: the first thing
//     ring_place_decide checks), so neither this batch's tiles nor its FFT stage nor the drain's k_ring_fill (hist_out) touched it. The
//     next writers are a LATER call's rows, or that call's place_ring moving the window to the front (k_hist_shift, on this stream) or
//     settling dB rows in place (k_rows_sub_thr, on this stream): all enqueued after this replay. Calls through the feed carry
//     no halo_psd: halo frames are the 8192-point deep pipeline's (run_call_deep, taken by overlapped device calls only), an ordinary
//     feed's calls are not device calls (run_batch: device_call = false), and the device calls a ring tracker's feed makes are of
//     65536 points and up, where no deep pipeline exists. If a call did carry one, its halo buffer (d_halo[L mod 2 nq]) is next
//     written 2 nq launches on, by a call enqueued later.
//   * the dB plane (d_psd2 rotation, DetectArgs::psd = last_psd), the noise ceiling and the pass mask: what k_best_blocked and k_save_tail
//     of the same digest read, on the same grounds (the comment at the top of this file).
//   * d_avg2[b] comes round again after nbuf batches — as the sparse plane of a later batch's detect stage, behind this stream.
// A later call's launches on the library's own queues wait for an event recorded on this stream first ("whatever the public stream
// holds ... comes first"), in-order calls are on it: everything above is ordered behind the digest by that one rule. From 65536
// points up there are no such queues at all and the rule is plain stream order: the argument at the top of this file, route by route.
// A ring batch (src.source == kRowsRing, stf_create_ring): the same recipe with the tile of the form the batch took, k_digest_tiles<layout>
// (st_replay_watch_tiles' kernels, on the column flags the device formed); last_det.psd is then the batch's rows in the ring's buffer.
int stf_replay_watch_tiles(stf_ctx* t, stf_slot& s, int nframes, const ss::RowsChoice& src) {
  ss_ctx* c = t->scan;
  const int n = c->n;
  if (!last_det_is_the_batch(c, nframes)) return fail(c, SS_ERR_INVALID, "tracked feed (sparse): the detect stage launched last is not this batch's");
  hipLaunchKernelGGL(ss::k_feed_watch_cols, dim3(1), dim3(256), 0, c->stream, (const int32_t*)s.d_watch.get(), (const ss::FeedDigestHeader*)s.d_hdr.get(), n,
                     t->rows.group_size / 2, t->d_col_flag.get());
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
  const int frame_tiles = (nframes + wa.det.shift + kFusedTF - 1) / kFusedTF, cols = t->nblocks;  // (256-bin blocks: the tile columns)
  const dim3 grid((unsigned)(frame_tiles * cols));
  if (src.source != ss::kRowsRing) hipLaunchKernelGGL(ss::k_watch_tiles, grid, dim3(256), 0, c->stream, wa);
  else if (src.layout == 4) hipLaunchKernelGGL(ss::k_digest_tiles<4>, grid, dim3(256), 0, c->stream, wa);
  else if (src.layout == 3) hipLaunchKernelGGL(ss::k_digest_tiles<3>, grid, dim3(256), 0, c->stream, wa);
  else hipLaunchKernelGGL(ss::k_digest_tiles<0>, grid, dim3(256), 0, c->stream, wa);
  t->sp_tiles_in_batches += (uint64_t)frame_tiles * (uint64_t)cols;
  return SS_OK;
}

// ss_feed_submit, under the context's lock, behind flush_stages and the result copies: the digest of the batch just enqueued.
int stf_enqueue(ss_feed* f, int slot_no, int nframes) {
  stf_ctx* t = static_cast<stf_ctx*>(f->tracker);
  ss_ctx* c = f->c;
  ss_feed_slot& fs = f->slots[(size_t)slot_no];
  stf_slot& s = t->slots[(size_t)slot_no];
  const int n = c->n;
  if (t->next_seq > 0xffffffffull) return fail(c, SS_ERR_INVALID, "tracked feed: 2^32 - 1 batches since stf_create / stf_reset (the device counts in 32 bits): stf_reset");
  // Where the batch's rows are (rows_source.h), from the state run_batch left a moment ago under this lock: nothing has run between the
  // two that could settle a row or move the window. A ring batch is for stf_create_ring's objects only.
  const ss::RowsChoice src = ss::decide_rows_source(c->last_psd != nullptr, c->last_rel_rows != nullptr, c->last_rows_perm8, c->dif_logq);
  const bool ring_batch = t->ring && c->fused && src.source == ss::kRowsRing;
  if (t->ring && c->fused && !c->last_psd && src.source == ss::kRowsNone) return fail(c, SS_ERR_INVALID, "tracked feed (ring): %s", src.refusal);
  if (!c->last_avg || (c->fused && ((!c->last_psd && !ring_batch) || !c->last_thr)) || (!c->fused && !c->d_rel))
    return fail(c, SS_ERR_INVALID, "tracked feed: the batch left no dB plane, avg plane or noise ceiling to digest");
  // (defence only, as in st_digest: run_batch has just cleared the pair, and nothing between it and this line settles a row)
  if (ring_batch && c->last_settled_lo && c->last_settled_lo > c->last_rel_rows && c->last_settled_hi < c->last_rel_rows + (size_t)nframes * (size_t)n)
    return fail(c, SS_ERR_INVALID, "tracked feed (ring): rows in the middle of the batch were settled since it ran: nothing a call leaves looks like that");
  const uint32_t seq = (uint32_t)t->next_seq, p = (uint32_t)t->post_seq;
  const int nkeys = (int)t->post_keys.size();
  if (nkeys > 0) {
    memcpy(s.h_keys.get(), t->post_keys.data(), sizeof(int32_t) * (size_t)nkeys);
    SS_HIP(c, hipMemcpyAsync(s.d_keys.get(), s.h_keys.get(), sizeof(int32_t) * (size_t)nkeys, hipMemcpyHostToDevice, c->stream));
  }
  const uint32_t *d_mark = t->d_mark.get(), *d_keymark = t->d_keymark.get();
  const int32_t* d_coff = s.d_coff.get();
  ss::FeedPrepareArgs pa{};
  pa.off = fs.d_off.get();
  pa.coff = s.d_coff.get();
  pa.keys = s.d_keys.get();
  pa.keymark = t->d_keymark.get();
  pa.hdr = s.d_hdr.get();
  pa.nframes = nframes;
  pa.cand_cap = f->cand_cap;
  pa.nkeys = nkeys;
  pa.seq = seq;
  hipLaunchKernelGGL(ss::k_feed_prepare, dim3((unsigned)grid_for((size_t)std::max(nframes + 1, nkeys), 256)), dim3(256), 0, c->stream, pa);
  // one of the two sources, fixed here: the kernels take it by value, so what the host does to last_* later does not reach them
  const ss::RelRows rows = ring_batch ? ss::RelRows{} : rel_rows(c, t->rows);
  const ss::RingRows ring = ring_batch ? ring_rows(c, t->rows, nframes) : ss::RingRows{};
  if (ring_batch) launch_cand_best(c, t->rows, ring, nframes, d_coff, fs.d_idx.get(), s.d_best.get(), s.d_cavg.get());
  else launch_cand_best(c, t->rows, rows, nframes, d_coff, fs.d_idx.get(), s.d_best.get(), s.d_cavg.get());
  hipLaunchKernelGGL(ss::k_feed_stamp, dim3((unsigned)std::min(grid_for((size_t)f->cand_cap, 256), 1024)), dim3(256), 0, c->stream, d_coff, nframes,
                     (const int32_t*)s.d_best.get(), t->d_mark.get(), n, seq, s.d_hdr.get());
  hipLaunchKernelGGL(ss::k_feed_count, dim3((unsigned)t->nblocks), dim3(ss::kFeedBlock), 0, c->stream, d_mark, d_keymark, n, p, seq, t->d_counts.get());
  hipLaunchKernelGGL(ss::k_feed_scan, dim3(1), dim3(64), 0, c->stream, t->d_counts.get(), t->nblocks, (const int32_t*)fs.d_off.get(), d_coff, nframes, t->cfg.max_watch,
                     s.d_hdr.get());
  hipLaunchKernelGGL(ss::k_feed_scatter, dim3((unsigned)t->nblocks), dim3(ss::kFeedBlock), 0, c->stream, d_mark, d_keymark, n, p, seq, (const int32_t*)t->d_counts.get(),
                     t->cfg.max_watch, s.d_watch.get());
  if (t->sparse) {
    const int st = stf_replay_watch_tiles(t, s, nframes, src);
    if (st != SS_OK) return st;
  }
  ss::FeedPeaksArgs pk{};
  pk.avg = c->last_avg;
  pk.watch = s.d_watch.get();
  pk.hdr = s.d_hdr.get();
  pk.peak_idx = s.d_pidx.get();
  pk.peak_avg = s.d_pavg.get();
  pk.n = n;
  pk.nframes = nframes;
  pk.half = t->rows.group_size / 2;
  // (the list's length is known to the device only: enough workgroups to fill the machine, each walks its share)
  const size_t most = ((size_t)nframes * (size_t)t->cfg.max_watch + 3) / 4;
  hipLaunchKernelGGL(ss::k_feed_peaks, dim3((unsigned)std::min<size_t>(most, 2048)), dim3(256), 0, c->stream, pk);
  if (ring_batch) launch_save_tail(c, t->rows, ring, nframes);
  else launch_save_tail(c, t->rows, rows, nframes);
  flip_tail(t->rows);  // (stream order: the next batch's digest reads what this one wrote)
  SS_HIP(c, hipGetLastError());
  SS_HIP(c, hipMemcpyAsync(s.h_hdr.get(), s.d_hdr.get(), sizeof(ss::FeedDigestHeader), hipMemcpyDeviceToHost, c->stream));
  s.seq = t->next_seq++;
  s.keys_seq = t->post_seq;
  return SS_OK;
}

// feed_collect, under the context's lock, behind the batch's ev_done and the candidate copies: the header the batch's digest left is
// checked against the batch, then exactly what it counts is read back on the feed's read-back stream (feed_collect waits for it).
int stf_collect_digest(ss_feed* f, int slot_no, int nframes, int ncopy, stf_result* digest, bool* copies) {
  stf_ctx* t = static_cast<stf_ctx*>(f->tracker);
  ss_ctx* c = f->c;
  stf_slot& d = t->slots[(size_t)slot_no];
  const ss::FeedDigestHeader h = *d.h_hdr.get();
  if (h.ncand != ncopy || h.nwatch < 0 || (h.flags & ss::kFeedBadBest))
    return fail(c, SS_ERR_HIP, "tracked feed: the digest's header does not fit the batch (ncand %d / %d, nwatch %d, flags %d)", h.ncand, ncopy, h.nwatch, h.flags);
  const bool over = (h.flags & ss::kFeedOverflow) != 0 || h.nwatch > t->cfg.max_watch;
  const size_t nw = over ? 0 : (size_t)h.nwatch, items = nw * (size_t)nframes;
  if (ncopy > 0) {
    SS_HIP(c, hipMemcpyAsync(d.h_best.get(), d.d_best.get(), sizeof(int32_t) * (size_t)ncopy, hipMemcpyDeviceToHost, f->d2h_stream));
    SS_HIP(c, hipMemcpyAsync(d.h_cavg.get(), d.d_cavg.get(), sizeof(float) * (size_t)ncopy, hipMemcpyDeviceToHost, f->d2h_stream));
  }
  if (nw > 0) {
    SS_HIP(c, hipMemcpyAsync(d.h_watch.get(), d.d_watch.get(), sizeof(int32_t) * nw, hipMemcpyDeviceToHost, f->d2h_stream));
    SS_HIP(c, hipMemcpyAsync(d.h_pidx.get(), d.d_pidx.get(), sizeof(int32_t) * items, hipMemcpyDeviceToHost, f->d2h_stream));
    SS_HIP(c, hipMemcpyAsync(d.h_pavg.get(), d.d_pavg.get(), sizeof(float) * items, hipMemcpyDeviceToHost, f->d2h_stream));
    *copies = true;
  }
  digest->seq = d.seq;
  digest->keys_seq = d.keys_seq;
  digest->status = over ? SS_ERR_INVALID : SS_OK;
  digest->ncand = ncopy;
  digest->nwatch = h.nwatch;
  digest->cand_best = d.h_best.get();
  digest->cand_avg = d.h_cavg.get();
  digest->watch = d.h_watch.get();
  digest->peak_idx = d.h_pidx.get();
  digest->peak_avg = d.h_pavg.get();
  digest->d2h_bytes = sizeof(ss::FeedDigestHeader) + 8ull * (uint64_t)ncopy + 4ull * nw + 8ull * items;
  t->collected = d.seq;
  return SS_OK;
}

// ss_feed_submit, under the context's lock, in front of run_batch: the batch goes through as a call that may keep no dB plane
// (call_route.h: CallAsk::device — what the fold, the culled chains and the ring-only calls ask for) when a ring tracker is bound and
// nothing else on the feed reads the plane. Below 65536 points no such form exists, and an 8192-point call of that kind would
// overlap on the library's own queues: those stay what they are through any feed.
// A ring spectrogram object (sgf_create_ring) reads such a batch's rows where the ring tracker does, and switches the feed alone as
// well; a plane-kind one (sgf_create) reads the plane and keeps every batch on it.
bool stf_wants_no_plane_calls(const ss_feed* f) {
  const stf_ctx* t = static_cast<const stf_ctx*>(f->tracker);
  const bool ring_rows = f->spectrogram && sgf_reads_ring_rows(f);
  return ((t && t->ring) || ring_rows) && f->c->n >= 65536 && !f->want_psd && (!f->spectrogram || ring_rows);
}

// stf_create, stf_create_sparse and stf_create_ring: allow_sparse = the context may lack SS_FLAG_KEEP_PLANES (the object is a sparse one
// if it does); allow_ring = ... at 65536 points and up too (the object then digests ring batches)
int stf_create_any(ss_feed* f, const stf_config* cfg, stf_ctx** out, bool allow_sparse, bool allow_ring = false) {
  if (create_args_refused(f, cfg, out, STF_ABI_VERSION)) return SS_ERR_INVALID;
  if (cfg->group_size < 0 || cfg->max_watch <= 0) return obj_fail<stf_ctx>(nullptr, SS_ERR_INVALID, "group_size >= 0 and max_watch > 0 required");
  ss_ctx* c = f->c;
  std::lock_guard<std::mutex> lock(c->mtx);
  const bool sparse = allow_sparse && !(c->cfg.flags & SS_FLAG_KEEP_PLANES);
  if (!allow_sparse && !(c->cfg.flags & SS_FLAG_KEEP_PLANES)) return obj_fail<stf_ctx>(nullptr, SS_ERR_INVALID, "the scan context needs SS_FLAG_KEEP_PLANES (the digest reads the kept dB and avg planes)");
  if (sparse && !c->fused)
    return obj_fail<stf_ctx>(nullptr, SS_ERR_INVALID, "sparse tracking needs the fused back end (grouping 21 x 21; this context has %d x %d): the unfused back end keeps no sparse avg plane",
                             c->cfg.grouping_x, c->cfg.grouping_y);
  if (sparse && c->ref_nan) return obj_fail<stf_ctx>(nullptr, SS_ERR_INVALID, "sparse tracking on a SS_FLAG_REFERENCE_NAN context: its NaN stage patches the planes behind the tiles");
  if (sparse && !allow_ring && c->n >= 65536) return obj_fail<stf_ctx>(nullptr, SS_ERR_INVALID, "sparse tracking at fft_size %d: 65536 points and up can leave no bin-ordered dB plane (32768 at most)", c->n);
  if (f->cand_cap <= 0) return obj_fail<stf_ctx>(nullptr, SS_ERR_INVALID, "the feed was created with cand_cap 0: there are no candidate lists to digest");
  if (feed_already_has<stf_ctx>(f->tracker, "a tracker") || feed_busy<stf_ctx>(f)) return SS_ERR_INVALID;
  digest_rows rows;
  if (const int st = digest_rows_plan(rows, c, cfg->group_size, cfg->start_level, create_err<stf_ctx>()); st != SS_OK) return st;
  stf_ctx* t = new (std::nothrow) stf_ctx();
  if (!t) return obj_fail<stf_ctx>(nullptr, SS_ERR_NOMEM, "out of memory");
  t->scan = c;
  t->feed = f;
  t->cfg = *cfg;
  t->rows = std::move(rows);
  t->sparse = sparse;
  t->ring = sparse && allow_ring;
  t->nblocks = (c->n + ss::kFeedBlock - 1) / ss::kFeedBlock;
  t->slots.resize((size_t)f->ring.depth());
  const size_t n = (size_t)c->n, frames = (size_t)c->cfg.max_batch, cap = (size_t)f->cand_cap, mw = (size_t)cfg->max_watch, nblocks = (size_t)t->nblocks;
  ss::hip_steps made;
  made.then([&] { return hipSetDevice(c->cfg.device_id); }).then([&] { return tails_alloc(t->rows, c); });
  made.alloc(t->d_mark, n).alloc(t->d_keymark, n).alloc(t->d_counts, nblocks);
  for (auto& s : t->slots) {
    made.alloc(s.d_coff, frames + 1).alloc(s.d_hdr, 1).alloc(s.d_best, cap).alloc(s.d_cavg, cap).alloc(s.d_watch, mw).alloc(s.d_keys, mw);
    made.alloc(s.d_pidx, frames * mw).alloc(s.d_pavg, frames * mw);
    made.alloc(s.h_hdr, 1).alloc(s.h_best, cap).alloc(s.h_cavg, cap).alloc(s.h_watch, mw).alloc(s.h_keys, mw).alloc(s.h_pidx, frames * mw).alloc(s.h_pavg, frames * mw);
  }
  if (sparse) {
    const size_t words = (n / 32) * frames, plane = sizeof(float) * n * frames;
    made.alloc(t->d_sp_mask, words).alloc(t->d_sp_counts, frames).alloc(t->d_col_flag, nblocks).alloc(t->d_sp_evaluated, 1);
    made.then([&] { return hipMemsetAsync(t->d_sp_mask.get(), 0, sizeof(uint32_t) * words, c->stream); });
    made.then([&] { return hipMemsetAsync(t->d_sp_counts.get(), 0, sizeof(int) * frames, c->stream); });
    made.then([&] { return hipMemsetAsync(t->d_col_flag.get(), 0, sizeof(int32_t) * nblocks, c->stream); });
    // every sparse plane to NaN, once (all bytes 0xff): a cell of a watch window the replay failed to write would be a NaN peak, not a
    // plausible value some earlier batch left there. Nothing pending (checked above); the planes are max_batch x n floats each.
    flush_stages(c);
    for (int k = 0; k < c->nbuf; ++k) made.then([&] { return hipMemsetAsync(c->d_avg2[k], 0xff, plane, c->stream); });
  }
  made.then([&] { return stf_clear(t); });
  if (!made.ok()) {
    delete t;
    return obj_fail<stf_ctx>(nullptr, SS_ERR_NOMEM, "allocating the tracked feed's buffers failed: %s", hipGetErrorString(made.error()));
  }
  f->tracker = t;
  *out = t;
  return SS_OK;
}

}  // namespace

extern "C" {

int stf_create(ss_feed* f, const stf_config* cfg, stf_ctx** out) { return stf_create_any(f, cfg, out, false); }

int stf_create_sparse(ss_feed* f, const stf_config* cfg, stf_ctx** out) { return stf_create_any(f, cfg, out, true); }

int stf_create_ring(ss_feed* f, const stf_config* cfg, stf_ctx** out) { return stf_create_any(f, cfg, out, true, true); }

int stf_sparse_stats(stf_ctx* t, uint64_t* tiles_evaluated, uint64_t* tiles_in_batches) {
  if (!t) return SS_ERR_INVALID;
  if (!tiles_evaluated || !tiles_in_batches) return obj_fail(t, SS_ERR_INVALID, "null argument");
  ss_ctx* c = t->scan;
  std::lock_guard<std::mutex> lock(c->mtx);
  if (!t->sparse) return obj_fail(t, SS_ERR_INVALID, "not a sparse object: the scan context keeps its planes (stf_create, or stf_create_sparse with SS_FLAG_KEEP_PLANES), nothing is replayed");
  if (feed_destroyed(t)) return SS_ERR_INVALID;
  unsigned long long ev = 0;
  if (hipSetDevice(c->cfg.device_id) != hipSuccess || hipMemcpyAsync(&ev, t->d_sp_evaluated.get(), sizeof(ev), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess)
    return obj_fail(t, SS_ERR_HIP, "reading the replay's counter failed: %s", hipGetErrorString(hipGetLastError()));
  *tiles_evaluated = ev;
  *tiles_in_batches = t->sp_tiles_in_batches;
  return SS_OK;
}

void stf_destroy(stf_ctx* t) {
  if (!t) return;
  {
    std::lock_guard<std::mutex> lock(t->scan->mtx);
    (void)hipSetDevice(t->scan->cfg.device_id);
    if (t->feed) {  // (a destroyed feed has waited for its streams already)
      (void)hipStreamSynchronize(t->scan->stream);
      (void)hipStreamSynchronize(t->feed->d2h_stream);
      t->feed->tracker = nullptr;
    }
  }
  delete t;
}

const char* stf_last_error(const stf_ctx* t) { return t ? t->err : create_err<stf_ctx>(); }

int stf_post_keys(stf_ctx* t, uint64_t seq, const int32_t* keys, int32_t nkeys) {
  if (!t) return SS_ERR_INVALID;
  if (nkeys < 0 || (nkeys > 0 && !keys)) return obj_fail(t, SS_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(t->scan->mtx);
  if (feed_destroyed(t)) return SS_ERR_INVALID;
  if (seq > t->collected) return obj_fail(t, SS_ERR_INVALID, "keys after batch %llu, but the newest collected batch is %llu: not collected yet", (unsigned long long)seq, (unsigned long long)t->collected);
  if (seq < t->post_seq) return obj_fail(t, SS_ERR_INVALID, "keys after batch %llu are older than the last post (%llu)", (unsigned long long)seq, (unsigned long long)t->post_seq);
  if (nkeys > t->cfg.max_watch) return obj_fail(t, SS_ERR_INVALID, "%d keys > max_watch %d", nkeys, t->cfg.max_watch);
  for (int k = 0; k < nkeys; ++k)
    if (keys[k] < 0 || keys[k] >= t->scan->n) return obj_fail(t, SS_ERR_INVALID, "key %d: bin %d outside [0, %d)", k, keys[k], t->scan->n);
  t->post_seq = seq;
  t->post_keys.assign(keys, keys + nkeys);
  return SS_OK;
}

int stf_collect(stf_ctx* t, stf_result* out) {
  if (!t) return SS_ERR_INVALID;
  if (!out) return obj_fail(t, SS_ERR_INVALID, "null argument");
  ss_feed* f = nullptr;
  {
    std::lock_guard<std::mutex> lock(t->scan->mtx);
    if (feed_destroyed(t)) return SS_ERR_INVALID;
    f = t->feed;
  }
  const int st = feed_collect(f, &out->batch, out);
  if (st != SS_OK) {
    std::lock_guard<std::mutex> lock(t->scan->mtx);
    return obj_fail(t, st, "%s", t->scan->err);
  }
  return SS_OK;
}

int stf_reset(stf_ctx* t) {
  if (!t) return SS_ERR_INVALID;
  ss_ctx* c = t->scan;
  std::lock_guard<std::mutex> lock(c->mtx);
  if (feed_destroyed(t)) return SS_ERR_INVALID;
  if (!t->feed->ring.idle()) return obj_fail(t, SS_ERR_INVALID, "stf_reset with batches pending: collect them first");
  if (hipSetDevice(c->cfg.device_id) != hipSuccess || stf_clear(t) != hipSuccess) return obj_fail(t, SS_ERR_HIP, "clearing the kept rows and marks failed: %s", hipGetErrorString(hipGetLastError()));
  t->rows.tail_cur = 0;
  return SS_OK;
}

}  // extern "C"
