/*
 * specscan_record_feed.h — C ABI of the recorder bound to the pipelined feed, part of libspecscan.so.
 *
 * A tracked feed (specscan_track_feed.h) uploads every batch once and hands the tracker's lists back for kilobytes. Recording
 * what the tracker found would otherwise mean sending the same samples over PCIe a second time (sc_process), and a recording
 * could only begin with the batch after the one that raised it. An srf_ctx bound to an ss_feed owns a channeliser
 * (specscan_channelizer.h) and runs it on the samples that are still on the device when a batch is collected: the feed slot's
 * own upload. The host reads the batch's per-frame lists, turns them into sample ranges of that batch (sc_range: frame f is
 * samples f * N .. (f + 1) * N) and records them with srf_record — including the frames the transmission was found in, which
 * the reference's Recorder never sees (it records what arrives after startRecording, recorder.cpp:58-73).
 *
 * Hold: while a recorder is bound, ss_feed_collect / stf_collect leave the collected slot HELD. ss_feed_acquire never hands out a
 * held slot (it fails with "no free feed slot" when the held one is next), and the next collect is refused until srf_record
 * or srf_release has let the held batch go. With a feed of depth 2 the producer can still fill the other slot meanwhile.
 *
 * Decimated scans: an ordinary feed (ss_feed_create) of a context with decim != 1 takes compact frames, the first N samples of
 * every N * decim item, so the samples between them never reach the feed and there is no stream to record from: srf_create
 * refuses it. A whole-item feed (ss_feed_create_items, specscan.h) keeps every item in the slot's pinned host memory and still
 * uploads only the frames for the scan. On such a feed srf_record works on the batch's item stream, nframes * N * decim
 * samples (frame f is samples f * N * decim .. f * N * decim + N, the rest of its item follows it): it uploads the union of the
 * ranges it is given from the held slot's pinned items (sc_process_ranges_upload) and channelises them where they land. What
 * crosses PCIe for recording is what is recorded; a batch that is released costs nothing. With decim == 1 the items are the
 * frames, and either kind of feed records from the slot's device upload without a copy.
 *
 * Threads: srf_record is synchronous (it follows the host's tracking anyway) and takes the scan context's mutex only around
 * the slot bookkeeping, so a producer thread keeps acquiring and submitting while a batch is recorded. One thread records.
 * The scan context must outlive the srf_ctx. ss_feed_destroy before srf_destroy is allowed: the srf_ctx then only accepts
 * srf_destroy and srf_last_error.
 */
#ifndef SPECSCAN_RECORD_FEED_H
#define SPECSCAN_RECORD_FEED_H

#include <stdint.h>

#include "specscan.h"
#include "specscan_channelizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRF_ABI_VERSION 2u

typedef struct srf_ctx srf_ctx;

typedef struct srf_config {
  uint32_t abi_version; /* SRF_ABI_VERSION */
  int32_t bandwidth;    /* as sc_config::bandwidth */
  int32_t threshold;    /* as sc_config::threshold (RESAMPLER_THRESHOLD, 125) */
  int32_t channels;     /* recording slots, 1..SC_MAX_CHANNELS */
  float pack_scale;     /* as sc_config::pack_scale (127.0) */
  int32_t want_cf32;    /* also deliver the last resampler's float output */
} srf_config;

/* Pointers: pinned host memory of the object, valid until the next srf_record / srf_destroy. */
typedef struct srf_result {
  int32_t nsamples, cap;       /* nframes * N * decim of the held batch; sc_output_capacity of the largest batch */
  const int32_t* counts;       /* [channels] */
  const int32_t* range_counts; /* [nranges] */
  const int8_t* out_i8;        /* [channels][cap][2] */
  const float* out_cf32;       /* [channels][cap][2], NULL unless want_cf32 */
  uint64_t h2d_bytes;          /* uploaded by this srf_record: bytes per sample * the union of the ranges; 0 when decim == 1 */
} srf_result;

/* Sample rate, input format, int_scale and device are the scan context's; the channeliser's max_samples is
 * max_batch * N * decim. SS_ERR_INVALID with a message (srf_last_error(NULL)): the scan context has decim != 1 and the feed
 * is not a whole-item feed (see above); max_batch * N * decim does not fit int32_t; the feed has batches pending or a slot
 * acquired; the feed has a recorder already; anything sc_create refuses (its status and message). */
int srf_create(ss_feed* feed, const srf_config* cfg, srf_ctx** out);
void srf_destroy(srf_ctx* ctx);
const char* srf_last_error(const srf_ctx* ctx); /* NULL: the last srf_create failure of this thread */

/* sc_process_ranges_device on the held batch (its rules for ranges; begin / end in samples of the batch's stream, see above;
 * on a whole-item feed of a decimated context sc_process_ranges_upload from the slot's pinned items), exactly counts[ch]
 * outputs per channel copied to pinned memory, and the batch let go. Returns when the outputs are there. A refused call
 * (no batch held, a bad range list) changes nothing and keeps the batch held. nranges == 0 is srf_release. */
int srf_record(srf_ctx* ctx, const sc_range* ranges, int32_t nranges, srf_result* out);
/* Let the held batch go without recording from it. SS_ERR_INVALID when none is held. */
int srf_release(srf_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif
