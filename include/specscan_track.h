/*
 * specscan_track.h — C ABI of the tracking digest, part of libspecscan.so.
 *
 * The host-side signal tracker (host/signal_tracker.h; the reference's Transmission::process, transmission.cpp:57-68)
 * reads very little of a batch's rel and avg planes:
 *
 *   1. getBestIndex(c) for a candidate c (transmission.cpp:132-154): the mode of the window arg-maxes of the newest
 *      ceil(grouping_y / 2) rel rows — a function of c, the frame and the rows, not of the tracker's state;
 *   2. updateSignals (:113-130): arg-max and maximum of the frame's avg row over the window of every tracked key;
 *   3. the candidates' own avg values (the sort key of :95).
 *
 * Every key the tracker can hold during a batch is alive when the batch starts or is getBestIndex(c) of one of the
 * batch's candidates. An st_ctx computes that digest on the device, next to the planes of the ss_ctx it is bound to:
 * one int and one float per candidate, and (index, value) per frame for a short, ascending watch list of keys —
 * kilobytes over PCIe where the two planes are 8 B/sample. SignalTracker::processFrameDigest
 * (sst_process_frame_digest) runs the unchanged bookkeeping on it and gives what processFrame gives on the planes.
 *
 * The price, in this version: the scan context must be created with SS_FLAG_KEEP_PLANES — the avg plane is kept on
 * the device (4 B/sample of HBM writes) and such a context takes neither the int8 fold nor the detect-mode calls
 * that write no dB plane. That is still two planes less over PCIe than the plane route.
 *
 * Use: after every batch (ss_process, or ss_process_device + ss_sync) call st_digest once with the batch's candidate
 * lists and the tracker's current keys (SignalTracker::signalKeys). The object keeps the batch's last
 * ceil(grouping_y / 2) - 1 rel rows for the next batch's first frames, so a batch that went by without st_digest
 * makes the next st_digest fail until st_reset. Call st_reset with ss_reset. The ss_feed_* pipeline (several
 * batches in flight: the last batch is not the collected one) has its own form of the digest: specscan_track_feed.h.
 */
#ifndef SPECSCAN_TRACK_H
#define SPECSCAN_TRACK_H

#include <stdint.h>

#include "specscan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ST_ABI_VERSION 1u

typedef struct st_ctx st_ctx;

typedef struct st_config {
  uint32_t abi_version; /* ST_ABI_VERSION */
  int32_t group_size;   /* indexStep = ceil(recordingBandwidth / (fs / N)), sdr_device.cpp:151: windows are [k - g/2, k + g/2] */
  float start_level;    /* Device::m_startLevel: a rel row counts for getBestIndex when start_level <= row[arg-max] */
  int32_t max_watch;    /* capacity of the watch list (keys + distinct cand_best) */
  int32_t cand_cap;     /* the most candidates a batch may bring (a limit: buffers grow with what comes) */
} st_config;

/* Pinned host memory of the object, valid until the next st_digest / st_destroy. */
typedef struct st_result {
  int32_t nframes, ncand, nwatch;
  const int32_t* cand_best; /* [ncand] getBestIndex of every candidate, in list order */
  const float* cand_avg;    /* [ncand] avg[f][c], the avg plane's own float */
  const int32_t* watch;     /* [nwatch] sort(unique(keys U cand_best)), ascending */
  const int32_t* peak_idx;  /* [nframes][nwatch] arg-max of avg[f] over the window of watch[w] (first maximum) */
  const float* peak_avg;    /* [nframes][nwatch] avg[f][peak_idx] */
  uint64_t d2h_bytes;       /* bytes this digest moved from the device to the host */
} st_result;

/* Binds a digest object to a scan context (which must outlive it). SS_ERR_INVALID unless scan was created with
 * SS_FLAG_KEEP_PLANES, for a bad config, or when one rel row of a 256-bin tile with its tables (8 B for each of
 * 256 + group_size bins) and the lanes' lists (1 KiB for each of ceil(grouping_y / 2) rows) do not fit the 64 KiB of LDS a
 * workgroup may use: group_size up to about 6500 bins with grouping_y = 21. Errors of st_create: st_last_error(NULL). */
int st_create(ss_ctx* scan, const st_config* cfg, st_ctx** out);
void st_destroy(st_ctx* ctx);
const char* st_last_error(const st_ctx* ctx);

/* Transmission::resetBuffers: the kept rel rows back to zero (as SignalTracker::reset zeroes its ring). */
int st_reset(st_ctx* ctx);

/* The digest of the LAST batch of the scan context. cand_off [nframes + 1] / cand_idx: the host lists as ss_process (or
 * ss_process_device + ss_sync and the caller's copy) left them; after SS_ERR_CAND_OVERFLOW the digest covers the truncated lists
 * (offsets clipped to the capacity that call was given). keys [nkeys]: the tracker's keys before the batch's first frame, any order.
 * Drains the context's deferred stages and returns when the result is in host memory. SS_ERR_INVALID, with nothing changed,
 * when no batch has been processed since ss_reset, when a batch went by without st_digest (until st_reset), after
 * ss_reset_noise or ss_set_frequency_range between the batch and this call, for more than cand_cap candidates or more
 * than max_watch watch keys, and for a candidate or key outside [0, N). */
int st_digest(st_ctx* ctx, const int32_t* cand_off, const int32_t* cand_idx, const int32_t* keys, int32_t nkeys, st_result* out);

#ifdef __cplusplus
}
#endif
#endif
