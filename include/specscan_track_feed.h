/*
 * specscan_track_feed.h — C ABI of the tracking digest behind the pipelined feed, part of libspecscan.so.
 *
 * st_digest (specscan_track.h) serves the synchronous ss_process: it takes the batch's lists and the tracker's keys from the
 * host and waits twice. An stf_ctx bound to an ss_feed digests every batch submitted through that feed IN THE STREAM, right
 * behind the batch's chain and with no host wait in between, and stf_collect delivers the digest with the batch.
 *
 * The watch list is a superset. While earlier batches are in flight the host cannot know the tracker's keys at the start of
 * batch k — but a key enters the tracker only as getBestIndex(c) of a candidate c of the current frame
 * (transmission.cpp:97-108) and leaves it only through clearSignals, so for any earlier batch p
 *
 *     keys at the start of batch k  is a subset of  K_p U cand_best(p + 1) U ... U cand_best(k - 1)
 *
 * (K_p: the tracker's keys after batch p). cand_best does not depend on the tracker, so the device forms
 *
 *     W_k = sort(unique(K_p U cand_best(p + 1) U ... U cand_best(k)))
 *
 * from the newest key set (p, K_p) the host had posted when batch k was submitted (nothing posted: p = 0, K_0 empty).
 * SignalTracker::processFrameDigest looks its keys up in the ascending watch list and ignores the rest, so it gives on W_k
 * what it gives on the exact list. Post the keys after every collect and W_k stays a handful of keys larger than needed; never
 * post and it grows to every bin that ever was a cand_best, until max_watch is exceeded.
 *
 * Use: ss_feed_create, stf_create; a producer thread goes on with ss_feed_acquire / ss_feed_submit and knows nothing of the
 * tracker; the consumer calls stf_collect (not ss_feed_collect), runs the batch's frames through processFrameDigest and calls
 * stf_post_keys(result.seq, tracker keys). Every entry point takes the scan context's mutex; any thread may call any of them.
 * The scan context must outlive the stf_ctx. ss_feed_destroy before stf_destroy is allowed: the stf_ctx then only accepts
 * stf_destroy and stf_last_error (pointers of earlier results stay valid until stf_destroy).
 *
 * ss_reset and ss_set_frequency_range go with stf_reset, as they go with st_reset — and both need the feed drained first
 * (every submitted batch collected): a batch in flight was digested with the rows and marks the reset would wipe.
 *
 * stf_create wants a scan context with SS_FLAG_KEEP_PLANES: every batch then writes its avg plane and no averaging tile is culled.
 * specscan_track_sparse.h has stf_create_sparse for a context without the flag — the scan stays on its culled path, writes no avg
 * plane, and only the tile columns the watch windows touch are evaluated once more behind the batch — and stf_sparse_stats. Every
 * other name of this header serves both kinds of object, and the digest is the same bit for bit.
 *
 * The device counts batches in 32 bits: a submit that would pass sequence number 2^32 - 1 without stf_reset fails with
 * SS_ERR_INVALID.
 *
 * Footprint, per slot of the feed: 8 B x cand_cap (cand_best, cand_avg) + 4 B x max_watch (watch list) + 4 B x max_watch
 * (the posted keys on their way up) + 8 B x max_batch x max_watch (peaks), each once on the device and once pinned;
 * per tracker 8 B x N for the two mark arrays, 4 B x N / 256 of block counts and the kept rel rows
 * (2 x 4 B x N x (ceil(grouping_y / 2) - 1)).
 */
#ifndef SPECSCAN_TRACK_FEED_H
#define SPECSCAN_TRACK_FEED_H

#include <stdint.h>

#include "specscan.h"
#include "specscan_track.h"

#ifdef __cplusplus
extern "C" {
#endif

#define STF_ABI_VERSION 1u

typedef struct stf_ctx stf_ctx;

typedef struct stf_config {
  uint32_t abi_version; /* STF_ABI_VERSION */
  int32_t group_size;   /* as st_config::group_size */
  float start_level;    /* as st_config::start_level */
  int32_t max_watch;    /* capacity of the watch list, and the most keys stf_post_keys takes */
} stf_config;

/* Pointers: pinned host memory of the object, valid until the batch's slot is acquired again (ss_feed_acquire). */
typedef struct stf_result {
  ss_feed_result batch;     /* exactly what ss_feed_collect gives for this batch */
  uint64_t seq;             /* 1, 2, 3 ... since stf_create / stf_reset */
  uint64_t keys_seq;        /* p: the posted key set W was built from (0: none) */
  int32_t status;           /* SS_OK, or SS_ERR_INVALID: more than max_watch watch keys — watch and peaks not valid, nwatch is the true count */
  int32_t ncand, nwatch;    /* ncand = min(cand_off[nframes], the feed's cand_cap) */
  const int32_t* cand_best; /* [ncand] getBestIndex of every candidate, in list order */
  const float* cand_avg;    /* [ncand] avg[f][c], gathered from the avg plane as st_digest does */
  const int32_t* watch;     /* [nwatch] ascending */
  const int32_t* peak_idx;  /* [nframes][nwatch] */
  const float* peak_avg;    /* [nframes][nwatch] */
  uint64_t d2h_bytes;       /* bytes the digest moved from the device to the host */
} stf_result;

/* From here on every batch submitted through feed is digested. SS_ERR_INVALID, with a message that names the reason
 * (stf_last_error(NULL)): the scan context was created without SS_FLAG_KEEP_PLANES; the feed has cand_cap 0, has batches
 * pending or has a tracker already; max_watch <= 0; one rel row of a 256-bin tile with its tables does not fit 64 KiB of
 * LDS (as st_create: group_size up to about 6500 bins with grouping_y = 21). */
int stf_create(ss_feed* feed, const stf_config* cfg, stf_ctx** out);
void stf_destroy(stf_ctx* ctx);
const char* stf_last_error(const stf_ctx* ctx); /* NULL: the last stf_create failure of this thread */

/* "These are the tracker's keys after it has processed batch seq" (any order, duplicates allowed). Batches submitted from now
 * on watch them. SS_ERR_INVALID when seq is newer than the newest collected batch or older than the last post, for more
 * than max_watch keys and for a key outside [0, N). */
int stf_post_keys(stf_ctx* ctx, uint64_t seq, const int32_t* keys, int32_t nkeys);

/* The oldest pending batch and its digest; blocks until it is done, as ss_feed_collect does (which a tracked feed refuses). */
int stf_collect(stf_ctx* ctx, stf_result* out);

/* Transmission::resetBuffers: the kept rel rows, the marks and the post back to zero; seq restarts at 1. Needs nothing pending. */
int stf_reset(stf_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif
