/*
 * specscan_track_feed_ring.h — the tracked feed (specscan_track_feed.h) at the reference's own transform sizes, part of libspecscan.so.
 *
 * The reference picks its transform from the sample rate (radio_utils.cpp:98-104: 131072 points at 20 MS/s, 262144 at 61.44 MS/s).
 * At 65536 points and up the scan's fast forms — the radix-8 / radix-16 int8 fold, the culled chains, the ring-only calls — write no
 * dB plane at all: a batch's rows go straight to the averager ring's buffer, as dB values, after a fold in the fold's blocked order.
 * stf_create keeps the scan off those forms (SS_FLAG_KEEP_PLANES), and so does every batch that goes through a feed as an ordinary
 * call; stf_create_sparse refuses the sizes outright.
 *
 * An object made by stf_create_ring lets its feed's batches take those forms, and digests a batch that kept no plane where it lies:
 * cand_best and the kept rows from the rows in the ring's buffer (the reads ss_read_window(SS_PLANE_REL) makes on the host), the
 * window peaks from a replay of the tile columns the watch windows touch, with the tile of the form the batch took. A batch that did
 * leave a bin-ordered dB plane — learning frames (noise_learner.cpp:11-28), a feed created with want_psd, a feed with spectrogram
 * rows — is digested as stf_create_sparse digests it, and the two kinds of batch may follow each other in any order. Every number of
 * stf_result is the one st_digest gives on an st_create_sparse object for the same calls, bit for bit; the scan's ss_get_stats tile
 * counters are those of the same calls made through ss_process_device, and do not move for the replay.
 *
 * Everything else is specscan_track_feed.h's and specscan_track_sparse.h's: stf_config, stf_result, stf_collect, stf_post_keys,
 * stf_reset, stf_destroy, stf_last_error and stf_sparse_stats serve the object unchanged, STF_ABI_VERSION is unchanged.
 *
 * Footprint: stf_create_sparse's — 4 B x (N / 32) x max_batch of scratch mask words, 4 B x max_batch of scratch counts, 4 B x N / 256 of
 * column flags and one 8-byte counter on top of stf_create's 8 B x N of marks and 2 x 10 x 4 B x N of kept rows. No plane is added,
 * and none is written: at 131072 points and 128-frame batches that is 64 MiB per batch the scan does not store.
 */
#ifndef SPECSCAN_TRACK_FEED_RING_H
#define SPECSCAN_TRACK_FEED_RING_H

#include <stdint.h>

#include "specscan_track_sparse.h"

#ifdef __cplusplus
extern "C" {
#endif

/* stf_create_sparse without its limit of 32768 points. Below 65536 points, and for every batch whose call left a bin-ordered dB
 * plane, the object behaves as stf_create_sparse's; on a context with SS_FLAG_KEEP_PLANES it is simply stf_create. While the object
 * is bound, a batch of 65536 points and up goes through the feed as ss_process_device makes its calls (no plane kept where the form
 * keeps none) unless the feed was created with want_psd or carries sgf_create's spectrogram rows (sgf_create_ring's read the ring's
 * buffer too: specscan_spectrogram_feed_ring.h). SS_ERR_INVALID, with the messages of
 * stf_create_sparse (stf_last_error(NULL)): the unfused back end, SS_FLAG_REFERENCE_NAN, a feed with cand_cap 0, a feed with
 * batches pending, a feed that has a tracker already, and everything stf_create refuses. */
int stf_create_ring(ss_feed* feed, const stf_config* cfg, stf_ctx** out);

#ifdef __cplusplus
}
#endif
#endif
