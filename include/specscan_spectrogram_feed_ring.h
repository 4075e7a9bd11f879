/*
 * specscan_spectrogram_feed_ring.h — the feed's spectrogram rows (specscan_spectrogram_feed.h) at the reference's own transform
 * sizes, part of libspecscan.so.
 *
 * The reference runs its Spectrogram branch beside the scan at every size (sources/radio/sdr_device.cpp:170-171): 131072 points at
 * 20 MS/s, 262144 at 61.44 MS/s (utils/radio_utils.cpp:98-104). At 65536 points and up the scan's fast forms — the radix-8 /
 * radix-16 int8 fold, the culled chains, the ring-only calls — write no dB plane: a batch's rows go straight to the averager ring's
 * buffer, as dB values, after a fold in the fold's blocked order. sgf_create keeps the scan off those forms: it wants
 * SS_FLAG_SPECTROGRAM, which makes every batch keep its plane.
 *
 * An object made by sgf_create_ring is bound to the feed of a context WITHOUT SS_FLAG_SPECTROGRAM and forms the rows of a batch
 * from wherever the batch left its dB values: the plane if it kept one (learning frames, a feed created with want_psd, every
 * batch below 65536 points), the rows in the ring's buffer otherwise — in bin order by the kernel sgf_create's objects run, in the
 * fold's order by one that does the same arithmetic in the same order through the fold's addresses (csrc/spectrogram_rows_ring.h).
 * The two kinds of batch may follow each other in any order, and a row may span both. While such an object is bound, a batch of
 * 65536 points and up goes through the feed as ss_process_device makes its calls (no plane kept where the form keeps none) unless
 * the feed was created with want_psd — with or without a ring tracker (specscan_track_feed_ring.h) beside it.
 *
 * The row size is the rule SS_FLAG_SPECTROGRAM applies — min(getFft(sample_rate, 1000), 16384, fft_size), spectrogram.cpp:14 — and
 * sgf_result.size carries it; ss_spectrogram_size stays 0 on such a context, and the context keeps no accumulator of its own
 * (ss_spectrogram_read refuses). Everything else is specscan_spectrogram_feed.h's: sgf_config, sgf_result, sgf_rows, sgf_destroy and
 * sgf_last_error serve the object unchanged, SGF_ABI_VERSION is unchanged, and the rows are byte for byte what the reference's
 * Spectrogram + DataController publish for the dB values sgf_batch_db_rows hands out.
 */
#ifndef SPECSCAN_SPECTROGRAM_FEED_RING_H
#define SPECSCAN_SPECTROGRAM_FEED_RING_H

#include <stdint.h>

#include "specscan_spectrogram_feed.h"

#ifdef __cplusplus
extern "C" {
#endif

/* SS_ERR_INVALID with a message (sgf_last_error(NULL)): the scan context has SS_FLAG_SPECTROGRAM (use sgf_create); the feed has
 * batches pending or a slot acquired; the feed has a spectrogram object already; abi_version or max_rows is bad; fft_size is no
 * power-of-two multiple of the row size, or no multiple of 64. */
int sgf_create_ring(ss_feed* feed, const sgf_config* cfg, sgf_ctx** out);

/* The dB rows [frame0, frame0 + nframes) of the batch SUBMITTED last (not the one collected last), in bin order, nframes x fft_size
 * floats to host memory: from the dB plane if the batch kept one, else from the rows it left in the averager ring's buffer, with the
 * fold's order undone on the host, a row at a time (a reader for tests and debugging, not a data path: a feed with want_psd delivers
 * planes). Waits for the stream. These are the values the batch's spectrogram rows were formed from; it
 * serves every sgf_ctx. SS_ERR_INVALID (sgf_last_error(ctx)): no batch yet; the range is outside the batch; the rows are no longer
 * dB values (a retune or ss_reset_noise since the submit). ss_read_window(SS_PLANE_PSD) keeps refusing a batch that kept
 * no plane. */
int sgf_batch_db_rows(sgf_ctx* ctx, int32_t frame0, int32_t nframes, float* out);

#ifdef __cplusplus
}
#endif
#endif
