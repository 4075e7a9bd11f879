/*
 * specscan_track_sparse.h — the tracked feed (specscan_track_feed.h) on a scan context that keeps no planes, part of libspecscan.so.
 *
 * stf_create wants SS_FLAG_KEEP_PLANES: every batch then writes a full avg plane (4 B per sample) and no averaging tile is culled.
 * The digest reads far less. cand_best is rebuilt from the dB plane, which a detect-mode batch leaves anyway; cand_avg is avg at
 * the candidates, cells the tiles with hits store into the batch's SPARSE avg plane whatever the flags; only the window peaks
 * (peak_idx / peak_avg: the maximum of avg around every watch key in every frame) read avg where no tile may have written it.
 *
 * An object made by stf_create_sparse therefore re-evaluates, behind the batch's chain and on the context's stream, exactly the
 * 256-bin tile columns the watch windows [key - group_size / 2, key + group_size / 2] touch — with the tile code of the scan, on
 * the batch's own arguments, into the sparse plane — and runs the same digest on that plane. Every number of stf_result is the one
 * a context with SS_FLAG_KEEP_PLANES gives, bit for bit; the scan stays on its culled path, writes no avg plane, and its
 * ss_get_stats counters do not move for the replay. At the reference's recording bandwidths a window spans one or two of the 32
 * columns of an 8192-point row.
 *
 * Everything else is specscan_track_feed.h's: stf_config, stf_result, stf_collect, stf_post_keys, stf_reset, stf_destroy and
 * stf_last_error serve both kinds of object, STF_ABI_VERSION is unchanged.
 *
 * Footprint on top of stf_create's: 4 B x (N / 32) x max_batch of scratch mask words and 4 B x max_batch of scratch counts (the
 * replayed tiles' by-products: the scan's own mask buffers must stay all zero between uses), 4 B x N / 256 of column flags and one
 * 8-byte counter. No plane is added.
 */
#ifndef SPECSCAN_TRACK_SPARSE_H
#define SPECSCAN_TRACK_SPARSE_H

#include <stdint.h>

#include "specscan_track_feed.h"

#ifdef __cplusplus
extern "C" {
#endif

/* stf_create for a scan context WITHOUT SS_FLAG_KEEP_PLANES: the fused back end (grouping 21 x 21), fft_size <= 32768;
 * SS_FLAG_NO_CULL, SS_FLAG_STREAM_ORDERED and SS_FLAG_SPECTROGRAM contexts are accepted. With SS_FLAG_KEEP_PLANES it is simply
 * stf_create. SS_ERR_INVALID, with a message that names the reason (stf_last_error(NULL)): the unfused back end (any other
 * grouping); SS_FLAG_REFERENCE_NAN (its NaN stage patches the planes behind the tiles); fft_size >= 65536 (a detect-mode call
 * there can leave no bin-ordered dB plane at all); and everything stf_create refuses. */
int stf_create_sparse(ss_feed* feed, const stf_config* cfg, stf_ctx** out);

/* Cumulative since stf_create_sparse / stf_reset: the tiles the replay evaluated, and the tiles of the batches it ran behind
 * (frame tiles x N / 256 columns each). Waits for the scan context's stream. SS_ERR_INVALID on an object made by stf_create
 * (also by stf_create_sparse on a context with SS_FLAG_KEEP_PLANES). */
int stf_sparse_stats(stf_ctx* ctx, uint64_t* tiles_evaluated, uint64_t* tiles_in_batches);

#ifdef __cplusplus
}
#endif
#endif
