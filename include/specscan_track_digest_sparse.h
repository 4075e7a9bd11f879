/*
 * specscan_track_digest_sparse.h — the tracking digest (specscan_track.h) on a scan context that keeps no planes, part of
 * libspecscan.so.
 *
 * st_create wants SS_FLAG_KEEP_PLANES: every batch then writes a full avg plane and no averaging tile is culled, and at 65536
 * points and up the context takes neither the int8 fold nor any call that writes no dB plane. The digest reads far less: cand_best
 * from the batch's rel rows, cand_avg from the cells the tiles with hits store into the batch's SPARSE avg plane whatever the
 * flags, and only the window peaks (peak_idx / peak_avg) read avg where no tile may have written it.
 *
 * An object made by st_create_sparse therefore re-evaluates, inside st_digest, exactly the 256-bin tile columns the watch windows
 * [key - group_size / 2, key + group_size / 2] touch — with the tile code of the scan, on the batch's own arguments, into the sparse
 * plane — and runs the same digest on that plane. The rel rows are read where the batch's call left them: the dB plane, or, after
 * a call that writes none (the radix-8 / radix-16 fold of int8 input, the culled chains of 65536 and 262144 points, the ring-only
 * calls of 2^20 points), the averager ring's buffer, as dB values and in the fold's order where that call's form says so. Every
 * number of st_result is defined by the context's own data: the rel rows of the batch and the ten before it, and the avg values
 * the scan's tile code gives on those rows. The scan's results, the form each call takes and the counters of ss_get_stats do not
 * change.
 *
 * Everything else is specscan_track.h's: st_config, st_result, st_digest, st_reset, st_destroy and st_last_error serve both kinds
 * of object, ST_ABI_VERSION is unchanged.
 *
 * Footprint on top of st_create's: 4 B x (N / 32) x max_batch of scratch mask words and 4 B x max_batch of scratch counts (the
 * replayed tiles' by-products), 4 B x N / 256 of column flags and one 8-byte counter. No plane is added.
 */
#ifndef SPECSCAN_TRACK_DIGEST_SPARSE_H
#define SPECSCAN_TRACK_DIGEST_SPARSE_H

#include <stdint.h>

#include "specscan_track.h"

#ifdef __cplusplus
extern "C" {
#endif

/* st_create for a scan context WITHOUT SS_FLAG_KEEP_PLANES: the fused back end (grouping 21 x 21), any fft_size. With
 * SS_FLAG_KEEP_PLANES it is simply st_create. SS_ERR_INVALID, with a message that names the reason (st_last_error(NULL)): the
 * unfused back end (any other grouping); SS_FLAG_REFERENCE_NAN (its NaN stage patches the planes behind the tiles); and
 * everything st_create refuses. */
int st_create_sparse(ss_ctx* scan, const st_config* cfg, st_ctx** out);

/* Cumulative since st_create_sparse / st_reset: the tiles the replay evaluated, and the tiles of the batches digested (frame
 * tiles x N / 256 columns each). Waits for the scan context's stream. SS_ERR_INVALID on an object made by st_create (also by
 * st_create_sparse on a context with SS_FLAG_KEEP_PLANES). */
int st_sparse_stats(st_ctx* ctx, uint64_t* tiles_evaluated, uint64_t* tiles_in_batches);

#ifdef __cplusplus
}
#endif
#endif
