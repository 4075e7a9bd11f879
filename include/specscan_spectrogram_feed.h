/*
 * specscan_spectrogram_feed.h — C ABI of the spectrogram rows delivered through the pipelined feed, part of libspecscan.so.
 *
 * The reference's Spectrogram block (sources/radio/blocks/spectrogram.cpp:29-75) looks at its send gate after EVERY frame: a row
 * closes at the first frame whose clock is more than 1000 ms past the last send, is stamped with that frame's time, holds the mean
 * over the frames since the last send, and the container starts again. An sgf_ctx bound to an ss_feed reproduces exactly that
 * behind every submitted batch: the frame times of a batch are known at ss_feed_submit, so which frames close a row is decided
 * on the host (sgf_gate_plan), and one kernel behind the batch's chain does the reference's arithmetic in the reference's order
 * on the batch's dB plane (csrc/spectrogram_rows.h). The rows are therefore independent of how the stream was cut into batches,
 * and — given the engine's dB plane — byte-identical to what the reference's Spectrogram + DataController publish.
 *
 * State is per centre frequency, as the reference's m_containers: a float sum row on the device, the counter and the gate on the
 * host. A batch runs at the centre in force at its submit; ss_set_frequency_range between submits switches containers and the
 * old one keeps sum, counter and gate until its centre returns. ss_reset does not touch the containers. The scan context's own
 * accumulator (ss_spectrogram_read) goes on as before: the rows have sums of their own.
 *
 * While an sgf_ctx is bound, ss_feed_submit needs t_ms: a submit with t_ms == NULL, or whose clock would close more than
 * max_rows rows, is refused with SS_ERR_INVALID before anything is enqueued — the slot stays acquired, no state changes.
 *
 * Threads: as the feed's. The scan context must outlive the sgf_ctx. ss_feed_destroy before sgf_destroy is allowed: the sgf_ctx
 * then only accepts sgf_destroy and sgf_last_error.
 */
#ifndef SPECSCAN_SPECTROGRAM_FEED_H
#define SPECSCAN_SPECTROGRAM_FEED_H

#include <stdint.h>

#include "specscan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGF_ABI_VERSION 1u
#define SGF_MAX_ROWS 64

typedef struct sgf_ctx sgf_ctx;

typedef struct sgf_config {
  uint32_t abi_version; /* SGF_ABI_VERSION */
  int32_t max_rows;     /* rows one batch may close, 1..SGF_MAX_ROWS (8 fits 1024 frames of 8192 points at 2.048 MS/s twice) */
  int32_t want_mean;    /* also deliver the float means */
} sgf_config;

/* The rows of one batch. Pointers: the slot's pinned memory, valid until the slot is acquired again. */
typedef struct sgf_result {
  int32_t nrows, size;            /* rows closed inside that batch (0 is normal); ss_spectrogram_size */
  int32_t frequency, sample_rate; /* centre at submit time: pushSpectrogram's arguments */
  int32_t open_count;             /* frames accumulated for this centre and not yet sent */
  const int64_t* time_ms;         /* [nrows] t_ms of the closing frame */
  const int32_t* frame;           /* [nrows] its index in the batch */
  const int32_t* count;           /* [nrows] m_counter at the send */
  const int8_t* rows;             /* [nrows][size] int8(sum / count), converted as ss_spectrogram_read converts */
  const float* mean;              /* [nrows][size] the float before conversion; NULL unless want_mean */
} sgf_result;

/* SS_ERR_INVALID with a message (sgf_last_error(NULL)): the scan context lacks SS_FLAG_SPECTROGRAM (the flag fixes the row size
 * and guarantees every batch a dB plane); the feed has batches pending or a slot acquired; the feed has a spectrogram object
 * already; abi_version or max_rows is bad. */
int sgf_create(ss_feed* feed, const sgf_config* cfg, sgf_ctx** out);
void sgf_destroy(sgf_ctx* ctx);
const char* sgf_last_error(const sgf_ctx* ctx); /* NULL: the last sgf_create failure of this thread */

/* The rows of the batch collected last — after ss_feed_collect or stf_collect, also while the recorder holds the slot. */
int sgf_rows(sgf_ctx* ctx, sgf_result* out);

/* Host only, no GPU: the reference's gate for ONE centre frequency's container over one batch. The container's first frame
 * stamps *last_send (*have_last 0 -> 1); a row closes at frame f iff *last_send + 1000 < t_ms[f], strictly, and then
 * *last_send = t_ms[f]. Nothing assumes a monotonic clock. Returns the number of rows closed and writes the first
 * min(that, cap) closing frames to cut_frame. */
int32_t sgf_gate_plan(int64_t* last_send, int32_t* have_last, const int64_t* t_ms, int32_t nframes, int32_t* cut_frame, int32_t cap);

#ifdef __cplusplus
}
#endif
#endif
