/*
 * specscan_channelizer.h — C ABI of the recorder channeliser, part of libspecscan.so.
 *
 * The reference records every detected transmission with a per-slot GNU Radio chain
 * (Recorder, sources/radio/recorder.cpp:14-46; `recordersCount` slots per device, sources/radio/sdr_device.cpp:39-41):
 *
 *   source -> Blocker(drop while idle) -> rotator_cc(-2*pi*shift/fs) -> rational_resampler<cc>(f1, f2) x stages
 *          -> complex_to_interleaved_char(vector, 127.0) -> stream_to_vector -> Buffer -> DataController::pushTransmission
 *
 * with the stage factors from getResamplersFactors(fs, recording bandwidth, RESAMPLER_THRESHOLD = 125)
 * (sources/utils/radio_utils.cpp:128-152, sources/config.h:20) and GNU Radio's default resampler taps.
 * One sc_ctx replaces the rotator -> resamplers -> int8 conversion of ALL slots of one device: every call takes
 * the device's IQ stream once and produces, per recording slot, the int8 samples the reference hands to its Buffer.
 * Slot bookkeeping (which shift is recorded where, flush intervals, MQTT framing) stays on the host
 * (sdr_device.cpp:82-144, recorder.cpp:58-98, network/data_controller.cpp:27-42).
 *
 * State carried between calls, exactly as the reference's blocks carry it: per slot the rotator phase and every
 * resampler's history and polyphase counter; an idle slot sees no samples (Blocker drops them) and keeps its state.
 * No CPU fallback: without a GPU sc_create fails.
 */
#ifndef SPECSCAN_CHANNELIZER_H
#define SPECSCAN_CHANNELIZER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SC_ABI_VERSION 1u
#define SC_MAX_CHANNELS 16
#define SC_MAX_STAGES 8

typedef struct sc_ctx sc_ctx;

typedef struct sc_config {
  uint32_t abi_version; /* SC_ABI_VERSION */
  int32_t sample_rate;  /* Recorder::m_sampleRate (recorder.cpp:16) */
  int32_t bandwidth;    /* Config::recordingBandwidth(): recording.min_sample_rate (config.cpp:79,140) */
  int32_t threshold;    /* RESAMPLER_THRESHOLD (config.h:20) */
  int32_t channels;     /* recordersCount (sdr_device.cpp:39): 1..SC_MAX_CHANNELS */
  int32_t max_samples;  /* largest nsamples of one call */
  float pack_scale;     /* complex_to_interleaved_char scale, 127.0 (recorder.cpp:36) */
  int32_t device_id;
} sc_config;

/* status codes are the ss_status values of specscan.h (0 = ok, < 0 = error) */
void sc_default_config(sc_config* cfg, int32_t sample_rate, int32_t bandwidth);
int sc_create(const sc_config* cfg, sc_ctx** out);
void sc_destroy(sc_ctx* ctx);
const char* sc_last_error(const sc_ctx* ctx); /* ctx may be NULL: last sc_create failure of this thread */

/* The resampler cascade this context runs (getResamplersFactors + rational_resampler's default taps). */
int sc_stage_count(const sc_ctx* ctx);
int sc_stage_info(const sc_ctx* ctx, int32_t stage, int32_t* interpolation, int32_t* decimation, int32_t* ntaps);
int sc_stage_taps(const sc_ctx* ctx, int32_t stage, float* taps /* ntaps */);
/* Upper bound of output samples per channel for a call of nsamples input samples. */
int32_t sc_output_capacity(const sc_ctx* ctx, int32_t nsamples);

/* Recorder::startRecording (recorder.cpp:58-73): rotator increment 2*pi*(-shift/fs), slot unblocked. Phase and filter
 * histories are NOT reset, as in the reference. Recorder::stopRecording (:75-87): slot blocked. */
int sc_start(sc_ctx* ctx, int32_t channel, int32_t shift_hz);
int sc_stop(sc_ctx* ctx, int32_t channel);
int sc_is_recording(const sc_ctx* ctx, int32_t channel);

/* Sample format of the stream sc_process / sc_process_device read from the next call on: an ss_format
 * (SS_FMT_CF32, SS_FMT_CS8, SS_FMT_CU8, SS_FMT_CS16) with ss_config.int_scale's meaning and defaults
 * (0 -> 1/128, 1/127.5, 1/32768). Phase and filter histories are kept (they hold converted, rotated floats).
 * A context starts in CF32. SS_ERR_INVALID for an unknown format or an int_scale that is negative or not finite.
 * The integers convert exactly as in the scan chain: cf32 = (int - offset) * int_scale. */
int sc_set_input_format(sc_ctx* ctx, int32_t in_format, float int_scale);

/* One work() pass over nsamples samples of the device stream, interleaved re,im in the context's input format
 * (sc_set_input_format; CF32 unless set): SS_FMT_BYTES(format) * nsamples bytes.
 *   out_i8   [channels][cap][2] int8 (re,im) — what complex_to_interleaved_char emits;   nullable
 *   out_cf32 [channels][cap][2] float — the last resampler's output (DEBUG_SAVE_RECORDING_RAW_IQ tap, recorder.cpp:42-45); nullable
 *   counts   [channels] samples produced per channel (0 for idle slots)
 * sc_process takes host pointers and is synchronous; sc_process_device takes device pointers, is asynchronous on the
 * context's stream (sc_sync), and returns counts (host array) immediately — they do not depend on the data.
 * sc_process_device refuses (SS_ERR_INVALID) an integer-format d_iq that is not aligned to the sample size. It only reads
 * d_iq, as ss_process_device does: one device upload of the receiver's native stream, nframes items of N*D samples in
 * the same format, may feed both ss_process_device and sc_process_device (nframes * N * D samples) at once. */
int sc_process(sc_ctx* ctx, const void* iq, int32_t nsamples, int8_t* out_i8, float* out_cf32, int32_t* counts, int32_t cap);
int sc_process_device(sc_ctx* ctx, const void* d_iq, int32_t nsamples, int8_t* d_out_i8, float* d_out_cf32, int32_t* counts, int32_t cap);
int sc_sync(sc_ctx* ctx);

/* Per-slot sample ranges in one call: recordings that begin, end and retune inside the stream of one call, at sample
 * resolution, without sc_start / sc_stop between calls. */
#define SC_MAX_RANGES 64
typedef struct sc_range {
  int32_t channel;    /* 0 .. channels-1 */
  int32_t shift_hz;   /* as sc_start */
  int32_t begin, end; /* samples of THIS call's stream: [begin, end), 0 <= begin <= end <= nsamples */
} sc_range;

/* Defined by the entry points above: for every channel, its ranges in the order given, and for each of them
 * sc_start(channel, shift_hz), a sc_process* of samples [begin, end) with only that channel unblocked, sc_stop(channel).
 * A channel's outputs are concatenated from element 0 of its plane ([channels][cap] as above); nothing is written at or
 * beyond cap, though the state advances past it. counts[channel] is the channel's true total, range_counts[i] the outputs
 * of ranges[i] (nullable); both are host arrays, do not depend on the data, and the device form returns them at once.
 * Phase, filter histories and polyphase counters carry across a channel's ranges and across calls as they carry across a
 * stop / restart; what lies between two ranges is dropped, as the Blocker drops it. Every range is bit-identical to its
 * step of that sequence run through sc_process_device on d_iq + begin.
 *   - ranges of one channel ascend and do not overlap (end_i <= begin_{i+1}); channels may interleave in any order
 *   - begin == end is a no-op with range_counts[i] = 0
 *   - nranges > SC_MAX_RANGES, a bad channel, begin > end or end > nsamples: SS_ERR_INVALID
 *   - the two ways of driving a context are not mixed: refused (SS_ERR_INVALID) while any channel sc_is_recording; on
 *     return no channel is recording
 *   - the device form keeps sc_process_device's alignment rule for d_iq
 *   - sc_output_capacity(ctx, nsamples) is a valid cap: a channel's total depends only on how many samples it saw
 * Everything is validated before the first launch: a refused call changes nothing. */
int sc_process_ranges(sc_ctx* ctx, const void* iq, int32_t nsamples, const sc_range* ranges, int32_t nranges, int8_t* out_i8, float* out_cf32,
                      int32_t* counts, int32_t* range_counts, int32_t cap);
int sc_process_ranges_device(sc_ctx* ctx, const void* d_iq, int32_t nsamples, const sc_range* ranges, int32_t nranges, int8_t* d_out_i8,
                             float* d_out_cf32, int32_t* counts, int32_t* range_counts, int32_t cap);

/* sc_process_ranges_device on a stream that is still in host memory, uploading only what the ranges read: the union of the
 * non-empty ranges, merged into intervals, one copy per interval to the same offsets of the context's own input buffer
 * (max_samples samples, allocated by the first host-form call). Definition, rules, outputs (device planes) and counts are
 * sc_process_ranges_device's; the call is asynchronous on the context's stream, and iq must stay valid and unchanged until
 * sc_sync has returned. Pinned memory makes the copies truly asynchronous; pageable memory works. *uploaded_bytes (nullable)
 * is the bytes copied for this call: bytes per sample times the size of the union. Everything is validated before the first
 * copy: a refused call changes nothing, *uploaded_bytes included. */
int sc_process_ranges_upload(sc_ctx* ctx, const void* iq, int32_t nsamples, const sc_range* ranges, int32_t nranges, int8_t* d_out_i8,
                             float* d_out_cf32, int32_t* counts, int32_t* range_counts, int32_t cap, uint64_t* uploaded_bytes);

/* DataController::pushTransmission payload (data_controller.cpp:27-42): uint64 time ms, int32 start, int32 stop,
 * uint32 sample rate, then the samples as offset-binary bytes (int8 ^ 0x80). Host-side helper; returns the byte count
 * (out may be NULL to query it), or < 0 if cap is too small. */
int sc_transmission_payload(uint64_t time_ms, int32_t frequency, int32_t sample_rate, const int8_t* iq_i8, int32_t nsamples, uint8_t* out,
                            int32_t cap);

#ifdef __cplusplus
}
#endif
#endif /* SPECSCAN_CHANNELIZER_H */
