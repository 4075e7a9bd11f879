// spectrogram_rows.h — the spectrogram rows of the pipelined feed (include/specscan_spectrogram_feed.h): Spectrogram::process and
// the arithmetic of Spectrogram::send (sources/radio/blocks/spectrogram.cpp:45-75) over one batch's dB plane, operation for operation
// and in the reference's order, so that a row's bytes do not depend on how the stream was cut into batches.
//
//   per frame and output bin   float s = +0.0f; s += the m input bins, ascending; s / m      (m == 1: the value itself)
//   per output bin             sum += that, frame by frame
//   at a closing frame         mean = sum / (float)count; row = int8(mean), truncated; sum = +0.0f; count = 0
//
// Which frames close a row is the host's decision (spectrogram_gate.h): the cut list comes by value. The only serial chain is the one
// per output bin, so one workgroup owns a column of output bins from the batch's first frame to its last — no atomics, no flags, no
// waits — and keeps the memory traffic off that chain: all 256 threads fetch a step of the column (kSpecRowsStage floats, four 16-byte
// loads per thread, issued one step ahead so that they are in flight while the chain runs), form the per-frame means into LDS, and
// then one thread per output bin adds the step's means in frame order.
//
//   m <= 4   a thread's 16 bytes hold 4 / m whole output bins: the means are formed in registers.
//   m > 4    the loaded floats are staged in LDS, every run of m (at most kSpecRowsRun) values behind one pad word, so that the
//            (frame, output bin) threads, whose runs begin m words apart, walk them in ascending order on different banks. Beyond
//            kSpecRowsRun input bins per output bin a run takes several steps, and the one walking thread carries its partial sum.
//
// The column is 64 input bins wide (m < 64) or one output bin (m >= 64): grid = n / 64 or n / m workgroups.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ss {

constexpr int kSpecRowsMaxCuts = 64;  // SGF_MAX_ROWS
constexpr int kSpecRowsStage = 4096;  // floats of the plane per workgroup and step: 256 threads x 4 loads x 16 bytes
constexpr int kSpecRowsRun = 4096;    // the longest run of input bins staged at once

struct SpecRowsArgs {
  const float* psd;  // [nframes][n] the batch's dB plane, 16-byte aligned
  float* sum;        // [size] the centre's container: read at the start, written at the end
  int8_t* rows;      // [ncuts][size]
  float* mean;       // [ncuts][size], or null
  int n, nframes, size;
  int log2_m;  // n == size << log2_m
  int count0;  // the container's counter in front of the batch
  int ncuts;
  int cut[kSpecRowsMaxCuts];  // closing frames, ascending
};

// float -> int8 as the host's conversion of ss_spectrogram_read gives it (truncation; the low byte of the 32-bit conversion, whose
// out-of-range result is 0x80000000)
__device__ __forceinline__ int8_t spec_rows_i8(float v) {
  const int i = fabsf(v) < 2147483648.0f ? (int)v : 0;
  return (int8_t)(i & 0xff);
}

struct SpecRowsChain {
  float sum;
  int count, k, next;
};

// One thread, one output bin: the step's means in frame order. The frames up to the next closing one are a plain run of adds whose
// LDS reads do not depend on the sum, so they stay in flight; the cut list is read from LDS (cuts), not from memory, so that nothing
// on the chain waits for the next step's loads.
__device__ __forceinline__ void spec_rows_chain(const SpecRowsArgs& a, SpecRowsChain& c, const float* means, const int* cuts, int pitch, int f0, int frames, int bin) {
#pragma clang fp contract(off)
  int fr = 0;
  while (fr < frames) {
    const bool closes = (unsigned)(c.next - f0) < (unsigned)frames;  // (cuts ascend: the next one is not behind fr)
    const int stop = closes ? c.next - f0 + 1 : frames;
    c.count += stop - fr;
#pragma unroll 8
    for (; fr < stop; ++fr) c.sum += means[fr * pitch];
    if (closes) {
      const float mean = c.sum / (float)c.count;
      const size_t at = (size_t)c.k * (size_t)a.size + (size_t)bin;
      a.rows[at] = spec_rows_i8(mean);
      if (a.mean) a.mean[at] = mean;
      c.sum = 0.0f;
      c.count = 0;
      ++c.k;
      c.next = c.k < a.ncuts ? cuts[c.k] : -1;
    }
  }
}

template <bool kStaged>
__global__ __launch_bounds__(256) void k_spec_rows(const SpecRowsArgs a) {
#pragma clang fp contract(off)
  __shared__ float means[kSpecRowsStage];
  __shared__ int cuts[kSpecRowsMaxCuts];
  const int tid = (int)threadIdx.x;
  __shared__ float sum0[64];
  if (tid < kSpecRowsMaxCuts) cuts[tid] = a.cut[tid];  // (read behind the first barrier of the loop)
  const int lm = a.log2_m;
  const int lrun = kStaged ? (lm < 12 ? lm : 12) : lm;      // log2 of the values one (frame, output bin) item takes per step
  const int lwidth = lrun > 6 ? lrun : 6;                   // log2 of the floats per frame and step
  const int bins = 1 << (lwidth - lrun);                    // output bins of this workgroup
  const int nseg = 1 << (lm - lrun);                        // steps per run
  const int chunk = kSpecRowsStage >> lwidth;               // frames per step
  const int nchunks = (a.nframes + chunk - 1) / chunk;
  const int steps = nchunks * nseg;
  const size_t col0 = (size_t)blockIdx.x << (lm > 6 ? lm : 6);

  float4 r[4];  // frames past the batch's end fetch its last frame again and are not used
  const auto fetch = [&](int step) {
    const int f0 = (step / nseg) * chunk, seg = step % nseg;
    const float* base = a.psd + col0 + ((size_t)seg << lrun);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = u * 256 + tid, fr = idx >> (lwidth - 2), q = idx & ((1 << (lwidth - 2)) - 1);
      const int f = f0 + fr < a.nframes ? f0 + fr : a.nframes - 1;
      r[u] = *reinterpret_cast<const float4*>(base + (size_t)f * (size_t)a.n + (size_t)(4 * q));
    }
  };

  // The container's sum goes through LDS: its load is then waited for here, in front of the loop, and not inside it, where the
  // wait would take the loads of the next step with it.
  const int bin = (int)blockIdx.x * bins + tid;
  const bool chains = tid < bins;
  if (chains) sum0[tid] = a.sum[bin];
  SpecRowsChain c{0.0f, a.count0, 0, a.ncuts > 0 ? a.cut[0] : -1};
  float carry = 0.0f;
  fetch(0);
  for (int step = 0; step < steps; ++step) {
    const int f0 = (step / nseg) * chunk, seg = step % nseg;
    const int frames = a.nframes - f0 < chunk ? a.nframes - f0 : chunk;
    if constexpr (!kStaged) {
      // lwidth == 6: 16 threads per frame, bins == 64 >> lm
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int idx = u * 256 + tid, fr = idx >> 4, q = idx & 15;
        if (fr >= frames) continue;
        const float4 v = r[u];
        if (lm == 0) {
          float* d = means + fr * 64 + 4 * q;
          d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
        } else if (lm == 1) {
          float s0 = 0.0f, s1 = 0.0f;
          s0 += v.x, s0 += v.y, s1 += v.z, s1 += v.w;
          means[fr * 32 + 2 * q] = s0 / 2.0f;
          means[fr * 32 + 2 * q + 1] = s1 / 2.0f;
        } else {
          float s = 0.0f;
          s += v.x, s += v.y, s += v.z, s += v.w;
          means[fr * 16 + q] = s / 4.0f;
        }
      }
      if (step + 1 < steps) fetch(step + 1);
      __syncthreads();
    } else {
      __shared__ float stage[kSpecRowsStage + kSpecRowsStage / 8];  // runs of >= 8 values, one pad word each
      const int run = 1 << lrun;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int idx = u * 256 + tid, fr = idx >> (lwidth - 2), q = idx & ((1 << (lwidth - 2)) - 1);
        if (fr >= frames) continue;
        const int i = 4 * q, item = fr * bins + (i >> lrun);
        float* d = stage + item * (run + 1) + (i & (run - 1));
        d[0] = r[u].x, d[1] = r[u].y, d[2] = r[u].z, d[3] = r[u].w;
      }
      if (step + 1 < steps) fetch(step + 1);
      __syncthreads();
      for (int item = tid; item < frames * bins; item += 256) {
        const float* p = stage + item * (run + 1);
        float s = seg == 0 ? 0.0f : carry;
        for (int j = 0; j < run; ++j) s += p[j];
        if (seg == nseg - 1) means[item] = s / (float)(1 << lm);
        else carry = s;  // (nseg > 1: one frame, one output bin, this thread)
      }
      __syncthreads();
    }
    if (step == 0 && chains) c.sum = sum0[tid];
    if (seg == nseg - 1 && chains) spec_rows_chain(a, c, means + tid, cuts, bins, f0, frames, bin);
    if constexpr (!kStaged) __syncthreads();  // (staged: the next step's barrier stands between this read and the next means)
  }
  if (chains) a.sum[bin] = c.sum;
}

}  // namespace ss
