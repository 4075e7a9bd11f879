// spectrogram_rows_ring.h — the feed's spectrogram rows (spectrogram_rows.h) over a batch that kept no dB plane and left its rows in the
// averager ring's buffer in the radix-8 / radix-16 fold's blocked order (include/specscan_spectrogram_feed_ring.h; fft65536_dif8.h:
// dif_bin_offset). The arithmetic is spectrogram_rows.h's, operation for operation — +0.0f, the m input bins in ascending bin order, / m;
// sum += frame by frame; sum / (float)count and spec_rows_i8 at a cut (spec_rows_chain itself) — only the addressing differs.
//
// A block of 32 Q positions (Q = 1 << logq = 8 or 16: 1 KB or 2 KB) holds the contiguous bin run [32 Q b, 32 Q (b + 1)), bin Q k' + g of
// it at 32 g + k' % 32. A workgroup owns a column of whole blocks — one block (m <= 32 Q: 32 Q / m output bins) or the m / (32 Q) blocks
// of one output bin — from the batch's first frame to its last, as k_spec_rows owns its column: no atomics, no flags, no waits.
//
//   load    all 256 threads fetch a step of the column in 16-byte lanes, one step ahead (kSpecRowsStage floats, whole blocks, coalesced)
//           and store the lines into LDS as they are (ds_write_b128: no scatter, no pad)
//   walk    one thread per (frame, output bin) adds its run in ascending bin order; the permutation is in its read addresses
//           (spec_ring_pos). Lanes go over consecutive k' first, so with m <= Q — the reference's own ratios: m = 4 at 65536 points,
//           m = 8 at 131072 — the 32 lanes of a half wave read 32 consecutive words at every step of the run: no bank conflict
//           (ds_read_b32 banks are word % 32 per half wave). With m = c Q the lanes of a frame are c words apart and the frames'
//           images alias (32 Q words apart): a c-way conflict, up to 32-way at m = 32 Q where one thread walks a whole block. Those
//           are the ratios of a low sample rate under a long transform; the run is then the serial chain it is in k_spec_rows too.
//   chain   one thread per output bin adds the step's means in frame order (spec_rows_chain). Its lane number is the walking lane's
//           (spec_ring_lane_bin), so the means are read at consecutive words; with Q = 16 and m = 1 a block has 512 output bins
//           and a thread carries two chains.
//
// One form serves both radices and every power-of-two m from 1 to n / 64: logq and log2_m are launch arguments.
// The address functions are plain C++: tests/host/spectrogram_rows_ring_check.cpp walks them on the CPU, in this file's order.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#include "spectrogram_rows.h"
#define SS_SRR_HD __host__ __device__ __forceinline__
#else
#define SS_SRR_HD inline
#endif

namespace ss {

constexpr int kSpecRingStage = 4096;  // floats per workgroup and step (kSpecRowsStage): 256 threads x 4 loads x 16 bytes
constexpr int kSpecRingChains = 2;    // output-bin chains a thread carries at most (512 output bins of a radix-16 block at m = 1)

struct SpecRingGeom {
  int lm, logq;
  int lblock;  // log2 of a block's positions: 5 + logq
  int lrun;    // log2 of the values one (frame, output bin) item takes per step: min(lm, 12)
  int lwidth;  // log2 of the floats per frame and step: whole blocks, max(lrun, lblock)
  int lbins;   // log2 of the workgroup's output bins: lwidth - lrun
  int nseg;    // steps per run: m / 4096 beyond 4096 input bins per output bin, else 1
  int chunk;   // frames per step
  int lcol;    // log2 of the column's input bins: max(lm, lblock); grid = n >> lcol
};

SS_SRR_HD SpecRingGeom spec_ring_geom(int log2_m, int logq) {
  SpecRingGeom g{};
  g.lm = log2_m;
  g.logq = logq;
  g.lblock = 5 + logq;
  g.lrun = log2_m < 12 ? log2_m : 12;
  g.lwidth = g.lrun > g.lblock ? g.lrun : g.lblock;
  g.lbins = g.lwidth - g.lrun;
  g.nseg = 1 << (log2_m - g.lrun);
  g.chunk = kSpecRingStage >> g.lwidth;
  g.lcol = log2_m > g.lblock ? log2_m : g.lblock;
  return g;
}

// Where bin j of a run of whole blocks sits (dif_bin_offset, restated so that a host compiler can read this file): bin Q k' + g at
// (k' / 32) * 32 Q + 32 g + k' % 32. The next g of the same k' is 32 positions on.
SS_SRR_HD int spec_ring_pos(int j, int logq) {
  const int g = j & ((1 << logq) - 1), k = j >> logq;
  return ((k >> 5) << (5 + logq)) + (g << 5) + (k & 31);
}

// The output bin (within the workgroup's column) of walking lane `lane` in [0, 1 << lbins). With m < Q an output bin is a run of m
// residues g of ONE k': the lanes go over the block's 32 k' first, then over the Q / m runs of g. With m >= Q the output bins are
// runs of m / Q consecutive k' and the lanes take them in order.
SS_SRR_HD int spec_ring_lane_bin(const SpecRingGeom& g, int lane) {
  if (g.lm >= g.logq) return lane;
  return ((lane & 31) << (g.logq - g.lm)) | (lane >> 5);
}

#ifdef __HIPCC__

struct SpecRowsRingArgs {
  SpecRowsArgs r;  // psd: the batch's rows in the ring's buffer, [nframes][n] in the fold's order, 16-byte aligned; the rest as k_spec_rows takes it
  int logq;        // 3 or 4
};

// grid: n >> max(log2_m, 5 + logq) workgroups of 256 threads
__global__ __launch_bounds__(256) void k_spec_rows_ring(const SpecRowsRingArgs ra) {
#pragma clang fp contract(off)
  __shared__ float4 stage4[kSpecRingStage / 4];
  __shared__ float means[kSpecRingStage];
  __shared__ int cuts[kSpecRowsMaxCuts];
  __shared__ float sum0[kSpecRingChains * 256];
  const SpecRowsArgs& a = ra.r;
  const float* stage = reinterpret_cast<const float*>(stage4);
  const int tid = (int)threadIdx.x;
  if (tid < kSpecRowsMaxCuts) cuts[tid] = a.cut[tid];  // (read behind the first barrier of the loop)
  const SpecRingGeom g = spec_ring_geom(a.log2_m, ra.logq);
  const int nbins = 1 << g.lbins, run = 1 << g.lrun, nseg = g.nseg, chunk = g.chunk;
  const int nchunks = (a.nframes + chunk - 1) / chunk;
  const int steps = nchunks * nseg;
  const size_t col0 = (size_t)blockIdx.x << g.lcol;
  // an item's run: `inner` residues of one k' (m < Q), or `outer` k' with all Q residues each
  const int inner = g.lrun < g.logq ? run : 1 << g.logq, outer = run / inner;

  // (four named registers, not an array: frames past the batch's end fetch its last frame again and are not used)
  const auto load = [&](int step, int u) {
    const int f0 = (step / nseg) * chunk, seg = step % nseg;
    const int idx = u * 256 + tid, fr = idx >> (g.lwidth - 2), q = idx & ((1 << (g.lwidth - 2)) - 1);
    const int f = f0 + fr < a.nframes ? f0 + fr : a.nframes - 1;
    return *reinterpret_cast<const float4*>(a.psd + col0 + ((size_t)seg << g.lrun) + (size_t)f * (size_t)a.n + (size_t)(4 * q));
  };
  float4 r0, r1, r2, r3;
  const auto fetch = [&](int step) { r0 = load(step, 0), r1 = load(step, 1), r2 = load(step, 2), r3 = load(step, 3); };

  // (the container's sum through LDS, as in k_spec_rows: its load is waited for in front of the loop)
  // (two chains in scalars: lane tid, and lane tid + 256 where a block has 512 output bins)
  const bool chains0 = tid < nbins, chains1 = tid + 256 < nbins;
  const int bin0 = ((int)blockIdx.x << g.lbins) + spec_ring_lane_bin(g, chains0 ? tid : 0);
  const int bin1 = ((int)blockIdx.x << g.lbins) + spec_ring_lane_bin(g, chains1 ? tid + 256 : 0);
  if (chains0) sum0[tid] = a.sum[bin0];
  if (chains1) sum0[tid + 256] = a.sum[bin1];
  SpecRowsChain c0{0.0f, a.count0, 0, a.ncuts > 0 ? a.cut[0] : -1}, c1 = c0;
  float carry = 0.0f;
  fetch(0);
  for (int step = 0; step < steps; ++step) {
    const int f0 = (step / nseg) * chunk, seg = step % nseg;
    const int frames = a.nframes - f0 < chunk ? a.nframes - f0 : chunk;
    stage4[tid] = r0, stage4[256 + tid] = r1, stage4[512 + tid] = r2, stage4[768 + tid] = r3;  // frame fr of the step at fr << lwidth, as loaded
    if (step + 1 < steps) fetch(step + 1);
    __syncthreads();
    for (int item = tid; item < (frames << g.lbins); item += 256) {
      const int fr = item >> g.lbins, lane = item & (nbins - 1);
      const float* p = stage + (fr << g.lwidth);
      int j = spec_ring_lane_bin(g, lane) << g.lrun;  // the run's first bin, counted from the step's first
      float s = seg == 0 ? 0.0f : carry;
      for (int o = 0; o < outer; ++o, j += inner) {
        const float* q = p + spec_ring_pos(j, g.logq);
        for (int i = 0; i < inner; ++i) s += q[i << 5];
      }
      if (seg == nseg - 1) means[item] = s / (float)(1 << g.lm);
      else carry = s;  // (nseg > 1: one frame, one output bin, this thread)
    }
    __syncthreads();
    if (step == 0 && chains0) c0.sum = sum0[tid];
    if (step == 0 && chains1) c1.sum = sum0[tid + 256];
    if (seg == nseg - 1 && chains0) spec_rows_chain(a, c0, means + tid, cuts, nbins, f0, frames, bin0);
    if (seg == nseg - 1 && chains1) spec_rows_chain(a, c1, means + tid + 256, cuts, nbins, f0, frames, bin1);
    // (the next step's first barrier stands between these reads and the next means; its stage stores are behind the second one above)
  }
  if (chains0) a.sum[bin0] = c0.sum;
  if (chains1) a.sum[bin1] = c1.sum;
}

#endif  // __HIPCC__

}  // namespace ss
