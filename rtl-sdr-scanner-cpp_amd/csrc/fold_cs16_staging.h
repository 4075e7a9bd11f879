// fold_cs16_staging.h — how a frame of four-byte samples (CS16) reaches the threads of the radix-8 / radix-16 fold (fft65536_dif8.h):
// which bytes of the frame every LDS-DMA instruction fetches, where they land, which word a thread reads, and the order of issues,
// waits and reads. Plain functions of integers, host and device: the fold's kernels call them, and tests/host/fold_cs16_staging_check.cpp
// walks the same functions over a model frame and a model LDS array on the CPU (no HIP include here: g++ compiles it).
//
// The frame goes through the two 16 KiB halves of the exchange plane in PIECES of 16 KiB, as the two-byte formats' does — half as many
// samples a piece: eight SLOTS of 512 samples (2 KiB), one per wave, each fetched by two wave-instructions of 64 lanes x 16 bytes.
//   radix 8  (65536 points):  sixteen pieces; piece p is run rho = p of every q: slot s holds q = s.
//   radix 16 (131072 points): thirty-two pieces; piece p is run rho = p / 2 of the four pairs (q, q + 8), q = 4 (p % 2) + i: slot i holds
//                             q, slot 4 + i holds q + 8 — what one pair sum s_q needs is in one piece, and the four sums of the first piece
//                             of a run wait in registers for the second.
// Thread t's sample of slot s is m = t + 512 rho + 8192 q: word 512 s + t of the piece.
// The order (Q = 8 or 16, P = pieces): pieces 0 and 1 are issued up front; then for p = 0 .. P - 1: every wave waits for its own fetches
// (vmcnt 0), barrier, piece issue_behind_barrier(p) is issued — into the half whose piece p - 1 every wave has read, having passed the
// barrier —, piece p is read from half p % 2.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define SS_FCS_HD __host__ __device__ __forceinline__
#else
#define SS_FCS_HD inline
#endif

namespace ss {

constexpr int kFoldCs16PieceBytes = 16384;  // = one half of the exchange plane
constexpr int kFoldCs16LaneBytes = 16;      // one lane of an LDS-DMA wave-instruction
constexpr int kFoldCs16Waves = 8, kFoldCs16FetchesPerWave = 2;

template <int Q>
struct FoldCs16Stage {
  static_assert(Q == 8 || Q == 16, "the folds that exist");
  static constexpr int kPieces = Q == 8 ? 16 : 32;
  static constexpr int kFrameBytes = 8192 * Q * 4;
  // the run and the q of piece p's slot `slot` (< 8)
  static SS_FCS_HD constexpr int rho(int p) { return Q == 8 ? p : p >> 1; }
  static SS_FCS_HD constexpr int q(int p, int slot) { return Q == 8 ? slot : 4 * (p & 1) + (slot & 3) + 8 * (slot >> 2); }
  static SS_FCS_HD constexpr int half(int p) { return p & 1; }
  // the j-th (< 2) wave-instruction of wave w (< 8, which fetches slot w) for piece p: the first byte it fetches, counted from the
  // frame's first, and the first byte it writes, counted from the plane's first; lane l adds lane_bytes(l) to both
  static SS_FCS_HD constexpr uint32_t src_wave(int p, int w, int j) { return 4u * (uint32_t)(512 * rho(p) + 8192 * q(p, w)) + 1024u * (uint32_t)j; }
  static SS_FCS_HD constexpr uint32_t dst_wave(int p, int w, int j) { return (uint32_t)(half(p) * kFoldCs16PieceBytes + w * 2048 + j * 1024); }
  static SS_FCS_HD constexpr uint32_t lane_bytes(int lane) { return (uint32_t)(kFoldCs16LaneBytes * lane); }
  // the 32-bit word of the plane that holds thread t's sample of piece p's slot `slot`
  static SS_FCS_HD constexpr uint32_t read_word(int p, int slot, int t) { return (uint32_t)(half(p) * (kFoldCs16PieceBytes / 4) + 512 * slot + t); }
  // the piece issued behind the barrier in front of piece p's reads, or -1 (pieces 0 and 1 are issued before the loop)
  static SS_FCS_HD constexpr int issue_behind_barrier(int p) { return (p >= 1 && p + 1 < kPieces) ? p + 1 : -1; }
};

}  // namespace ss
