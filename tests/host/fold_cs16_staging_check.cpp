// fold_cs16_staging_check.cpp — the staging of four-byte samples in the radix-8 / radix-16 fold (csrc/fold_cs16_staging.h), walked on the
// CPU with the functions the kernels call (fft65536_dif8.h: dif8_front2_bfly / dif16_front2_bfly, FMT_CS16), as a stand-alone program under
// the address and undefined-behaviour sanitizers. A model frame holds the value m at sample m (one 32-bit word a sample), a model LDS
// array stands for the exchange plane's two halves. For Q = 8 and Q = 16:
//   every sample of the frame is fetched exactly once;
//   no fetch leaves the frame's N * 4 bytes or its piece's half of the plane, no read leaves its piece's half;
//   thread t's read for (rho, q) yields sample t + 512 rho + 8192 q, and the reads of a run cover every q once, pairs (q, q + Q / 2) in one piece;
//   a piece's place is not refetched before its last read, and not read before its fetch is waited for: the kernel's order of issues,
//   waits, barriers and reads, written out as a list of events and replayed with every wave at its own pace between the barriers.
// The last line is "all ok" or the count of failures.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../rtl-sdr-scanner-cpp_amd/csrc/fold_cs16_staging.h"

namespace {

long g_bad = 0;
#define EXPECT(cond, ...)                       \
  do {                                          \
    if (!(cond) && ++g_bad <= 20) {             \
      printf("FAIL %s: ", #cond);               \
      printf(__VA_ARGS__);                      \
      printf("\n");                             \
    }                                           \
  } while (0)

constexpr int kThreads = 512, kLanes = 64;
constexpr uint32_t kPoison = 0xffffffffu;

enum Kind { ISSUE, WAIT, BARRIER, READ };
struct Event {
  Kind kind;
  int piece;  // ISSUE, READ
};

// The order every wave of the workgroup runs through (fft65536_dif8.h, the CS16 branches): pieces 0 and 1 up front, then per piece
// wait (vmcnt 0: the wave's own fetches) - barrier - the next issue - the reads.
template <int Q>
std::vector<Event> kernel_order() {
  using S = ss::FoldCs16Stage<Q>;
  std::vector<Event> ev;
  ev.push_back({ISSUE, 0});
  ev.push_back({ISSUE, 1});
  for (int p = 0; p < S::kPieces; ++p) {
    ev.push_back({WAIT, -1});
    ev.push_back({BARRIER, -1});
    if (S::issue_behind_barrier(p) >= 0) ev.push_back({ISSUE, S::issue_behind_barrier(p)});
    ev.push_back({READ, p});
  }
  ev.push_back({BARRIER, -1});  // the plane goes back to the transform
  return ev;
}

template <int Q>
struct Model {
  using S = ss::FoldCs16Stage<Q>;
  static constexpr int N = 8192 * Q;
  std::vector<uint32_t> frame = std::vector<uint32_t>(N);          // sample m holds m
  std::vector<uint32_t> lds = std::vector<uint32_t>(2 * ss::kFoldCs16PieceBytes / 4, kPoison);
  std::vector<int> fetched = std::vector<int>(N, 0);               // times sample m was fetched
  std::vector<int> word_piece = std::vector<int>(lds.size(), -1);  // the piece whose fetch wrote the word last (landed or not)
  std::vector<char> landed = std::vector<char>(lds.size(), 0);     // ... and whether that fetch has been waited for by its wave
  std::vector<char> visible = std::vector<char>(lds.size(), 0);    // ... and whether every wave had done so when the last barrier was passed
  std::vector<int> reads_left = std::vector<int>(S::kPieces, 0);   // reads of piece p still to come (all waves)
  std::vector<int> seen = std::vector<int>(N, 0);                  // times sample m reached its thread
  struct InFlight {
    uint32_t first_word;
  };
  std::vector<std::vector<InFlight>> in_flight = std::vector<std::vector<InFlight>>(ss::kFoldCs16Waves);

  Model() {
    for (int m = 0; m < N; ++m) frame[(size_t)m] = (uint32_t)m;
    for (int p = 0; p < S::kPieces; ++p) reads_left[(size_t)p] = kThreads * 8;
  }

  void issue(int w, int p) {
    for (int j = 0; j < ss::kFoldCs16FetchesPerWave; ++j)
      for (int lane = 0; lane < kLanes; ++lane) {
        const uint32_t src = S::src_wave(p, w, j) + S::lane_bytes(lane), dst = S::dst_wave(p, w, j) + S::lane_bytes(lane);
        EXPECT(src % 4 == 0 && src + ss::kFoldCs16LaneBytes <= (uint32_t)S::kFrameBytes, "Q %d piece %d wave %d fetch %d lane %d: source byte %u", Q, p, w, j, lane, src);
        const uint32_t lo = (uint32_t)(S::half(p) * ss::kFoldCs16PieceBytes);
        EXPECT(dst % 4 == 0 && dst >= lo && dst + ss::kFoldCs16LaneBytes <= lo + ss::kFoldCs16PieceBytes, "Q %d piece %d wave %d fetch %d lane %d: LDS byte %u", Q, p, w, j, lane, dst);
        if (src + ss::kFoldCs16LaneBytes > (uint32_t)S::kFrameBytes || dst + ss::kFoldCs16LaneBytes > lds.size() * 4) continue;
        for (uint32_t k = 0; k < ss::kFoldCs16LaneBytes / 4; ++k) {
          const uint32_t word = dst / 4 + k;
          // the place must be free: whatever piece it held has been read by everybody
          const int old = word_piece[word];
          EXPECT(old < 0 || reads_left[(size_t)old] == 0, "Q %d piece %d overwrites word %u of piece %d, %d reads of which are still to come", Q, p, word, old, old < 0 ? 0 : reads_left[(size_t)old]);
          lds[word] = frame[src / 4 + k];
          word_piece[word] = p;
          landed[word] = visible[word] = 0;
          ++fetched[src / 4 + k];
        }
        in_flight[(size_t)w].push_back({dst / 4});
      }
  }
  void wait(int w) {  // vmcnt(0): everything this wave has issued has landed
    for (const InFlight& f : in_flight[(size_t)w])
      for (uint32_t k = 0; k < ss::kFoldCs16LaneBytes / 4; ++k) landed[f.first_word + k] = 1;
    in_flight[(size_t)w].clear();
  }
  void barrier() { visible = landed; }  // what has landed by now is visible to every wave behind it; what is still in flight is not
  void read(int w, int p) {
    for (int t = 64 * w; t < 64 * w + 64; ++t)
      for (int slot = 0; slot < 8; ++slot) {
        const uint32_t word = S::read_word(p, slot, t);
        const uint32_t lo = (uint32_t)(S::half(p) * ss::kFoldCs16PieceBytes / 4);
        EXPECT(word >= lo && word < lo + ss::kFoldCs16PieceBytes / 4, "Q %d piece %d slot %d thread %d: word %u", Q, p, slot, t, word);
        if (word >= lds.size()) continue;
        const int rho = S::rho(p), q = S::q(p, slot);
        EXPECT(rho >= 0 && rho < 16 && q >= 0 && q < Q, "Q %d piece %d slot %d: run %d q %d", Q, p, slot, rho, q);
        const uint32_t want = (uint32_t)(t + 512 * rho + 8192 * q);
        EXPECT(word_piece[word] == p && visible[word], "Q %d piece %d slot %d thread %d reads word %u, which holds piece %d (%s)", Q, p, slot, t, word, word_piece[word],
               visible[word] ? "visible" : "not waited for behind a barrier");
        EXPECT(lds[word] == want, "Q %d piece %d slot %d thread %d: sample %u, wanted %u", Q, p, slot, t, lds[word], want);
        if (want < (uint32_t)N) ++seen[want];
        --reads_left[(size_t)p];
      }
  }
};

// Replays the order with the eight waves at their own pace: between two barriers the waves run their events in an order drawn from `rng`
// (seed 0: wave by wave). What a read may rely on is what every wave had waited for when the barrier before it was passed.
template <int Q>
void run(unsigned seed) {
  using S = ss::FoldCs16Stage<Q>;
  const std::vector<Event> order = kernel_order<Q>();
  Model<Q> m;
  std::mt19937 rng(seed);
  size_t at = 0;
  while (at < order.size()) {
    size_t end = at;
    while (end < order.size() && order[end].kind != BARRIER) ++end;  // the span [at, end) runs between two barriers
    std::vector<size_t> pos((size_t)ss::kFoldCs16Waves, at);
    for (;;) {
      std::vector<int> ready;
      for (int w = 0; w < ss::kFoldCs16Waves; ++w)
        if (pos[(size_t)w] < end) ready.push_back(w);
      if (ready.empty()) break;
      const int w = seed == 0 ? ready.front() : ready[rng() % ready.size()];
      const Event& e = order[pos[(size_t)w]++];
      if (e.kind == ISSUE) m.issue(w, e.piece);
      else if (e.kind == WAIT) m.wait(w);
      else m.read(w, e.piece);
    }
    m.barrier();
    at = end + 1;
  }
  for (int i = 0; i < Model<Q>::N; ++i) {
    EXPECT(m.fetched[(size_t)i] == 1, "Q %d seed %u: sample %d fetched %d times", Q, seed, i, m.fetched[(size_t)i]);
    EXPECT(m.seen[(size_t)i] == 1, "Q %d seed %u: sample %d read %d times", Q, seed, i, m.seen[(size_t)i]);
  }
  for (int p = 0; p < S::kPieces; ++p) EXPECT(m.reads_left[(size_t)p] == 0, "Q %d piece %d: %d reads missing", Q, p, m.reads_left[(size_t)p]);
  for (int w = 0; w < ss::kFoldCs16Waves; ++w) EXPECT(m.in_flight[(size_t)w].empty(), "Q %d wave %d leaves the fold with fetches in flight", Q, w);
}

// what the butterflies assume of a run's pieces: radix 8 — slot q holds q; radix 16 — slot i holds 4 sub + i, slot 4 + i its partner q + 8
template <int Q>
void check_slots() {
  using S = ss::FoldCs16Stage<Q>;
  static_assert(S::kPieces * ss::kFoldCs16PieceBytes == S::kFrameBytes, "the pieces are the frame");
  for (int p = 0; p < S::kPieces; ++p) {
    EXPECT(S::half(p) == (p & 1), "Q %d piece %d half", Q, p);
    if (Q == 8) {
      EXPECT(S::rho(p) == p, "Q 8 piece %d run", p);
      for (int s = 0; s < 8; ++s) EXPECT(S::q(p, s) == s, "Q 8 piece %d slot %d", p, s);
    } else {
      EXPECT(S::rho(p) == p / 2, "Q 16 piece %d run", p);
      for (int i = 0; i < 4; ++i) EXPECT(S::q(p, i) == 4 * (p & 1) + i && S::q(p, 4 + i) == S::q(p, i) + 8, "Q 16 piece %d pair %d", p, i);
    }
    const int next = S::issue_behind_barrier(p);
    EXPECT(next == -1 || (next == p + 1 && S::half(next) != S::half(p)), "Q %d piece %d issues %d", Q, p, next);
  }
  EXPECT(S::issue_behind_barrier(0) == -1 && S::issue_behind_barrier(S::kPieces - 1) == -1, "Q %d first and last", Q);
}

}  // namespace

int main() {
  check_slots<8>();
  check_slots<16>();
  for (unsigned seed = 0; seed < 6; ++seed) {
    run<8>(seed);
    run<16>(seed);
  }
  if (g_bad) printf("%ld failures\n", g_bad);
  else printf("all ok\n");
  return g_bad ? 1 : 0;
}
