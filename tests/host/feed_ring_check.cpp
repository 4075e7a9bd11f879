// Host-side check of the pipelined feed's slot ring (csrc/feed_ring.h), compiled with g++ under the sanitizers and run on the CPU by
// tests/test_feed_ring.py: no GPU and no Python in the process.
//   * by hand, at depth 2 and depth 8: a second acquire returns the same slot; a full ring refuses; batches are collected in the order
//     they were submitted; a held slot refuses the next collect at once and an acquire only when the ring has come round to it; let_go
//     frees it; a collect with nothing pending, a collected on another slot than the oldest pending one, a submit with nothing acquired and a let_go
//     with nothing held refuse and change nothing;
//   * a seeded random walk of acquire / submit / collect / let_go against a queue of batch numbers (batch k lives in slot k mod depth;
//     the live batches are the held one, the pending ones and the acquired one, in that order, and the ring is full when there are depth
//     of them), with a recorder (every collected slot is held) and without: every refusal, every slot and every counter agrees.
// Last line: cases <hand-written checks> ops <random operations> refused <of them> collected <batches> bad <failed checks>.
#include <cstdio>
#include <deque>
#include <random>

#include "../../rtl-sdr-scanner-cpp_amd/csrc/feed_ring.h"

namespace {

using ss::feed_ring;
using ss::ring_refusal;
using ss::slot_state;

long g_cases = 0, g_bad = 0;

void expect(bool ok, const char* what, int depth) {
  ++g_cases;
  if (!ok) {
    ++g_bad;
    std::printf("FAILED (depth %d): %s\n", depth, what);
  }
}

int acquire(feed_ring& r) {  // the slot, or -1 for a refusal
  int slot = -7;
  return r.acquire(&slot) == ring_refusal::none ? slot : -1;
}

int collect(feed_ring& r, bool hold) {  // the slot collected, -1 nothing pending, -2 held
  int slot = -7;
  const ring_refusal why = r.oldest_pending(&slot);
  if (why == ring_refusal::slot_held) return -2;
  if (why != ring_refusal::none) return -1;
  return r.collected(slot, hold) == ring_refusal::none ? slot : -3;
}

void by_hand(int depth) {
  {  // a fresh ring
    feed_ring r(depth);
    expect(r.depth() == depth && r.pending() == 0 && r.acquired() == -1 && r.held() == -1 && r.last_collected() == -1 && r.idle(), "a fresh ring is idle", depth);
    expect(collect(r, false) == -1 && r.collected(0, false) == ring_refusal::nothing_pending, "collect with nothing pending refuses", depth);
    expect(r.submit() == ring_refusal::not_acquired && r.pending() == 0, "submit with nothing acquired refuses", depth);
    expect(r.let_go() == ring_refusal::nothing_held, "let_go with nothing held refuses", depth);
    expect(r.idle() && r.last_collected() == -1, "refusals change nothing", depth);
  }
  {  // without a recorder: fill, refuse, drain in order
    feed_ring r(depth);
    expect(acquire(r) == 0 && acquire(r) == 0 && r.acquired() == 0 && !r.idle(), "a second acquire returns the same slot", depth);
    expect(r.state(0) == slot_state::acquired && r.pending() == 0, "an acquired slot is not pending", depth);
    expect(r.submit() == ring_refusal::none && r.acquired() == -1 && r.pending() == 1 && r.state(0) == slot_state::submitted, "submit", depth);
    bool ok = true;
    for (int k = 1; k < depth; ++k) ok = ok && acquire(r) == k && r.submit() == ring_refusal::none;
    expect(ok && r.pending() == depth, "every slot can be in flight", depth);
    expect(acquire(r) == -1 && r.acquired() == -1 && r.pending() == depth, "a full ring refuses", depth);
    expect(r.collected(1, false) == ring_refusal::not_the_oldest && r.pending() == depth && r.state(1) == slot_state::submitted && r.last_collected() == -1,
           "collected on a slot that is not the oldest pending one refuses", depth);
    ok = true;
    for (int k = 0; k < depth; ++k) ok = ok && collect(r, false) == k && r.last_collected() == k && r.state(k) == slot_state::free && r.pending() == depth - 1 - k;
    expect(ok, "collection is in submit order", depth);
    expect(collect(r, false) == -1 && r.idle() && r.last_collected() == depth - 1, "drained: nothing pending", depth);
    expect(acquire(r) == 0, "the ring wraps", depth);
    r.forget_last_collected();
    expect(r.last_collected() == -1 && r.acquired() == 0, "forget_last_collected touches nothing else", depth);
  }
  {  // with a recorder: the collected slot is held
    feed_ring r(depth);
    bool ok = true;
    for (int k = 0; k < 2; ++k) ok = ok && acquire(r) == k && r.submit() == ring_refusal::none;
    expect(ok && collect(r, true) == 0 && r.held() == 0 && r.state(0) == slot_state::held && r.pending() == 1 && r.last_collected() == 0, "a collected slot is held", depth);
    expect(collect(r, true) == -2 && r.collected(1, true) == ring_refusal::slot_held && r.pending() == 1 && r.held() == 0, "a held slot refuses the next collect", depth);
    // slots 2 .. depth - 1 are free: the held slot 0 is in the way only when the ring wraps onto it
    ok = true;
    for (int k = 2; k < depth; ++k) ok = ok && acquire(r) == k && r.submit() == ring_refusal::none;
    expect(ok && r.pending() == depth - 1, "a held slot does not refuse an acquire of another slot", depth);
    expect(acquire(r) == -1 && r.acquired() == -1, "... and refuses once the ring wraps onto it", depth);
    expect(r.let_go() == ring_refusal::none && r.held() == -1 && r.state(0) == slot_state::free && r.last_collected() == 0, "let_go frees it", depth);
    expect(acquire(r) == 0 && acquire(r) == 0, "... for the producer", depth);
    expect(collect(r, true) == 1 && r.held() == 1 && r.last_collected() == 1, "... and the next collect goes on in order", depth);
    expect(r.let_go() == ring_refusal::none && r.let_go() == ring_refusal::nothing_held, "let_go twice: the second refuses", depth);
  }
}

// the queue the ring is compared with
struct Model {
  long next = 0;           // batches acquired so far
  long held = -1;          // batch numbers, -1: none
  std::deque<long> pending;
  long acquired = -1;
  long last = -1;
  int live() const { return (held >= 0) + (int)pending.size() + (acquired >= 0); }
};

void random_walk(int depth, bool recorder, unsigned seed, long ops, long* refused, long* collected) {
  std::mt19937 rng(seed);
  feed_ring r(depth);
  Model m;
  char what[160];
  for (long i = 0; i < ops; ++i) {
    const int op = (int)(rng() % 8);
    bool ok = true;
    if (op < 3) {  // acquire
      const int got = acquire(r);
      if (m.acquired < 0 && m.live() < depth) m.acquired = m.next++;
      const int want = m.acquired >= 0 ? (int)(m.acquired % depth) : -1;
      ok = got == want;
      *refused += got < 0;
    } else if (op < 5) {  // submit
      const ring_refusal got = r.submit();
      ok = (got == ring_refusal::none) == (m.acquired >= 0) && (got == ring_refusal::none || got == ring_refusal::not_acquired);
      if (m.acquired >= 0) m.pending.push_back(m.acquired);
      m.acquired = -1;
      *refused += got != ring_refusal::none;
    } else if (op < 7) {  // collect
      const int got = collect(r, recorder);
      int want = -1;
      if (m.held >= 0) want = -2;
      else if (!m.pending.empty()) {
        want = (int)(m.pending.front() % depth);
        m.last = m.pending.front();
        if (recorder) m.held = m.pending.front();
        m.pending.pop_front();
        ++*collected;
      }
      ok = got == want;
      *refused += got < 0;
    } else {  // let_go
      const ring_refusal got = r.let_go();
      ok = (got == ring_refusal::none) == (m.held >= 0) && (got == ring_refusal::none || got == ring_refusal::nothing_held);
      m.held = -1;
      *refused += got != ring_refusal::none;
    }
    ok = ok && r.pending() == (int)m.pending.size() && r.acquired() == (m.acquired >= 0 ? (int)(m.acquired % depth) : -1) &&
         r.held() == (m.held >= 0 ? (int)(m.held % depth) : -1) && r.last_collected() == (m.last >= 0 ? (int)(m.last % depth) : -1) &&
         r.idle() == (m.pending.empty() && m.acquired < 0);
    int occupied = 0;
    for (int s = 0; s < depth; ++s) occupied += r.state(s) != slot_state::free;
    ok = ok && occupied == m.live();
    std::snprintf(what, sizeof what, "random walk, %s a recorder, seed %u: operation %ld (kind %d)", recorder ? "with" : "without", seed, i, op);
    expect(ok, what, depth);
    if (!ok) return;
  }
}

}  // namespace

int main() {
  for (int depth : {2, 8}) by_hand(depth);
  const long hand = g_cases;
  long ops = 0, refused = 0, collected = 0;
  for (int depth : {2, 3, 8})
    for (int recorder = 0; recorder < 2; ++recorder)
      for (unsigned seed = 1; seed <= 2; ++seed) {
        random_walk(depth, recorder != 0, seed * 100u + (unsigned)depth, 4000, &refused, &collected);
        ops += 4000;
      }
  std::printf("cases %ld ops %ld refused %ld collected %ld bad %ld\n", hand, ops, refused, collected, g_bad);
  return g_bad == 0 ? 0 : 1;
}
