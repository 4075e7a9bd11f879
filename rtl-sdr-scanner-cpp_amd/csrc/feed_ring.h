// feed_ring.h — the slots of the pipelined feed (host_feed.h) as a ring: which slot the producer fills next, which batch the consumer
// collects next, and the one collected slot a recorder holds (host_record_feed.h). No HIP in here, and nothing but these functions
// writes the counters: tests/host/feed_ring_check.cpp runs them on the CPU against a queue.
//
// A slot goes free -> acquired -> submitted -> free, or, on a feed with a recorder, submitted -> held -> free. Slots are acquired and
// collected in ring order, so batches are collected in the order they were submitted. A held slot stops the next collect at once and
// an acquire only when the ring has come round to it.
#pragma once

namespace ss {
namespace {  // (one includer per binary: nothing of this is exported)

enum class slot_state { free, acquired, submitted, held };

enum class ring_refusal {
  none,
  no_free_slot,     // acquire: the next slot is still submitted or held
  not_acquired,     // submit without an acquired slot
  slot_held,        // oldest_pending / collected: the batch collected last is still held
  nothing_pending,  // oldest_pending / collected
  not_the_oldest,   // collected: another collect took the batch between oldest_pending and here
  nothing_held,     // let_go
};

class feed_ring {
 public:
  static constexpr int kMaxDepth = 8;

  explicit feed_ring(int depth) : depth_(depth) {}

  int depth() const { return depth_; }
  int pending() const { return pending_; }                // submitted, not collected
  int acquired() const { return acquired_; }              // the slot being filled, or -1
  int held() const { return held_; }                      // the slot held for the recorder, or -1
  int last_collected() const { return last_collected_; }  // the slot of the batch collected last, or -1
  bool idle() const { return pending_ == 0 && acquired_ < 0; }
  slot_state state(int slot) const { return state_[slot]; }

  // the slot to fill: the same one again until it is submitted
  ring_refusal acquire(int* slot) {
    if (acquired_ < 0) {
      if (state_[next_acquire_] != slot_state::free) return ring_refusal::no_free_slot;
      state_[next_acquire_] = slot_state::acquired;
      acquired_ = next_acquire_;
      next_acquire_ = (next_acquire_ + 1) % depth_;
    }
    *slot = acquired_;
    return ring_refusal::none;
  }

  ring_refusal submit() {
    if (acquired_ < 0) return ring_refusal::not_acquired;
    state_[acquired_] = slot_state::submitted;
    acquired_ = -1;
    ++pending_;
    return ring_refusal::none;
  }

  // the slot of the batch to collect next
  ring_refusal oldest_pending(int* slot) const {
    if (held_ >= 0) return ring_refusal::slot_held;
    if (pending_ == 0) return ring_refusal::nothing_pending;
    *slot = next_collect_;
    return ring_refusal::none;
  }

  // the batch in `slot`, the oldest pending one, has been collected: its slot is free again, or held until let_go
  ring_refusal collected(int slot, bool hold) {
    int oldest = 0;
    if (const ring_refusal r = oldest_pending(&oldest); r != ring_refusal::none) return r;
    if (slot != oldest) return ring_refusal::not_the_oldest;
    state_[slot] = hold ? slot_state::held : slot_state::free;
    if (hold) held_ = slot;
    last_collected_ = slot;
    next_collect_ = (next_collect_ + 1) % depth_;
    --pending_;
    return ring_refusal::none;
  }

  ring_refusal let_go() {
    if (held_ < 0) return ring_refusal::nothing_held;
    state_[held_] = slot_state::free;
    held_ = -1;
    return ring_refusal::none;
  }

  // a reader of last_collected() that attaches later starts with no batch
  void forget_last_collected() { last_collected_ = -1; }

 private:
  int depth_;
  slot_state state_[kMaxDepth] = {};
  int next_acquire_ = 0, next_collect_ = 0, pending_ = 0;
  int acquired_ = -1, held_ = -1, last_collected_ = -1;
};

}  // namespace
}  // namespace ss
