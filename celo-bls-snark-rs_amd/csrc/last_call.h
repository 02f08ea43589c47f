// The "last call" records of the library (what the celo_amd_*_last* getters report), in one type.  Standard library only: a plain host
// compiler builds this header (tests/last_call_tsan_main.cpp runs it under ThreadSanitizer).  The rule is in runtime.h and DESIGN.md section 1b:
// times are call-local, published once, sub-call times are handed up; a getter takes the record's lock alone, never a unit's whole-call lock.
#pragma once
#include <chrono>
#include <mutex>

namespace celo {

// One published record: whole under its own lock.  update(): for a record whose slots have different owners (the R1CS record's prover and setup slots)
template <class T> class Last {
 public:
  void note(const T& v) { std::lock_guard<std::mutex> lk(mu_); v_ = v; }
  T read() const { std::lock_guard<std::mutex> lk(mu_); return v_; }
  template <class F> void update(F f) { std::lock_guard<std::mutex> lk(mu_); f(v_); }
 private:
  mutable std::mutex mu_;
  T v_{};
};

// stage times in ms and up to two integers (path / lanes / window bits, by the record's own header comment)
struct CallTimes { float ms[8] = {}; int tag[2] = {-1, 0}; };

// Wall-clock ms since construction.  With a slot: written there on destruction.
struct WallMs {
  explicit WallMs(float* slot_ = nullptr) : slot(slot_) {}
  ~WallMs() { if (slot) *slot = ms(); }
  float ms() const { return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
  const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  float* const slot;
};

// The record of a call that publishes on EVERY exit: the call fills `t`, the destructor writes the wall slot and notes the record.  Declared
// in front of the CallScope, the wall time includes the release of the call's resources, and a call that leaves early publishes what it had.
struct TimedCall {
  TimedCall(Last<CallTimes>& rec_, int wall_slot_) : rec(rec_), wall_slot(wall_slot_) {}
  TimedCall(const TimedCall&) = delete;
  ~TimedCall() { t.ms[wall_slot] = wall.ms(); rec.note(t); }
  CallTimes t;
  const WallMs wall;
  Last<CallTimes>& rec; const int wall_slot;
};

}  // namespace celo
