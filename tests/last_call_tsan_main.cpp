// A program of its own for tests/test_last_call_host.py, built with -fsanitize=thread: csrc/last_call.h alone, no device, no library.
//   1. Last<> under contention: four threads note() records whose eight slots and two tags all equal the writer's constant, one thread
//      update()s slot 3 of a second record with 1, 2, 3, .., two threads read() both.  Every record read is uniform, the updated slot only
//      ever holds a value that was written (and never goes back), the other slots of that record stay as they were.
//   2. TimedCall: a scope left normally publishes its slots and a wall slot > 0; a scope left early publishes what it had; the wall slot of a
//      guard declared in front of an object whose destructor sleeps 5 ms is at least 5 ms (the declaration-order rule of runtime.h).
// Prints "last_call ok" and exits 0; any violated check prints a line and exits 1.  A ThreadSanitizer report makes the exit status non-zero.
#include "last_call.h"
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

using namespace celo;

static constexpr int ITER = 100000, WRITERS = 4, UPDATED_SLOT = 3;
static std::atomic<int> g_bad{0};
static void fail(const char* what, double a, double b) {
  if (g_bad.fetch_add(1) < 10) fprintf(stderr, "FAIL %s: %g %g\n", what, a, b);
}

static CallTimes uniform(int k) {
  CallTimes t;
  for (float& v : t.ms) v = (float)k;
  t.tag[0] = t.tag[1] = k;
  return t;
}
static void check_uniform(const CallTimes& t) {
  const int k = t.tag[0];
  if (k < 1 || k > WRITERS) fail("tag out of range", k, 0);
  if (t.tag[1] != k) fail("tags differ", k, t.tag[1]);
  for (float v : t.ms) if (v != (float)k) fail("slot differs from tag", v, k);
}
// the second record: slot 3 a whole number in [lo, ITER], everything else as constructed
static float check_updated(const CallTimes& t, float lo) {
  const float v = t.ms[UPDATED_SLOT];
  if (v < lo || v > (float)ITER || v != (float)(int)v) fail("updated slot", v, lo);
  for (int i = 0; i < 8; i++) if (i != UPDATED_SLOT && t.ms[i] != 0.f) fail("foreign slot touched", i, t.ms[i]);
  if (t.tag[0] != -1 || t.tag[1] != 0) fail("tags touched", t.tag[0], t.tag[1]);
  return v;
}

struct SleepsOnExit { ~SleepsOnExit() { std::this_thread::sleep_for(std::chrono::milliseconds(5)); } };

static int leaves_early(Last<CallTimes>& rec, volatile bool early) {
  TimedCall call(rec, 6);
  call.t.ms[1] = 2.5f;
  call.t.tag[0] = 4;
  if (early) return 7;
  call.t.ms[2] = 9.f;
  return 0;
}

int main() {
  // ---- 1
  Last<CallTimes> noted, updated;
  noted.note(uniform(1));
  std::vector<std::thread> th;
  for (int k = 1; k <= WRITERS; k++)
    th.emplace_back([&noted, k] { const CallTimes mine = uniform(k); for (int i = 0; i < ITER; i++) noted.note(mine); });
  th.emplace_back([&updated] { for (int i = 1; i <= ITER; i++) updated.update([i](CallTimes& t) { t.ms[UPDATED_SLOT] = (float)i; }); });
  for (int r = 0; r < 2; r++)
    th.emplace_back([&noted, &updated] {
      float seen = 0.f;
      for (int i = 0; i < ITER; i++) {
        check_uniform(noted.read());
        seen = check_updated(updated.read(), seen);
      }
    });
  for (auto& t : th) t.join();
  check_uniform(noted.read());
  if (check_updated(updated.read(), (float)ITER) != (float)ITER) fail("last update lost", 0, 0);

  // ---- 2
  Last<CallTimes> rec;
  {
    TimedCall call(rec, 6);
    call.t.ms[0] = 1.5f;
    call.t.tag[1] = 8;
    std::this_thread::sleep_for(std::chrono::milliseconds(1));
    if (rec.read().ms[0] != 0.f) fail("published before the scope ended", rec.read().ms[0], 0);
  }
  CallTimes t = rec.read();
  if (t.ms[0] != 1.5f || t.tag[0] != -1 || t.tag[1] != 8 || !(t.ms[6] > 0.f)) fail("normal exit", t.ms[0], t.ms[6]);
  for (int i = 1; i < 8; i++) if (i != 6 && t.ms[i] != 0.f) fail("normal exit: unused slot", i, t.ms[i]);

  if (leaves_early(rec, true) != 7) fail("early return value", 0, 0);
  t = rec.read();
  if (t.ms[0] != 0.f || t.ms[1] != 2.5f || t.ms[2] != 0.f || t.tag[0] != 4 || !(t.ms[6] >= 0.f)) fail("early exit", t.ms[1], t.ms[2]);

  {
    TimedCall call(rec, 3);
    SleepsOnExit resources;          // declared after the guard: released before the guard takes the wall time
  }
  t = rec.read();
  if (!(t.ms[3] >= 5.f)) fail("declaration order: wall below the release time", t.ms[3], 5);

  if (g_bad.load()) { printf("last_call FAILED: %d checks\n", g_bad.load()); return 1; }
  printf("last_call ok\n");
  return 0;
}
