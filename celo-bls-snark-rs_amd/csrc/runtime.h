// Process-wide runtime of the gfx950 library: device binding per host thread and pools of engine instances.
//
// The reference's callers are synchronous, re-entrant and multi-threaded (bls-snark-sys is called from Go/Rust worker threads:
// crates/bls-snark-sys/src/cache.rs:5, signatures.rs:343-400; epoch-snark's prover runs its MSMs from rayon tasks,
// crates/epoch-snark/src/api/prover.rs:78).  So there is no global API lock: every entry point
//   1. api_enter()          binds the calling thread to its device (HIP's current device is per thread),
//   2. EnginePool::lease()  checks out an engine instance of that device (workspace arena, pinned staging, events and its
//                           own non-blocking HIP stream); a new one is created when all are busy (up to MAX_PER_DEVICE,
//                           then callers wait),
//   3. runs, copies its timings to the per-kind "last call" record, and returns the engine.
// The records (last_call.h): a call keeps its times in its own frame and publishes them once - at its successful end, or, for the composed bulk
// calls, through a TimedCall on every exit; a sub-call hands its time up through a trailing `float* kernel_ms` (units.h) and notes its own record
// besides; no unit reads another's record, and a getter takes the record's lock alone.  The whole-call locks of the bulk units stay (one call fills
// the GPU) and guard: hash_mu the hash scratch, its stream and the generator tables' device copies; agg_mu, vb_mu and setup_mu their units' settings
// (g_agg_lanes / g_agg_complement, g_vb_c / g_vb_chunk, g_fb_c); wire_mu, w761_mu, wenc_mu, trans_mu and epoch_mu serialisation only.
// Independent calls therefore overlap on the GPU (separate streams) and several devices can be driven from one process:
// celo_amd_use_device() binds a host thread to a device, the msm_*_multi entry points do that internally (one thread per device).
#pragma once
#include <hip/hip_runtime.h>
#include <sys/random.h>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <memory>
#include <mutex>
#include <vector>
#include "last_call.h"

// a failed HIP call: logged (the expression, HIP's message, where), then the calling function returns rc
#define HIP_TRY(x, rc)                                                                                            \
  do {                                                                                                            \
    const hipError_t e_ = (x);                                                                                    \
    if (e_ != hipSuccess) {                                                                                       \
      fprintf(stderr, "[celo-amd] %s: %s at %s:%d\n", #x, hipGetErrorString(e_), __FILE__, __LINE__);             \
      return rc;                                                                                                  \
    }                                                                                                             \
  } while (0)

namespace celo {

constexpr int MAX_DEVICES = 16;

int api_enter();                 // 0, or 100 (no device).  Applies the thread's device.
int api_device();                // device of the calling thread (after api_enter)
int api_bind_thread(int device); // celo_amd_use_device: 0 or 101

template <class E> class EnginePool {
 public:
  static constexpr int MAX_PER_DEVICE = 8;
  class Lease {
   public:
    Lease(EnginePool* p, int dev, E* e) : pool(p), device(dev), eng(e) {}
    Lease(Lease&& o) noexcept : pool(o.pool), device(o.device), eng(o.eng) { o.eng = nullptr; }
    Lease(const Lease&) = delete;
    ~Lease() { if (eng) pool->give_back(device, eng); }
    E* operator->() { return eng; }
    E& operator*() { return *eng; }
    explicit operator bool() const { return eng != nullptr; }
   private:
    EnginePool* pool; int device; E* eng;
  };
  // the calling thread must have passed api_enter()
  Lease lease() {
    const int dev = api_device();
    std::unique_lock<std::mutex> lk(mu);
    Slot& s = slots[dev];
    for (;;) {
      if (!s.free_list.empty()) { E* e = s.free_list.back(); s.free_list.pop_back(); return Lease(this, dev, e); }
      if (s.created < MAX_PER_DEVICE) {   // engines live for the process
        s.created++;
        lk.unlock();
        E* e = nullptr;
        try { e = new E(); } catch (...) {            // a failed construction must not cost the pool a slot for good
          { std::lock_guard<std::mutex> g(mu); slots[dev].created--; }
          cv.notify_one();
          throw;
        }
        return Lease(this, dev, e);
      }
      cv.wait(lk);
    }
  }
 private:
  struct Slot { std::vector<E*> free_list; int created = 0; };
  Slot slots[MAX_DEVICES];
  std::mutex mu;
  std::condition_variable cv;
  void give_back(int dev, E* e) {
    { std::lock_guard<std::mutex> lk(mu); slots[dev].free_list.push_back(e); }
    cv.notify_one();
  }
};

// celo_amd_msm_set_host_chunks (tests, bench.py's sweep): >= 0 overrides CELO_HOST_CHUNKS for the host-pointer MSM calls that follow
// (msm.h run_host_windows); -1 = the default
inline std::atomic<int>& host_chunks_override() { static std::atomic<int> v{-1}; return v; }
inline std::atomic<int>& batched_affine_override() { static std::atomic<int> v{-1}; return v; }   // -1: CELO_BA / the default (csrc/msm_ba.h)

// The chunks of the host-pointer pipeline: `chunks` index chunks of cm points (a multiple of 1024), the FIRST of them cut in halves
// `head_split` times, smallest piece first - the pipeline is bound by the GPU's work from the moment the first chunk has landed
// (accumulating a chunk takes a little longer than sending the next), so what the call pays beyond the resident pipeline is the
// first chunk's transfer: it is short.  On the device chunk k lives at the virtual index k cm (the staging buffers have holes behind
// short chunks): nothing below the transfers knows chunk lengths.  Returns the number of chunks (<= 80 = 64 + 8 + 8).
constexpr uint32_t HOST_CHUNKS_MAX = 80;
inline uint32_t host_chunk_plan(size_t n, uint32_t chunks, uint32_t head_split, uint32_t tail_split, uint32_t& cm, uint32_t* clen) {
  cm = (uint32_t)(((n + chunks - 1) / chunks + 1023u) & ~size_t(1023));
  const uint32_t base = (uint32_t)((n + cm - 1) / cm);
  uint32_t halves[8], nh = 0, piece = base >= 2 ? cm : (uint32_t)n;      // (one chunk: the whole job, cut by head_split only)
  for (uint32_t t = 0; t < head_split && t < 8 && piece >= (1u << 16); t++) {
    halves[nh] = ((piece + 1) / 2 + 1023u) & ~1023u;
    piece -= halves[nh++];
  }
  uint32_t K = 0;
  clen[K++] = piece;
  while (nh) clen[K++] = halves[--nh];
  if (base < 2) return K;
  for (uint32_t b = 1; b + 1 < base; b++) clen[K++] = cm;
  piece = (uint32_t)(n - (size_t)(base - 1) * cm);           // the last base chunk, largest piece first
  for (uint32_t t = 0; t < tail_split && t < 8 && piece >= (1u << 16); t++) {
    const uint32_t half = ((piece + 1) / 2 + 1023u) & ~1023u;
    clen[K++] = half;
    piece -= half;
  }
  clen[K++] = piece;
  return K;
}

// an engine-owned stream: non-blocking, so that engines of different calls do not serialise through the null stream
struct OwnedStream {
  hipStream_t s = nullptr;
  hipStream_t get() {
    if (!s && hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) s = nullptr;
    return s;
  }
};

// n bytes from the operating system (the seed of an exponent stream); false when it gives none
inline bool os_random(void* buf, size_t n) {
  for (size_t got = 0; got < n;) {
    const ssize_t r = getrandom((uint8_t*)buf + got, n - got, 0);
    if (r <= 0) return false;
    got += (size_t)r;
  }
  return true;
}

// The device resources of ONE call: its allocations, its events and, when create_stream() made one, its stream.  The call runs on
// stream() - the caller's, the null stream, or its own.  Released on every exit, in this order: the stream is synchronised, the
// allocations freed, the events destroyed, then an owned stream destroyed.
//
// The call frame of an entry point that takes host pointers (dev = 0) or device pointers (dev = 1): open() picks the stream, in() / out() /
// inout() name what crosses the bus - with dev set they hand the caller's pointer through, otherwise they allocate and stage -, the unit
// enqueues its work on stream(), copy_back() enqueues the way home, and the unit synchronises where it reads the results.
class CallScope {
 public:
  explicit CallScope(hipStream_t s = nullptr) : s_(s) {}
  CallScope(const CallScope&) = delete;
  CallScope& operator=(const CallScope&) = delete;
  ~CallScope() {
    (void)hipStreamSynchronize(s_);
    for (void* p : mem_) (void)hipFree(p);
    for (hipEvent_t e : ev_) (void)hipEventDestroy(e);
    if (owned_) (void)hipStreamDestroy(s_);
  }
  hipStream_t stream() const { return s_; }
  hipError_t create_stream() {        // a non-blocking stream of the call's own, in place of the one given
    hipStream_t s = nullptr;
    const hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e == hipSuccess) { s_ = s; owned_ = true; }
    return e;
  }
  template <class T> hipError_t alloc(T** p, size_t bytes) {
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, bytes);
    if (e == hipSuccess) mem_.push_back(q);
    *p = (T*)q;
    return e;
  }
  hipError_t event(hipEvent_t* out) {
    hipEvent_t e = nullptr;
    const hipError_t rc = hipEventCreate(&e);
    if (rc == hipSuccess) ev_.push_back(e);
    *out = e;
    return rc;
  }
  // dev: the call runs on the caller's stream; else on a non-blocking stream of its own
  hipError_t open(int dev, void* caller_stream) {
    if (!dev) return create_stream();
    s_ = (hipStream_t)caller_stream;
    return hipSuccess;
  }
  // an input of `bytes` at p: *d = p (dev, or p == nullptr: an optional input that is absent), else a device copy of bytes + pad, enqueued
  template <class T> hipError_t in(T** d, const void* p, size_t bytes, int dev, size_t pad = 0) {
    *d = (T*)p;
    if (dev || !p) return hipSuccess;
    const hipError_t e = alloc(d, bytes + pad);
    return e != hipSuccess ? e : hipMemcpyAsync(*d, p, bytes, hipMemcpyHostToDevice, s_);
  }
  // an output of `bytes` at p: *d = p (dev, or p == nullptr), else a device buffer that copy_back() returns to p
  template <class T> hipError_t out(T** d, void* p, size_t bytes, int dev) {
    *d = (T*)p;
    if (dev || !p) return hipSuccess;
    const hipError_t e = alloc(d, bytes);
    if (e == hipSuccess) back_.push_back({p, *d, bytes});
    return e;
  }
  // a buffer the call overwrites in place
  template <class T> hipError_t inout(T** d, void* p, size_t bytes, int dev) {
    const hipError_t e = in(d, p, bytes, dev);
    if (e == hipSuccess && !dev && p) back_.push_back({p, *d, bytes});
    return e;
  }
  hipError_t copy_back() {            // every registered output, in registration order; the caller synchronises
    for (const Back& b : back_) {
      const hipError_t e = hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, s_);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }
 private:
  struct Back { void* host; const void* dev; size_t bytes; };
  hipStream_t s_ = nullptr;
  bool owned_ = false;
  std::vector<void*> mem_;
  std::vector<Back> back_;
  std::vector<hipEvent_t> ev_;
};


// kernel-time accounting by event pairs per category (read after the call's final synchronisation).  The log owns every event from its creation:
// a call that leaves between open() and close() leaks none
struct EvLog {
  struct Rec { int cat; hipEvent_t a, b; };
  std::vector<Rec> recs;
  std::vector<hipEvent_t> events;
  hipStream_t s;
  explicit EvLog(hipStream_t st) : s(st) {}
  hipEvent_t open() { hipEvent_t e = nullptr; if (hipEventCreate(&e) != hipSuccess) return nullptr; events.push_back(e); (void)hipEventRecord(e, s); return e; }
  void close(int cat, hipEvent_t a) { if (hipEvent_t e = a ? open() : nullptr) recs.push_back({cat, a, e}); }
  void sum(float* ms) {
    for (auto& r : recs) { float t = 0.f; if (hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) ms[r.cat] += t; }
  }
  ~EvLog() { for (hipEvent_t e : events) (void)hipEventDestroy(e); }
};

// ---- chaining engines on the device (batch verification: MSM results -> normalise -> pairing inputs, no host round trip)
// A batched MSM that has been ENQUEUED on its engine's stream: d_out = m Jacobian results (arkworks form) in the engine's
// arena; the engine stays leased until msm_batch_end_*.
// bits: in - the length of the longest scalar if the caller knows it (0: measure); out - what the run used
struct BatchRun { void* lease = nullptr; uint64_t* d_out = nullptr; hipStream_t stream = nullptr; int bits = 0; };
// A pairing engine whose input slots (k pairs in m products) are handed to a producer kernel; pairing_run_staged_* runs the
// check on what the slots hold (stream order) and returns the engine.
struct PairingStage { void* lease = nullptr; uint64_t* d_g1 = nullptr; uint64_t* d_g2 = nullptr; uint8_t* d_i1 = nullptr; uint8_t* d_i2 = nullptr; hipStream_t stream = nullptr; };
// One staged pairing product over the engine of D (units.h Pairing377 / Pairing761): stage(), optionally after() a producer, the caller's
// pack kernel and tail uploads into ps's slots on ps.stream, run().  An engine that was staged and not run goes back to its pool.
template <class D> struct StagedProduct {
  PairingStage ps;
  ~StagedProduct() { if (ps.lease) (void)D::run_staged(&ps, nullptr, 0, nullptr, nullptr); }
  int stage(uint32_t pairs, size_t products) { return D::stage(pairs, products, &ps); }
  int after(CallScope& cs) {          // the engine's stream waits for what cs.stream() holds now
    hipEvent_t ready;
    HIP_TRY(cs.event(&ready), 10);
    HIP_TRY(hipEventRecord(ready, cs.stream()), 10);
    HIP_TRY(hipStreamWaitEvent(ps.stream, ready, 0), 10);
    return 0;
  }
  // m verdicts (host bytes) for the products [off[p], off[p + 1]); synchronises the engine's stream, and a producer's through after()'s event.
  // The engine's time for this product is ADDED to *ms_pair
  int run(const uint32_t* off, size_t m, uint8_t* is_one, float* ms_pair) {
    float pm = 0.f;
    if (int rc = D::run_staged(&ps, off, m, is_one, &pm)) return rc;
    *ms_pair += pm;
    return 0;
  }
};

}  // namespace celo
