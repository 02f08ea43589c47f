// Seam A, the batch verifiers (seam.h has the map of the units): batch_verify_signature, and batch_verify_strict with the per-device
// mirrors of the handle arenas it keeps in HBM.
#include <algorithm>
#include <condition_variable>
#include <functional>
#include <memory>
#include <new>
#include <unistd.h>
#include "seam.h"

using namespace celo;
using namespace celo::seam;

namespace {
// Persistent host workers for the per-call passes over 10^6 handles: creating 64 threads costs 1.5-4 ms per call (measured inside
// batch_verify_strict at config-3 scale), waking 64 sleeping ones ~0.1 ms.  One job at a time; a caller that finds the pool busy (a
// concurrent call on another device) or without threads runs its ranges on threads of its own / inline as before.  The pool object is
// never destroyed and its threads are detached: nothing to join at process exit.
struct HostPool {
  std::mutex mu, busy;
  std::condition_variable cv, cv_done;
  std::function<void(unsigned)> job;
  unsigned n = 0, next = 0, finished = 0, nthreads = 0;
  std::atomic<bool> job_failed{false};          // a range of the current job threw (out of memory): the submitter treats the call as failed
  pid_t owner = 0;                              // a fork()ed child has this object but none of its threads: it must not wait for them
  static HostPool& get() { static HostPool* p = new HostPool; return *p; }
  HostPool() {
    owner = getpid();
    unsigned hw = std::thread::hardware_concurrency();
    if (hw > 64) hw = 64;
    for (unsigned i = 0; i < hw; i++) {
      try { std::thread([this]() { loop(); }).detach(); nthreads++; } catch (...) { break; }
    }
  }
  void loop() {
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      cv.wait(lk, [&] { return next < n; });
      const unsigned i = next++;
      lk.unlock();
      try { job(i); } catch (...) { job_failed = true; }
      lk.lock();
      if (++finished == n) cv_done.notify_all();
    }
  }
  bool try_begin(unsigned count, std::function<void(unsigned)> fn) {
    if (count == 0 || count > nthreads || getpid() != owner || !busy.try_lock()) return false;
    { std::lock_guard<std::mutex> lk(mu); job = std::move(fn); n = count; next = 0; finished = 0; job_failed = false; }
    cv.notify_all();
    return true;
  }
  bool finish() {      // false: a range of the job threw
    bool ok;
    { std::unique_lock<std::mutex> lk(mu); cv_done.wait(lk, [&] { return finished == n; }); n = 0; next = 0; finished = 0; job = nullptr; ok = !job_failed.load(); }
    busy.unlock();
    return ok;
  }
};

// ---------------------------------------------------------------- batch_verify_strict: what a device keeps between calls
// Per device (a caller bound to another device with celo_amd_use_device must not run its engines against device-0 memory and a
// device-0 stream): one grow-only PINNED host staging buffer, its device twin, one copy stream, and the MIRRORS of the two handle
// arenas - for every arena slot the affine point (192 / 96 bytes) and an identity byte in HBM, tagged on the host with the serial of
// the allocation they were uploaded for.  A call then moves, per signer, two 4-byte slot numbers (the exponents are drawn on the device); only
// handles the device has not seen in their present state (new since the last call, or a reused slot) are normalised and uploaded,
// and the dense point arrays the batch MSMs read are gathered on the GPU (unit_batchverify.hip: k_mirror_scatter / k_mirror_gather).
// Round 3 gathered and shipped 320 bytes per signer on every call: 8 ms before the G2 MSM - the longest leg - could start.
struct Mirror {
  uint64_t* d_xy = nullptr; uint8_t* d_inf = nullptr; uint32_t cap = 0;
  std::unique_ptr<std::atomic<uint64_t>[]> seen;                      // serial of the allocation whose point sits in the slot's row (0: none)
  bool grow(uint32_t need, int words) {
    if (need <= cap) return true;
    uint64_t ncap64 = ((uint64_t)need + 0xffffu) & ~(uint64_t)0xffffu;
    if (ncap64 < 2 * (uint64_t)cap) ncap64 = 2 * (uint64_t)cap;
    if (ncap64 > 0xffffffffu) ncap64 = 0xffffffffu;
    const uint32_t ncap = (uint32_t)ncap64;
    uint64_t* nx = nullptr; uint8_t* ni = nullptr;
    std::unique_ptr<std::atomic<uint64_t>[]> ns(new (std::nothrow) std::atomic<uint64_t>[ncap]);
    if (!ns || hipMalloc((void**)&nx, (size_t)ncap * words * 8) != hipSuccess) return false;
    if (hipMalloc((void**)&ni, ncap) != hipSuccess) { (void)hipFree(nx); return false; }
    if (cap && (hipMemcpy(nx, d_xy, (size_t)cap * words * 8, hipMemcpyDeviceToDevice) != hipSuccess ||
                hipMemcpy(ni, d_inf, cap, hipMemcpyDeviceToDevice) != hipSuccess)) { (void)hipFree(nx); (void)hipFree(ni); return false; }
    for (uint32_t i = 0; i < ncap; i++) ns[i].store(i < cap ? seen[i].load(std::memory_order_relaxed) : 0, std::memory_order_relaxed);
    if (d_xy) (void)hipFree(d_xy);
    if (d_inf) (void)hipFree(d_inf);
    d_xy = nx; d_inf = ni; cap = ncap; seen = std::move(ns);
    return true;
  }
  void forget() { for (uint32_t i = 0; i < cap; i++) seen[i].store(0, std::memory_order_relaxed); }
};
// A grow-only buffer, pinned host memory or device memory: reserve() leaves at least `need` bytes and, when it has to reallocate, a
// quarter more (the contents are not kept).  On failure the buffer is empty.
struct GrowBuf {
  enum Kind { PINNED_HOST, DEVICE };
  uint8_t* p = nullptr; size_t cap = 0;
  bool reserve(size_t need, Kind kind) {
    if (need <= cap) return true;
    if (p) (void)(kind == PINNED_HOST ? hipHostFree(p) : hipFree(p));
    p = nullptr; cap = 0;
    const size_t bytes = need + need / 4;
    if ((kind == PINNED_HOST ? hipHostMalloc((void**)&p, bytes, hipHostMallocDefault) : hipMalloc((void**)&p, bytes)) != hipSuccess) { p = nullptr; return false; }
    cap = bytes;
    return true;
  }
};
// Per device: the mirrors, the pinned host staging and the upload buffer are shared by the calls and used under `mu` - but only for the
// MIRROR PHASE of a call (host pass over the handles, new rows across, the dense arrays gathered: a few ms); the gathered arrays, the
// exponents and the hash points live in a per-call lease from `dpool`, so the lock is released before the call's long part - two batch
// MSMs and the pairing checks on pooled, lock-free engines - and two host threads verifying different epochs overlap there (round 5,
// the reference's batch_verify_strict is re-entrant, crates/bls-snark-sys/src/signatures.rs:343; rounds 3-4 held the
// lock for the whole call).
struct DStage { GrowBuf buf; bool busy = false; };
struct DevStage {
  std::mutex mu; GrowBuf stage, d_up; hipStream_t copy_stream = nullptr; Mirror keys, sigs;
  std::mutex pool_mu; std::condition_variable pool_cv; DStage dpool[8];
};
DevStage& dev_stage(int device) { static DevStage s[MAX_DEVICES]; return s[device]; }
struct DLease {
  DevStage& ds; DStage* slot = nullptr;
  explicit DLease(DevStage& d) : ds(d) {}
  uint8_t* take(size_t need) {          // a free buffer of the pool, grown if it is too small; waits while all eight are out
    std::unique_lock<std::mutex> lk(ds.pool_mu);
    for (;;) {
      DStage *fit = nullptr, *big = nullptr;          // the smallest free buffer that holds the call, else the largest free one (to be grown)
      for (DStage& q : ds.dpool) {
        if (q.busy) continue;
        if (q.buf.cap >= need && (!fit || q.buf.cap < fit->buf.cap)) fit = &q;
        if (!big || q.buf.cap > big->buf.cap) big = &q;
      }
      DStage* best = fit ? fit : big;
      if (best) { best->busy = true; slot = best; break; }
      ds.pool_cv.wait(lk);
    }
    lk.unlock();
    return slot->buf.reserve(need, GrowBuf::DEVICE) ? slot->buf.p : nullptr;
  }
  ~DLease() {
    if (!slot) return;
    { std::lock_guard<std::mutex> lk(ds.pool_mu); slot->busy = false; }
    ds.pool_cv.notify_one();
  }
};
struct JoinAll { std::vector<std::thread>& v; ~JoinAll() { for (auto& t : v) if (t.joinable()) t.join(); } };
struct PoolWait { HostPool& p; bool on; bool& failed; ~PoolWait() { if (on && !p.finish()) failed = true; } };   // the job holds references to the caller's frame

// ---------------------------------------------------------------- batch_verify_strict: one call
// The two staging buffers of a call are carved by ONE walk each over a running offset: the walk hands out every sub-array's offset and adds
// up what to allocate - the arrays, a full 256 bytes for every rounding, 4 096 bytes of slack - so a sub-array cannot be added to the one and
// forgotten in the other.  Index 0 is the keys, index 1 the signatures, as in Side below.
constexpr int XY_WORDS[2] = {24, 12}, JAC_WORDS[2] = {36, 18};           // u64 per affine / Jacobian point: G2, G1
struct Walk {
  size_t off = 0, bytes = 4096;
  template <class T> size_t take(size_t count) { const size_t at = off; off += count * sizeof(T); bytes += count * sizeof(T); return at; }
  void round256() { off = (off + 255) & ~size_t(255); bytes += 256; }
};
struct HostLayout {      // pinned host staging: rows of the handles to upload (worst case: every signer's) and the slot numbers
  size_t rows[2], idx[2], slots[2], inf[2], bytes;
  explicit HostLayout(size_t tot) {
    Walk w;
    for (int s = 0; s < 2; s++) rows[s] = w.take<uint64_t>(tot * XY_WORDS[s]);
    for (int s = 0; s < 2; s++) idx[s] = w.take<uint32_t>(tot);
    for (int s = 0; s < 2; s++) slots[s] = w.take<uint32_t>(tot);
    for (int s = 0; s < 2; s++) inf[s] = w.take<uint8_t>(tot);
    bytes = w.bytes;
  }
};
struct DevLayout {       // device staging: the gathered point arrays, the exponents, the slot numbers; m hash points and flags behind them
  // (the roundings act on OFFSETS: they align the addresses because hipMalloc returns blocks aligned to 256 bytes at least)
  size_t rows[2], sc, idx[2], inf[2], hxy, hinf, offs, bytes;
  DevLayout(size_t tot, size_t m) {
    Walk w;
    for (int s = 0; s < 2; s++) rows[s] = w.take<uint64_t>(tot * XY_WORDS[s]);
    sc = w.take<uint64_t>(tot * 4);
    for (int s = 0; s < 2; s++) idx[s] = w.take<uint32_t>(tot);
    for (int s = 0; s < 2; s++) inf[s] = w.take<uint8_t>(tot);
    w.round256();
    hxy = w.take<uint64_t>(m * 12);
    hinf = w.take<uint8_t>(m);
    w.round256();
    offs = w.take<uint32_t>(m + 1);
    bytes = w.bytes;
  }
};
// What a pass works on: the keys' (index 0) or the signatures' (index 1)
struct Side {
  Mirror* mirror; int xy_words, jac_words;
  uint64_t one_z[12];                                                   // Z of a handle that is affine already (everything that came from the wire)
  uint64_t* up_xy; uint32_t* up_slot; uint8_t* up_inf; uint32_t* idx;   // pinned host staging: rows to upload with their slots and identity bytes; the call's slot numbers
  uint32_t* d_idx; uint64_t* d_xy; uint8_t* d_inf;                      // the call's device lease: slot numbers, gathered rows, gathered identity bytes
};
struct HandleRef { uint32_t slot = 0; uint64_t serial = 0; const uint64_t* xyz = nullptr; };      // (null handle: serial 0)
template <class H> HandleRef handle_ref(const H* h) { return h ? HandleRef{h->slot, h->serial, h->xyz} : HandleRef{}; }

// the message hashes depend on nothing computed in the call: they run on the host cores while the GPU does the two MSMs
struct MessageHashes {
  std::vector<uint64_t> hxy; std::vector<HashJob> jobs; std::vector<uint8_t> failed; bool ok = false; std::thread hasher;
  MessageHashes(const BatchMessageFFI* batches, size_t m, bool composite, bool cip22) : hxy(m * 12), jobs(m), failed(m, 0) {
    for (size_t b = 0; b < m; b++) jobs[b] = {batches[b].data.ptr, batches[b].data.len, batches[b].extra.ptr, batches[b].extra.len, &hxy[b * 12]};
    hasher = std::thread([this, composite, cip22]() { ok = hash_many(composite, cip22, SIG_DOMAIN, jobs, &failed); });
  }
  void join() { if (hasher.joinable()) hasher.join(); }
  ~MessageHashes() { join(); }                                          // early returns must not leave it running
};

struct StrictCall {
  // Each pass runs in PHASES phases over the batch range that all workers share, and a phase stages its new rows in a region of its own
  // (the rows of the positions before it are the worst case before it): the calling thread ships a finished phase's rows while the
  // workers stage the next - what matters when many handles are new to the device (every signature of a block is; the first call of a
  // process brings 10^6 keys too)
  static constexpr size_t PHASES = 4;
  const BatchMessageFFI* const batches; const size_t m;
  std::vector<uint32_t> offs; std::vector<size_t> blen; size_t tot = 0;
  DevStage* ds = nullptr; hipStream_t copy_stream = nullptr;
  Side side[2];
  uint64_t* d_sc = nullptr; uint64_t* d_hxy = nullptr; uint8_t* d_hinf = nullptr; uint32_t* d_offs = nullptr;
  uint32_t exp_key[8];                                                  // this call's exponent stream (unit_batchverify.hip k_draw_exponents)
  unsigned nt = 1;
  std::atomic<size_t> up_n[2][PHASES];
  std::atomic<unsigned> phase_done[2][PHASES];
  std::atomic<bool> bad_handle{false};
  std::atomic<bool> work_failed{false};        // a range threw (out of memory in its vectors): the call fails, on whichever thread the range ran
  BvJob job;
  int rc_keys = 0, rc_sigs = 0;

  StrictCall(const BatchMessageFFI* b, size_t m_) : batches(b), m(m_), offs(m_ + 1, 0), blen(m_) {
    for (int q = 0; q < 2; q++) for (size_t f = 0; f < PHASES; f++) { up_n[q][f].store(0); phase_done[q][f].store(0); }
  }
  size_t phase_lo(size_t f) const { return m * f / PHASES; }
  HandleRef handle_at(int pass, size_t b, size_t i) const {
    return pass == 0 ? handle_ref(batches[b].public_keys[i]) : handle_ref(batches[b].signatures[i]);
  }

  // Step 1: the lengths and offsets of the batches; false for a length without its array
  bool size_batches() {
    for (size_t b = 0; b < m; b++) {
      // Batch::verify zips keys with signatures (batch.rs:60-64): a longer side is truncated to the shorter
      blen[b] = batches[b].public_keys_len < batches[b].signatures_len ? batches[b].public_keys_len : batches[b].signatures_len;
      if (blen[b] && (!batches[b].public_keys || !batches[b].signatures)) return false;
      offs[b + 1] = offs[b] + (uint32_t)blen[b];
    }
    tot = offs[m];
    return true;
  }

  // Step 2 (under the device's stage lock): the pinned staging, the call's device lease and the copy stream, carved into the two sides by
  // the layouts, and mirrors large enough for the call
  bool allocate(DevStage& DS, DLease& dlease) {
    ds = &DS;
    const HostLayout hl(tot);
    if (!DS.stage.reserve(hl.bytes, GrowBuf::PINNED_HOST)) { log_err("batch_verify_strict: pinned staging allocation failed"); return false; }
    const DevLayout dl(tot, m);
    uint8_t* const d_stage = dlease.take(dl.bytes);
    if (!d_stage) { log_err("batch_verify_strict: device staging allocation failed"); return false; }
    if (!DS.copy_stream && hipStreamCreateWithFlags(&DS.copy_stream, hipStreamNonBlocking) != hipSuccess) { DS.copy_stream = nullptr; return false; }
    copy_stream = DS.copy_stream;
    uint8_t* const stage = DS.stage.p;
    for (int s = 0; s < 2; s++) {
      Side& S = side[s];
      S.mirror = s == 0 ? &DS.keys : &DS.sigs;
      S.xy_words = XY_WORDS[s]; S.jac_words = JAC_WORDS[s];
      S.up_xy = (uint64_t*)(stage + hl.rows[s]); S.up_slot = (uint32_t*)(stage + hl.slots[s]); S.up_inf = stage + hl.inf[s]; S.idx = (uint32_t*)(stage + hl.idx[s]);
      S.d_idx = (uint32_t*)(d_stage + dl.idx[s]); S.d_xy = (uint64_t*)(d_stage + dl.rows[s]); S.d_inf = d_stage + dl.inf[s];
    }
    Fq2_::one().to_ark(side[0].one_z);
    Fq_::one().to_ark(side[1].one_z);
    d_sc = (uint64_t*)(d_stage + dl.sc); d_hxy = (uint64_t*)(d_stage + dl.hxy); d_hinf = d_stage + dl.hinf; d_offs = (uint32_t*)(d_stage + dl.offs);
    return grow_mirrors();
  }
  // the mirrors cover every slot THIS call's lists name (not every slot either arena has ever handed out - a process that holds
  // millions of live handles and verifies a few would pay 192 + 96 B of HBM per handle it never shows the device).  The largest slot of
  // the call is looked up only when a mirror is smaller than its arena - new handles since the last call, when rows are about to be
  // normalised and uploaded anyway; in the steady state (same validator set, epoch after epoch) the check is two comparisons.
  bool grow_mirrors() {
    uint32_t need[2] = {0, 0};
    const uint32_t hw[2] = {public_key_high_water(), signature_high_water()};
    if (hw[0] > side[0].mirror->cap || hw[1] > side[1].mirror->cap) {
      // (a destroyed or foreign handle carries serial 0 or a garbage slot - neither may size an allocation; slots the arenas never
      // handed out are ignored here and the workers fail the call with bad_handle as before; so they do for null handles)
      for (size_t b = 0; b < m; b++)
        for (size_t i = 0; i < blen[b]; i++)
          for (int s = 0; s < 2; s++) {
            const HandleRef h = handle_at(s, b, i);
            if (h.serial != 0 && h.slot < hw[s] && h.slot >= need[s]) need[s] = h.slot + 1;
          }
    }
    for (int s = 0; s < 2; s++)
      if (!side[s].mirror->grow(need[s], side[s].xy_words)) { log_err("batch_verify_strict: device mirror allocation failed"); return false; }
    return true;
  }

  // Step 3: host pass over the handles, ranges of batches across host threads, keys and then signatures (the exponents are drawn on the device,
  // from a ChaCha20 key taken from the OS-seeded master stream: bv_draw_exponents): a handle contributes its slot number; one whose
  // serial differs from the mirror's tag is claimed by exactly one thread (atomic exchange on the tag) and staged for upload - copied
  // straight if its Z is 1 (everything that came from the wire), otherwise normalised with one shared inversion per thread.
  void host_pass(unsigned t, int pass) {
   const Side& S = side[pass];
   Mirror& M = *S.mirror;
   for (size_t f = 0; f < PHASES; f++) {
    // a range never lets an exception out - the pool's workers, the fallback threads and the inline calls all run it - and always
    // counts its phase as done: the calling thread waits on that counter
    try {
    const size_t p_lo = phase_lo(f), p_hi = phase_lo(f + 1);
    const size_t b_lo = p_lo + (p_hi - p_lo) * t / nt, b_hi = p_lo + (p_hi - p_lo) * (t + 1) / nt;
    std::vector<const uint64_t*> todo;          // xyz of the handles this thread uploads
    std::vector<uint32_t> todo_slot;
    for (size_t b = b_lo; b < b_hi; b++) {
      const size_t n = blen[b], at0 = offs[b];
      for (size_t i = 0; i < n; i++) {
        HandleRef h = handle_at(pass, b, i);
        if (h.serial == 0 || h.slot >= M.cap) { bad_handle = true; h.slot = 0; }      // null, a destroyed handle, or not one of this library's
        else if (M.seen[h.slot].load(std::memory_order_relaxed) != h.serial && M.seen[h.slot].exchange(h.serial, std::memory_order_relaxed) != h.serial) {
          todo.push_back(h.xyz); todo_slot.push_back(h.slot);
        }
        S.idx[at0 + i] = h.slot;
      }
    }
    if (!todo.empty()) {
      const int A3 = S.jac_words, A2 = S.xy_words;
      const size_t base = offs[p_lo] + up_n[pass][f].fetch_add(todo.size());     // the phase's region starts at its first position
      std::vector<uint32_t> nz;                                         // not affine yet (aggregates, fresh signatures, identities)
      for (size_t k = 0; k < todo.size(); k++) {
        S.up_slot[base + k] = todo_slot[k];
        if (std::equal(S.one_z, S.one_z + (A3 - A2), todo[k] + A2)) { memcpy(S.up_xy + (base + k) * A2, todo[k], (size_t)A2 * 8); S.up_inf[base + k] = 0; }
        else nz.push_back((uint32_t)k);
      }
      if (!nz.empty()) {
        std::vector<uint64_t> jac(nz.size() * A3), xy(nz.size() * A2);
        std::vector<uint8_t> inf(nz.size());
        for (size_t k = 0; k < nz.size(); k++) memcpy(&jac[k * A3], todo[nz[k]], (size_t)A3 * 8);
        const bool is_pk = pass == 0;
        if (is_pk) batch_to_affine_range<Fq2_>(jac.data(), nz.size(), xy.data(), inf.data());
        else batch_to_affine_range<Fq_>(jac.data(), nz.size(), xy.data(), inf.data());
        for (size_t k = 0; k < nz.size(); k++) {
          memcpy(S.up_xy + (base + nz[k]) * A2, &xy[k * A2], (size_t)A2 * 8);
          S.up_inf[base + nz[k]] = inf[k];
        }
      }
    }
    } catch (...) { work_failed = true; }
    phase_done[pass][f].fetch_add(1);
   }
  }

  // Step 4: a finished phase's new rows: staging -> device -> their mirror slots (enqueued on the copy stream; the device buffer is reused
  // phase after phase in stream order)
  bool ship_phase(int pass, size_t f) {
    const Side& S = side[pass];
    const int W = S.xy_words;
    const size_t k = up_n[pass][f].load(), base = offs[phase_lo(f)];
    if (!k) return true;
    const size_t row = (size_t)W * 8, upb = k * (row + 5) + 256;
    if (upb > ds->d_up.cap && hipStreamSynchronize(copy_stream) != hipSuccess) return false;        // an earlier phase may still be reading the old buffer
    if (!ds->d_up.reserve(upb, GrowBuf::DEVICE)) return false;
    uint64_t* du_xy = (uint64_t*)ds->d_up.p;
    uint32_t* du_slot = (uint32_t*)(du_xy + k * W);
    uint8_t* du_inf = (uint8_t*)(du_slot + k);
    return hipMemcpyAsync(du_xy, S.up_xy + base * W, k * row, hipMemcpyHostToDevice, copy_stream) == hipSuccess &&
           hipMemcpyAsync(du_slot, S.up_slot + base, k * 4, hipMemcpyHostToDevice, copy_stream) == hipSuccess &&
           hipMemcpyAsync(du_inf, S.up_inf + base, k, hipMemcpyHostToDevice, copy_stream) == hipSuccess &&
           bv_mirror_scatter(W, du_xy, du_inf, du_slot, S.mirror->d_xy, S.mirror->d_inf, k, copy_stream) == 0;
  }

  // Step 5: a pass's slot numbers (and, with the keys, the offsets and the exponents) to the device, the dense arrays gathered there
  bool stage_pass(int pass) {
    const Side& S = side[pass];
    const bool is_pk = pass == 0;
    if (tot) {
      if (hipMemcpyAsync(S.d_idx, S.idx, tot * 4, hipMemcpyHostToDevice, copy_stream) != hipSuccess) return false;
      if (is_pk && (hipMemcpyAsync(d_offs, offs.data(), (m + 1) * 4, hipMemcpyHostToDevice, copy_stream) != hipSuccess ||
                    bv_draw_exponents(exp_key, d_offs, m, tot, d_sc, copy_stream) != 0)) return false;
      if (bv_mirror_gather(S.xy_words, S.mirror->d_xy, S.mirror->d_inf, S.d_idx, S.d_xy, S.d_inf, tot, copy_stream) != 0) return false;
    }
    return hipStreamSynchronize(copy_stream) == hipSuccess;
  }

  // Step 6, the mirror phase (under the device's stage lock): the workers run both host passes, and the
  // calling thread: when a pass is through, the new rows go to their mirror slots, the slot numbers (and, with the keys, the exponents)
  // cross PCIe, the GPU gathers the dense arrays, and that leg's batch MSM starts - the G2 leg (the longest of the chain) first, the
  // signatures' host pass runs under it
  // `seen` is advanced by the workers BEFORE the rows are on the device: any failure between the first claim and the last scatter drops both
  // tag sets - under the lock, at the end of the mirror phase (nothing between the first claim and there returns).
  // Returns false when rows may be missing from the mirrors or the dense arrays.
  bool mirror_phase(PhaseLog& ph) {
    bool copy_failed = false, pool_failed = false;
    {
      std::vector<std::thread> th;
      JoinAll guard{th};
      HostPool& pool = HostPool::get();
      const bool pooled = nt > 1 && pool.try_begin(nt, [&](unsigned t) { host_pass(t, 0); host_pass(t, 1); });
      PoolWait pool_wait{pool, pooled, pool_failed};
      if (!pooled) {
        if (nt > 1) {
          try { for (unsigned t = 0; t < nt; t++) th.emplace_back([&, t]() { host_pass(t, 0); host_pass(t, 1); }); }
          catch (...) { for (unsigned t = (unsigned)th.size(); t < nt; t++) { host_pass(t, 0); host_pass(t, 1); } }   // no more threads: the rest of the ranges here
        } else { host_pass(0, 0); host_pass(0, 1); }
      }
      for (int pass = 0; pass < 2 && !copy_failed; pass++) {
        for (size_t f = 0; f < PHASES; f++) {
          while (phase_done[pass][f].load() < nt) std::this_thread::yield();
          if (bad_handle || work_failed || !ship_phase(pass, f)) { copy_failed = true; break; }
        }
        if (copy_failed) break;
        ph.mark(pass == 0 ? "  host pass over the key handles" : "  host pass over the signature handles");
        if (bad_handle || !stage_pass(pass)) { copy_failed = true; break; }
        ph.mark("  rows / slots across, gathered on the device");
        if (pass == 0) { rc_keys = bv_begin_keys(&job, side[0].d_xy, side[0].d_inf, d_sc, 1, offs.data(), m); ph.mark("key slots + exponents across, G2 batch MSM started"); }
        else { rc_sigs = bv_begin_sigs(&job, side[1].d_xy, side[1].d_inf, d_sc, 1, offs.data(), m); ph.mark("signature slots across, G1 batch MSM started"); }
      }
    }
    if (pool_failed || work_failed) copy_failed = true;                   // a range threw (out of memory): rows may be missing
    if (copy_failed) {
      side[0].mirror->forget(); side[1].mirror->forget();
      (void)hipStreamSynchronize(copy_stream);      //  copies and scatters of the phases shipped before the failure may still be queued on the shared
                                                    // stream, reading the shared pinned stage and d_up: they end before the next call on this device may stage
    }
    return !copy_failed;
  }

  // Step 7: the hash points follow the MSM results to the device and the chained pairing checks give the verdicts.  bv_finish is called
  // after a failed begin too: it releases the engines either way.
  bool finish(PhaseLog& ph, MessageHashes& mh, bool mirrored, bool* out_results) {
    mh.join();
    ph.mark("  message hashes joined");
    std::vector<uint8_t> hinf(m, 0), ok(m, 0);
    if (mh.ok) for (size_t b = 0; b < m; b++) if (mh.failed[b]) hinf[b] = 1;   // no H(m): that pair is left out, the verdict is forced below
    uint64_t ng2[24];
    neg_g2_generator(ng2);
    const bool staged = mh.ok && mirrored && rc_keys == 0 && rc_sigs == 0 &&
                        hipMemcpyAsync(d_hxy, mh.hxy.data(), m * 96, hipMemcpyHostToDevice, copy_stream) == hipSuccess &&
                        hipMemcpyAsync(d_hinf, hinf.data(), m, hipMemcpyHostToDevice, copy_stream) == hipSuccess &&
                        hipStreamSynchronize(copy_stream) == hipSuccess;
    ph.mark("  hashes across");
    if (bv_finish(&job, staged ? 1 : 0, d_hxy, d_hinf, 1, ng2, m, ok.data()) != 0 || !staged) return false;
    ph.mark("pairs -> pairing checks (GPU, chained)");
    bool all = true;
    for (size_t b = 0; b < m; b++) { out_results[b] = ok[b] != 0 && !mh.failed[b]; all = all && out_results[b]; }
    ph.mark("results");
    return all;
  }
};
}  // namespace

extern "C" {

// Signature::batch_verify (crates/bls-crypto/src/bls/signature.rs:101-155): aggregate the signatures, hash every message,
// ONE (n+1)-pair product on the GPU
bool batch_verify_signature(const MessageFFI* messages, size_t n, bool composite, bool cip22, bool* verified) {       /* signatures.rs:290 */
  if (!hash_flags_supported(composite, cip22) || (!messages && n) || !verified) return false;
  std::vector<uint64_t> sigs(n * 18), pkj(n * 36);
  for (size_t i = 0; i < n; i++) {
    if (!messages[i].public_key || !messages[i].sig) return false;
    memcpy(&sigs[i * 18], messages[i].sig->xyz, 144);
    memcpy(&pkj[i * 36], messages[i].public_key->xyz, 288);
  }
  uint64_t asig[18];
  if (celo_amd_sum_jacobian_bls12_377_g1(sigs.data(), n, asig) != 0) return false;
  std::vector<uint64_t> g1((n + 1) * 12), g2((n + 1) * 24);
  std::vector<uint8_t> i1(n + 1, 0), i2(n + 1, 0);
  batch_to_affine<Fq_>(asig, 1, g1.data(), i1.data());
  neg_g2_generator(g2.data());
  batch_to_affine<Fq2_>(pkj.data(), n, g2.data() + 24, i2.data() + 1);
  std::vector<HashJob> jobs(n);
  for (size_t i = 0; i < n; i++) jobs[i] = {messages[i].data.ptr, messages[i].data.len, messages[i].extra.ptr, messages[i].extra.len, &g1[(i + 1) * 12]};
  if (n && !hash_many(composite, cip22, SIG_DOMAIN, jobs)) { *verified = false; return true; }   // a message that does not hash: not verified, not an error
  int one = 0;
  if (pairing_product_is_one_bls12_377(g1.data(), i1.data(), g2.data(), i2.data(), n + 1, &one) != 0) return false;
  *verified = one != 0;
  return true;
}
// Batch::verify per batch (crates/bls-crypto/src/bls/batch.rs:44-84), all batches at once: random exponents from the OS
// RNG, all G2 MSMs in one call, all G1 MSMs in one call, all 2-pair checks in one call.  out_results is always filled;
// the return value is false if any batch fails (signatures.rs:392-400).
bool batch_verify_strict(const BatchMessageFFI* batches, size_t m, bool composite, bool cip22, bool* out_results) {   /* signatures.rs:343 */
  if ((!batches && m) || !out_results) return false;
  PhaseLog ph("batch_verify_strict");
  for (size_t i = 0; i < m; i++) out_results[i] = false;      // always filled: every early return below leaves "not verified"
  if (!composite && cip22) return false;                      // per-batch false (signatures.rs:387)
  if (m == 0) return true;
  StrictCall call(batches, m);
  if (!call.size_batches()) return false;                     // a length without its array
  if (api_enter() != 0) return false;
  DevStage& DS = dev_stage(api_device());
  DLease dlease(DS);                       // (declared before the lock: released after everything below, when bv_finish has drained the GPU work)
  std::unique_lock<std::mutex> stage_lk(DS.mu);
  if (!call.allocate(DS, dlease)) return false;
  ChaCha20Rng master;
  if (!os_seeded_rng(master)) { log_err("batch_verify_strict: no OS randomness"); return false; }
  ph.mark("validate + allocate");
  MessageHashes hashes(batches, m, composite, cip22);         // (joined on every path: by finish(), or by its destructor)
  unsigned nt = std::thread::hardware_concurrency();
  if (nt > 64) nt = 64;
  if (nt < 1 || call.tot < 8192) nt = 1;
  call.nt = nt;
  for (int k = 0; k < 8; k++) call.exp_key[k] = master.next_u32();
  const bool mirrored = call.mirror_phase(ph);
  stage_lk.unlock();                                          // end of the mirror phase: the next call on this device may stage while this one computes
  if (call.bad_handle) log_err("batch_verify_strict: a destroyed or foreign handle in the batch lists");
  return call.finish(ph, hashes, mirrored, out_results);
}
}
