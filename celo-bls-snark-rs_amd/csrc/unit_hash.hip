// Translation unit: batched hash-to-G1 and hash-to-G2 (see hash_direct.h): rounds of candidate counters, then the cofactor ladder.  The two
// groups have kernels of their own and share the round loop (hash_rounds), the scratch, the stream and the mutex.
#include "hash_direct.h"
#include "pedersen.h"
#include <hip/hip_runtime.h>
#include <atomic>
#include <mutex>
#include <vector>
#include <cstring>
#include <cstdio>

#include "runtime.h"
#include "units.h"
// two waves per SIMD (scratch instead of AGPRs for what does not fit 256 VGPRs) unless overridden: -DFROW_OCC= for the A/B
#ifndef FROW_OCC
#define FROW_OCC __attribute__((amdgpu_waves_per_eu(2, 2)))
#endif
namespace celo {
static std::mutex hash_mu;                 // bulk calls, serialised per process; guards the per-device scratch, its stream and the generator tables' device copies

struct HashDom { uint8_t b[8]; };
struct HashIn { const uint8_t* msgs; const uint64_t* msg_off; const uint8_t* extras; const uint64_t* extra_off; };

// One round of try-and-increment for the messages still without a point.  list: their indices (nullptr = all of 0..count);
// each gets CAND adjacent lanes trying the counters base .. base + CAND - 1 side by side (CAND = 1, 2, ... 64 divides the wave:
// many messages -> 1, so every lane's square root is one the serial loop would also have computed; few messages -> up to 16,
// so a round finds a point with probability 1 - 0.58^16 and the call is two launches deep instead of eight).  The lowest
// successful counter of the group wins (ballot), its lane stores the curve point BEFORE the cofactor; a group without success
// appends its message to the next round's list.
__global__ void __launch_bounds__(64) FROW_OCC
k_hash_candidates(HashDom dom, HashIn in, const uint32_t* __restrict__ list, uint32_t count, uint32_t cand_log, uint32_t base, int mode, const EdPoint* __restrict__ gens,
                  uint64_t* __restrict__ cand_xy, uint8_t* __restrict__ attempts, uint32_t* __restrict__ next_list, uint32_t* __restrict__ next_count,
                  WireConsts k) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t j = t >> cand_log, s = t & ((1u << cand_log) - 1);
  const bool live = j < count;
  const uint32_t i = live ? (list ? list[j] : j) : 0;
  const uint32_t c = base + s;
  bool ok = false;
  Affine<Fq> p = {Fq::zero(), Fq::zero()};
  if (live && c < 255) {
    const uint8_t* msg = in.msgs + in.msg_off[i];
    const size_t mlen = (size_t)(in.msg_off[i + 1] - in.msg_off[i]);
    const uint8_t* extra = in.extra_off ? in.extras + in.extra_off[i] : nullptr;
    const size_t elen = in.extra_off ? (size_t)(in.extra_off[i + 1] - in.extra_off[i]) : 0;
    ok = tai_candidate(dom.b, msg, mlen, extra, elen, (int)c, k, p, mode, gens);
  }
  const uint64_t mask = __ballot(ok);
  const uint32_t lane = threadIdx.x & 63, g0 = lane & ~((1u << cand_log) - 1);
  const uint64_t gm = (mask >> g0) & (cand_log == 6 ? ~0ull : ((1ull << (1u << cand_log)) - 1));
  if (!live) return;
  if (gm) {
    const uint32_t win = (uint32_t)__builtin_ctzll(gm);
    if (s == win) {
      uint64_t* o = cand_xy + (size_t)i * 12;
      p.x.to_ark(o);
      p.y.to_ark(o + 6);
      attempts[i] = (uint8_t)c;
    }
  } else if (s == 0) {
    if (base + (1u << cand_log) >= 255) attempts[i] = 255;                // every counter tried: the reference errs
    else next_list[atomicAdd(next_count, 1u)] = i;
  }
}
// scale_by_cofactor + normalisation of the winning candidates, one message per lane (uniform: a 124-step ladder and one
// inversion).  A multiple that is the identity (probability ~2^-125 per message) is flagged for the host's serial loop.
__global__ void __launch_bounds__(64) FROW_OCC
k_hash_finish(const uint64_t* __restrict__ cand_xy, const uint8_t* __restrict__ attempts, uint64_t* __restrict__ out, uint8_t* __restrict__ redo, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t* o = out + (size_t)i * 12;
  redo[i] = 0;
  if (attempts[i] == 255) { for (int j = 0; j < 12; j++) o[j] = 0; return; }
  const uint64_t* ci = cand_xy + (size_t)i * 12;
  const Affine<Fq> p = {Fq::norm(Fq::from_ark(ci)), Fq::norm(Fq::from_ark(ci + 6))};
  Affine<Fq> r = {Fq::zero(), Fq::zero()};
  if (tai_finish(p, r)) { r.x.to_ark(o); r.y.to_ark(o + 6); }
  else { redo[i] = 1; for (int j = 0; j < 12; j++) o[j] = 0; }
}

// ---- the same two kernels for G2: candidates are points of the twist over Fq2 (three XOF blocks, an Fq2 root: hash_direct.h
// tai_candidate_g2), rows are 24 limbs (x.c0, x.c1, y.c0, y.c1: the layout of msm_bls12_377_g2's bases), the cofactor ladder has 501 steps.
// Siblings, not instantiations of one template: the G1 kernels stay the source they were measured as.
__global__ void __launch_bounds__(64) FROW_OCC
k_hash_candidates_g2(HashDom dom, HashIn in, const uint32_t* __restrict__ list, uint32_t count, uint32_t cand_log, uint32_t base, int mode, int compat,
                     const EdPoint* __restrict__ gens, uint64_t* __restrict__ cand_xy, uint8_t* __restrict__ attempts, uint32_t* __restrict__ next_list,
                     uint32_t* __restrict__ next_count, WireConsts k) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t j = t >> cand_log, s = t & ((1u << cand_log) - 1);
  const bool live = j < count;
  const uint32_t i = live ? (list ? list[j] : j) : 0;
  const uint32_t c = base + s;
  bool ok = false;
  Affine<Fq2> p = {Fq2::zero(), Fq2::zero()};
  if (live && c < 255) {
    const uint8_t* msg = in.msgs + in.msg_off[i];
    const size_t mlen = (size_t)(in.msg_off[i + 1] - in.msg_off[i]);
    const uint8_t* extra = in.extra_off ? in.extras + in.extra_off[i] : nullptr;
    const size_t elen = in.extra_off ? (size_t)(in.extra_off[i + 1] - in.extra_off[i]) : 0;
    ok = tai_candidate_g2(dom.b, msg, mlen, extra, elen, (int)c, compat, k, p, mode, gens);
  }
  const uint64_t mask = __ballot(ok);
  const uint32_t lane = threadIdx.x & 63, g0 = lane & ~((1u << cand_log) - 1);
  const uint64_t gm = (mask >> g0) & (cand_log == 6 ? ~0ull : ((1ull << (1u << cand_log)) - 1));
  if (!live) return;
  if (gm) {
    const uint32_t win = (uint32_t)__builtin_ctzll(gm);
    if (s == win) {
      uint64_t* o = cand_xy + (size_t)i * 24;
      p.x.to_ark(o);
      p.y.to_ark(o + 12);
      attempts[i] = (uint8_t)c;
    }
  } else if (s == 0) {
    if (base + (1u << cand_log) >= 255) attempts[i] = 255;                // every counter tried: the reference errs
    else next_list[atomicAdd(next_count, 1u)] = i;
  }
}
__global__ void __launch_bounds__(64) FROW_OCC
k_hash_finish_g2(const uint64_t* __restrict__ cand_xy, const uint8_t* __restrict__ attempts, uint64_t* __restrict__ out, uint8_t* __restrict__ redo, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t* o = out + (size_t)i * 24;
  redo[i] = 0;
  if (attempts[i] == 255) { for (int j = 0; j < 24; j++) o[j] = 0; return; }
  const uint64_t* ci = cand_xy + (size_t)i * 24;
  const Affine<Fq2> p = {Fq2::norm(Fq2::from_ark(ci)), Fq2::norm(Fq2::from_ark(ci + 12))};
  Affine<Fq2> r = {Fq2::zero(), Fq2::zero()};
  if (tai_finish_g2(p, r)) { r.x.to_ark(o); r.y.to_ark(o + 12); }
  else { redo[i] = 1; for (int j = 0; j < 24; j++) o[j] = 0; }
}

// celo_composite_gens (seam_hash.hip): the generator table, built once from the ChaCha20 stream of the reference
static EdPoint* g_d_gens_dev[MAX_DEVICES] = {};      // its device copies (11.7 MB each), uploaded on first use (under hash_mu)
#define g_d_gens g_d_gens_dev[api_device()]
static int ensure_device_gens(const EdPoint* h_gens, size_t ngens) {
  if (g_d_gens) return 0;
  if (hipMalloc(&g_d_gens, ngens * sizeof(EdPoint)) != hipSuccess) { g_d_gens = nullptr; return 10; }
  if (hipMemcpy(g_d_gens, h_gens, ngens * sizeof(EdPoint), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(g_d_gens); g_d_gens = nullptr; return 10; }
  return 0;
}
// Device scratch and stream of the bulk hashers, per device, grow-only (under hash_mu).  Round 4: the calls used to hipMalloc / hipFree
// eight buffers and run on the null stream - inside batch_verify_strict, whose hashing thread runs BESIDE the two batch MSMs, the null
// stream's implicit joins and hipFree's device-wide wait held the hashes back until the MSMs had drained (hashes joined at 23.5 of
// 29.9 ms) and the pairing leg was enqueued only then.  A non-blocking stream of their own and one cached allocation: they finish
// under the G2 accumulation.
struct HashScratch { hipStream_t stream = nullptr; uint8_t* buf = nullptr; size_t cap = 0; };
static HashScratch g_hash_scratch[MAX_DEVICES];
// keep: bytes at the head of the scratch that outlive a growth (the CRH rows of a CIP22 call, between its two steps; the step that wrote
// them has drained)
static int hash_scratch(size_t need, HashScratch** out, size_t keep = 0) {
  HashScratch& h = g_hash_scratch[api_device()];
  if (!h.stream && hipStreamCreateWithFlags(&h.stream, hipStreamNonBlocking) != hipSuccess) { h.stream = nullptr; return 10; }
  if (need > h.cap) {
    uint8_t* old = keep ? h.buf : nullptr;
    if (h.buf && !old) (void)hipFree(h.buf);
    h.buf = nullptr; h.cap = 0;
    if (hipMalloc((void**)&h.buf, need + need / 4) != hipSuccess) { h.buf = nullptr; if (old) (void)hipFree(old); return 10; }
    h.cap = need + need / 4;
    if (old) {
      const hipError_t e = hipMemcpy(h.buf, old, keep, hipMemcpyDeviceToDevice);
      (void)hipFree(old);
      if (e != hipSuccess) return 10;
    }
  }
  *out = &h;
  return 0;
}
// Where a call's operands live.  msgs / rest: the message bytes / the extras, rows and attempts are DEVICE pointers (the _dev entries set both; the
// second step of a CIP22 call reads its messages, the CRH rows, at the head of the scratch in either form).  stream: the caller's, with rest.
// head: bytes at the start of the scratch that the call leaves alone.
// at_head: the messages ARE the head of the scratch (the `msgs` argument is not used).  kernel_ms (optional): receives what the step notes as its time.
struct HashWhere { bool msgs = false, rest = false, at_head = false; hipStream_t stream = nullptr; size_t head = 0; float* kernel_ms = nullptr; };
// the kernel ms of the last round loop or CRH that succeeded (a CIP22 composite call runs both: its CRH's time is overwritten by the loop's, so
// such a call reports its tail alone), the rounds of the last loop, the width of the last CRH kernel (celo_amd_crh_last_lanes)
struct HashLast { float ms = 0.f; int rounds = 0, crh_lanes = 0; };
static Last<HashLast> g_hash_last;
static std::atomic<int> g_crh_lanes{0};         // 0 = the rule (crh_pick_lanes), else 1, 2, 4, .. 256 (celo_amd_crh_set_lanes)

static Last<CallTimes> g_hash_g2_last;          // the last G2 call's [0] candidate rounds, [1] finish kernel
static std::atomic<int> g_g2_budget_log{17};    // celo_amd_hash_g2_set_lane_budget_log

// What differs between the groups: the row width, the two kernels, the serial loop, the lane budget.  compat reaches only G2.
struct HashG1 {
  static constexpr int ROW = 12;
  static int budget_log() { return 17; }
  static void candidates(dim3 grid, hipStream_t st, const HashDom& dom, const HashIn& in, const uint32_t* list, uint32_t count, uint32_t cand_log, uint32_t base, int mode,
                         int, const EdPoint* gens, uint64_t* cand, uint8_t* att, uint32_t* next, uint32_t* cnt, const WireConsts& k) {
    hipLaunchKernelGGL(k_hash_candidates, grid, dim3(64), 0, st, dom, in, list, count, cand_log, base, mode, gens, cand, att, next, cnt, k);
  }
  static void finish(dim3 grid, hipStream_t st, const uint64_t* cand, const uint8_t* att, uint64_t* out, uint8_t* redo, uint32_t n) {
    hipLaunchKernelGGL(k_hash_finish, grid, dim3(64), 0, st, cand, att, out, redo, n);
  }
  static bool serial(const uint8_t* dom, const uint8_t* msg, size_t mlen, const uint8_t* extra, size_t elen, int, const WireConsts& kh, uint64_t* o, int& c, int c_start,
                     int mode, const EdPoint* gens) {
    Affine<Fq> p = {Fq::zero(), Fq::zero()};
    if (!hash_to_g1_direct_tai(dom, msg, mlen, extra, elen, kh, p, c, c_start, mode, gens)) return false;
    p.x.to_ark(o); p.y.to_ark(o + 6);
    return true;
  }
};
struct HashG2 {
  static constexpr int ROW = 24;
  static int budget_log() { return g_g2_budget_log.load(); }
  static void candidates(dim3 grid, hipStream_t st, const HashDom& dom, const HashIn& in, const uint32_t* list, uint32_t count, uint32_t cand_log, uint32_t base, int mode,
                         int compat, const EdPoint* gens, uint64_t* cand, uint8_t* att, uint32_t* next, uint32_t* cnt, const WireConsts& k) {
    hipLaunchKernelGGL(k_hash_candidates_g2, grid, dim3(64), 0, st, dom, in, list, count, cand_log, base, mode, compat, gens, cand, att, next, cnt, k);
  }
  static void finish(dim3 grid, hipStream_t st, const uint64_t* cand, const uint8_t* att, uint64_t* out, uint8_t* redo, uint32_t n) {
    hipLaunchKernelGGL(k_hash_finish_g2, grid, dim3(64), 0, st, cand, att, out, redo, n);
  }
  static bool serial(const uint8_t* dom, const uint8_t* msg, size_t mlen, const uint8_t* extra, size_t elen, int compat, const WireConsts& kh, uint64_t* o, int& c,
                     int c_start, int mode, const EdPoint* gens) {
    Affine<Fq2> p = {Fq2::zero(), Fq2::zero()};
    if (!hash_to_g2_tai(dom, msg, mlen, extra, elen, compat, kh, p, c, c_start, mode, gens)) return false;
    p.x.to_ark(o); p.y.to_ark(o + 12);
    return true;
  }
};

// The round loop of both groups, under hash_mu.  split: the G2 record of the candidate rounds and the finish kernel is noted too.
template <class G>
static int hash_rounds_locked(const uint8_t* domain, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* extras, const uint64_t* extra_off, size_t n, int compat,
                              uint64_t* out_xy, uint8_t* attempts, int mode, bool split, const EdPoint* h_gens, size_t ngens, const HashWhere& w) {
  constexpr int ROW = G::ROW;
  if (n == 0) return 0;
  if (mode == TAI_COMPOSITE) {
    if (int rcg = ensure_device_gens(h_gens, ngens)) return rcg;
    for (size_t i = 0; i < n; i++)   // counter || extra || message must fit the generator table (the reference panics)
      if ((1 + (msg_off ? msg_off[i + 1] - msg_off[i] : 0) + (extra_off ? extra_off[i + 1] - extra_off[i] : 0)) * 8 > PEDERSEN_MAX_BITS) return 2;
  }
  const EdPoint* d_gens = mode == TAI_COMPOSITE ? g_d_gens : nullptr;
  if (!domain || !msg_off || !out_xy || !attempts || n > 0x3fffffffu) return 2;
  for (size_t i = 0; i < n; i++) {
    if (msg_off[i + 1] < msg_off[i] || (extra_off && extra_off[i + 1] < extra_off[i])) return 2;
  }
  const size_t mb = msg_off[n], eb = extra_off ? extra_off[n] : 0;
  if ((mb && !msgs && !w.at_head) || (eb && !extras)) return 2;
  const bool dev_msgs = w.msgs || w.at_head;
  const WireConsts& kh = wire_consts();   // host tables (the serial fallback below)
  WireConsts k;
  if (int rck = wire_consts_device(k)) return rck;
  HashDom dom;
  memcpy(dom.b, domain, 8);
  std::vector<uint8_t> redo(n);
  // what the caller holds on the device is used where it lies; the rest takes a slice of the scratch
  size_t off = w.head;
  auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~size_t(255); return o; };
  const size_t o_off = take((n + 1) * 2 * 8), o_out = take(w.rest ? 0 : n * ROW * 8), o_cand = take(n * ROW * 8), o_list = take(2 * n * 4), o_cnt = take(256 * 4),
               o_att = take(w.rest ? 0 : n), o_redo = take(n), o_msgs = take(dev_msgs ? 0 : mb + 8), o_extras = take(w.rest ? 0 : eb + 8);
  HashScratch* hs = nullptr;
  if (hash_scratch(off, &hs, w.head)) return 10;
  CallScope cs(w.rest ? w.stream : hs->stream);   // the scratch and its stream stay with the device; the call owns its events
  const hipStream_t st = cs.stream();
  uint64_t *d_off = (uint64_t*)(hs->buf + o_off), *d_out = w.rest ? out_xy : (uint64_t*)(hs->buf + o_out), *d_cand = (uint64_t*)(hs->buf + o_cand);
  uint32_t *d_list = (uint32_t*)(hs->buf + o_list), *d_cnt = (uint32_t*)(hs->buf + o_cnt);
  uint8_t *d_att = w.rest ? attempts : hs->buf + o_att, *d_redo = hs->buf + o_redo;
  const uint8_t *d_msgs = w.at_head ? hs->buf : w.msgs ? msgs : hs->buf + o_msgs, *d_extras = w.rest ? extras : hs->buf + o_extras;
  if (mb && !dev_msgs) HIP_TRY(hipMemcpyAsync(hs->buf + o_msgs, msgs, mb, hipMemcpyHostToDevice, st), 10);
  if (eb && !w.rest) HIP_TRY(hipMemcpyAsync(hs->buf + o_extras, extras, eb, hipMemcpyHostToDevice, st), 10);
  HIP_TRY(hipMemcpyAsync(d_off, msg_off, (n + 1) * 8, hipMemcpyHostToDevice, st), 10);
  if (extra_off) HIP_TRY(hipMemcpyAsync(d_off + n + 1, extra_off, (n + 1) * 8, hipMemcpyHostToDevice, st), 10);
  HIP_TRY(hipMemsetAsync(d_cnt, 0, 256 * 4, st), 10);
  hipEvent_t e0, e1, em = nullptr;
  HIP_TRY(cs.event(&e0), 10);
  HIP_TRY(cs.event(&e1), 10);
  if (split) HIP_TRY(cs.event(&em), 10);
  HIP_TRY(hipEventRecord(e0, st), 10);
  const HashIn in = {d_msgs, d_off, d_extras, extra_off ? d_off + n + 1 : nullptr};
  const size_t budget = size_t(1) << G::budget_log();
  uint32_t count = (uint32_t)n, base = 0;
  int round = 0;
  while (count && base < 255) {
    uint32_t cand_log = 0;
    while (cand_log < 4 && ((size_t)count << (cand_log + 1)) <= budget) cand_log++;     // fill the lane budget (2^17), at most 16 counters
    const uint32_t* list = round ? d_list + (size_t)(round & 1) * n : nullptr;
    uint32_t* next = d_list + (size_t)((round + 1) & 1) * n;
    const size_t lanes = (size_t)count << cand_log;
    G::candidates(dim3((uint32_t)((lanes + 63) / 64)), st, dom, in, list, count, cand_log, base, mode, compat, d_gens, d_cand, d_att, next, d_cnt + round, k);
    HIP_TRY(hipGetLastError(), 10);
    HIP_TRY(hipMemcpyAsync(&count, d_cnt + round, 4, hipMemcpyDeviceToHost, st), 10);
    HIP_TRY(hipStreamSynchronize(st), 10);
    base += 1u << cand_log;
    round++;
  }
  if (split) HIP_TRY(hipEventRecord(em, st), 10);
  G::finish(dim3(((uint32_t)n + 63) / 64), st, d_cand, d_att, d_out, d_redo, (uint32_t)n);
  HIP_TRY(hipGetLastError(), 10);
  HIP_TRY(hipEventRecord(e1, st), 10);
  if (!w.rest) {
    HIP_TRY(hipMemcpyAsync(out_xy, d_out, n * ROW * 8, hipMemcpyDeviceToHost, st), 10);
    HIP_TRY(hipMemcpyAsync(attempts, d_att, n, hipMemcpyDeviceToHost, st), 10);
  }
  HIP_TRY(hipMemcpyAsync(redo.data(), d_redo, n, hipMemcpyDeviceToHost, st), 10);
  HIP_TRY(hipStreamSynchronize(st), 10);
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, e0, e1), 10);
  g_hash_last.update([&](HashLast& r) { r.ms = ms; r.rounds = round; });
  if (w.kernel_ms) *w.kernel_ms = ms;
  if (split) {
    CallTimes sp;
    HIP_TRY(hipEventElapsedTime(&sp.ms[0], e0, em), 10);
    HIP_TRY(hipEventElapsedTime(&sp.ms[1], em, e1), 10);
    g_hash_g2_last.note(sp);
  }
  // the counter whose cofactor multiple was the identity is skipped like the reference's loop does: continue serially after it.  What lies on
  // the device is fetched for the flagged row alone, and the row and its counter go back where the caller reads them.
  for (size_t i = 0; i < n; i++) {
    if (!redo[i]) continue;
    const size_t mlen = msg_off[i + 1] - msg_off[i], elen = extra_off ? extra_off[i + 1] - extra_off[i] : 0;
    std::vector<uint8_t> hm, he;
    const uint8_t *m = (dev_msgs ? d_msgs : msgs) + msg_off[i], *e = extra_off ? extras + extra_off[i] : nullptr;
    if (dev_msgs && mlen) { hm.resize(mlen); HIP_TRY(hipMemcpy(hm.data(), m, mlen, hipMemcpyDeviceToHost), 10); m = hm.data(); }
    if (w.rest && elen) { he.resize(elen); HIP_TRY(hipMemcpy(he.data(), e, elen, hipMemcpyDeviceToHost), 10); e = he.data(); }
    uint64_t row[ROW];
    uint8_t att = 255;
    if (w.rest) HIP_TRY(hipMemcpy(&att, attempts + i, 1, hipMemcpyDeviceToHost), 10);
    else att = attempts[i];
    int c = 255;
    if (G::serial(domain, m, mlen, e, elen, compat, kh, row, c, att + 1, mode, h_gens)) att = (uint8_t)c;
    else { att = 255; memset(row, 0, sizeof row); }
    if (w.rest) {
      HIP_TRY(hipMemcpy(out_xy + i * ROW, row, sizeof row, hipMemcpyHostToDevice), 10);
      HIP_TRY(hipMemcpy(attempts + i, &att, 1, hipMemcpyHostToDevice), 10);
    } else {
      memcpy(out_xy + i * ROW, row, sizeof row);
      attempts[i] = att;
    }
  }
  return 0;
}
static int pedersen_crh_locked(const uint8_t* msgs, const uint64_t* msg_off, size_t n, uint8_t* out48, const EdPoint* gens, size_t ngens, const HashWhere& w, bool out_at_head);
// The hash step of a protocol mode (units.h): the round loop in the caller's mode, or for CIP22 (mode 3) one CRH per message and then the
// loops over xof(c || extra || inner) - kernel_ms is then the loops' time alone, as the record's
template <class G>
static int hash_step(const uint8_t* domain, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* extras, const uint64_t* extra_off, size_t n, int compat,
                     uint64_t* out_xy, uint8_t* attempts, int mode, bool split, int dev = 0, void* stream = nullptr, float* kernel_ms = nullptr) {
  HashWhere w;
  w.msgs = w.rest = dev != 0;
  w.stream = (hipStream_t)stream;
  w.kernel_ms = kernel_ms;
  if (mode != 3) {
    size_t ngens = 0;
    const EdPoint* h_gens = mode == TAI_COMPOSITE ? celo_composite_gens(&ngens) : nullptr;   // before the lock: 0.5 s on first use
    if (int rc0 = api_enter()) return rc0;
    std::lock_guard<std::mutex> lk(hash_mu);
    return hash_rounds_locked<G>(domain, msgs, msg_off, extras, extra_off, n, compat, out_xy, attempts, mode, split, h_gens, ngens, w);
  }
  if (n == 0) return 0;
  if (!msg_off) return 2;
  size_t ngens = 0;
  const EdPoint* h_gens = celo_composite_gens(&ngens);
  if (int rc0 = api_enter()) return rc0;
  std::lock_guard<std::mutex> lk(hash_mu);
  // the CRH rows stay on the device: the CRH kernel writes them at the head of the scratch, where the round loop reads them as its messages
  std::vector<uint64_t> ioff(n + 1);
  for (size_t i = 0; i <= n; i++) ioff[i] = 48 * i;
  HashWhere wc = w;
  wc.head = (n * 48 + 255) & ~size_t(255);
  if (int rc = pedersen_crh_locked(msgs, msg_off, n, nullptr, h_gens, ngens, wc, true)) return rc;
  wc.at_head = true;
  return hash_rounds_locked<G>(domain, nullptr, ioff.data(), extras, extra_off, n, compat, out_xy, attempts, 1, split, nullptr, 0, wc);
}
int hash_to_g1_direct_run(const uint8_t* domain, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* extras, const uint64_t* extra_off,
                          size_t n, uint64_t* out_xy, uint8_t* attempts, int mode, int dev, void* stream, float* kernel_ms) {
  return hash_step<HashG1>(domain, msgs, msg_off, extras, extra_off, n, 0, out_xy, attempts, mode, false, dev, stream, kernel_ms);
}
int hash_to_g2_run(const uint8_t* domain, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* extras, const uint64_t* extra_off, size_t n, int compat,
                   uint64_t* out_xy, uint8_t* attempts, int mode) {
  if (compat != 0 && compat != 1) return 2;
  return hash_step<HashG2>(domain, msgs, msg_off, extras, extra_off, n, compat, out_xy, attempts, mode, true);
}
// one message on the host, no device touched: mode 0 direct, 1 the CIP22 tail (`msg` is the inner CRH), 2 composite, 3 composite CIP22
int hash_to_g2_one_run(const uint8_t* domain, const uint8_t* msg, size_t mlen, const uint8_t* extra, size_t elen, int mode, int compat, uint64_t* out_xy, int* attempt) {
  if (!domain || !out_xy || !attempt || (mlen && !msg) || (elen && !extra) || mode < 0 || mode > 3 || (compat != 0 && compat != 1)) return 2;
  size_t ngens = 0;
  const EdPoint* gens = mode >= 2 ? celo_composite_gens(&ngens) : nullptr;
  uint8_t inner[48];
  if (mode == 3) {
    if (mlen * 8 > PEDERSEN_MAX_BITS) return 2;
    pedersen_crh(gens, msg, mlen, inner);
    msg = inner;
    mlen = 48;
  } else if (mode == 2 && (1 + mlen + elen) * 8 > PEDERSEN_MAX_BITS) return 2;
  int c = 255;
  *attempt = 255;
  memset(out_xy, 0, 24 * 8);
  if (!HashG2::serial(domain, msg, mlen, extra, elen, compat, wire_consts(), out_xy, c, 0, mode == 0 ? TAI_DIRECT : mode == 2 ? TAI_COMPOSITE : TAI_XOF_ONLY, gens)) return 0;
  *attempt = c;
  return 0;
}
int hash_g2_set_lane_budget_log(int log) {
  if (log < 4 || log > 17) return 2;
  g_g2_budget_log.store(log);
  return 0;
}
void hash_g2_last_split(float ms[2]) { const CallTimes sp = g_hash_g2_last.read(); ms[0] = sp.ms[0]; ms[1] = sp.ms[1]; }
// ---- bulk Pedersen CRH (pedersen.h): one message per lane; the 52080-generator table (11.7 MB) is uploaded on first use
__global__ void __launch_bounds__(64) FROW_OCC
k_pedersen_crh(const EdPoint* __restrict__ gens, const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ off, uint8_t* __restrict__ out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint8_t h[48];
  pedersen_crh(gens, msgs + off[i], (size_t)(off[i + 1] - off[i]), h);
  for (int j = 0; j < 48; j++) out[(size_t)i * 48 + j] = h[j];
}
// (the many-lane form, k_pedersen_crh_lanes, is a unit of its own, unit_hash_lanes.hip: in this unit's code object it cost k_pedersen_crh 4 % at
// 65 536 x 127 B)

// under hash_mu.  out_at_head: the rows stay at the head of the scratch (w.head bytes; out48 is not used)
static int pedersen_crh_locked(const uint8_t* msgs, const uint64_t* msg_off, size_t n, uint8_t* out48, const EdPoint* gens, size_t ngens, const HashWhere& w, bool out_at_head) {
  if (n == 0) return 0;
  if (!msg_off || (!out48 && !out_at_head) || n > 0x7fffffffu) return 2;
  size_t max_len = 0;
  for (size_t i = 0; i < n; i++) {
    if (msg_off[i + 1] < msg_off[i] || (msg_off[i + 1] - msg_off[i]) * 8 > PEDERSEN_MAX_BITS) return 2;   // the reference panics on longer messages
    if (msg_off[i + 1] - msg_off[i] > max_len) max_len = msg_off[i + 1] - msg_off[i];
  }
  const uint32_t L = crh_pick_lanes((uint32_t)g_crh_lanes.load(), (max_len * 8 + 2) / 3, n);   // one width per call, from the longest message
  const size_t mb = msg_off[n];
  if (mb && !msgs) return 2;
  if (int rcg = ensure_device_gens(gens, ngens)) return rcg;
  EdPoint* d_gens = g_d_gens;
  const bool to_dev = out_at_head || w.rest;
  const size_t o_off = w.head, o_out = o_off + (((n + 1) * 8 + 255) & ~size_t(255)), o_bytes = o_out + (to_dev ? 0 : (n * 48 + 255) & ~size_t(255));
  HashScratch* hs = nullptr;
  if (hash_scratch(o_bytes + (w.msgs ? 0 : mb + 8), &hs)) return 10;
  CallScope cs(w.rest ? w.stream : hs->stream);
  const hipStream_t st = cs.stream();
  uint64_t* d_off = (uint64_t*)(hs->buf + o_off);
  uint8_t* d_out = out_at_head ? hs->buf : w.rest ? out48 : hs->buf + o_out;
  const uint8_t* d_bytes = w.msgs ? msgs : hs->buf + o_bytes;
  if (mb && !w.msgs) HIP_TRY(hipMemcpyAsync(hs->buf + o_bytes, msgs, mb, hipMemcpyHostToDevice, st), 10);
  HIP_TRY(hipMemcpyAsync(d_off, msg_off, (n + 1) * 8, hipMemcpyHostToDevice, st), 10);
  EvLog log(st);
  const hipEvent_t e0 = log.open();
  if (L == 1) hipLaunchKernelGGL(k_pedersen_crh, dim3(((uint32_t)n + 63) / 64), dim3(64), 0, st, d_gens, d_bytes, d_off, d_out, (uint32_t)n);
  else {
    const uint32_t per = CRH_BLOCK / L;         // messages per workgroup
    crh_lanes_launch((uint32_t)((n + per - 1) / per), st, d_gens, d_bytes, d_off, d_out, (uint32_t)n, L);
  }
  HIP_TRY(hipGetLastError(), 10);
  log.close(0, e0);
  if (!to_dev) HIP_TRY(hipMemcpyAsync(out48, d_out, n * 48, hipMemcpyDeviceToHost, st), 10);
  HIP_TRY(hipStreamSynchronize(st), 10);
  float ms = 0.f;
  log.sum(&ms);
  g_hash_last.update([&](HashLast& r) { r.ms = ms; r.crh_lanes = (int)L; });
  if (w.kernel_ms) *w.kernel_ms = ms;
  return 0;
}
int pedersen_crh_run(const uint8_t* msgs, const uint64_t* msg_off, size_t n, uint8_t* out48, int dev, void* stream, float* kernel_ms) {
  size_t ngens = 0;
  const EdPoint* gens = celo_composite_gens(&ngens);      // before the lock: building the table takes 0.5 s on first use
  if (int rc0 = api_enter()) return rc0;
  std::lock_guard<std::mutex> lk(hash_mu);
  HashWhere w;
  w.msgs = w.rest = dev != 0;
  w.stream = (hipStream_t)stream;
  w.kernel_ms = kernel_ms;
  return pedersen_crh_locked(msgs, msg_off, n, out48, gens, ngens, w, false);
}
int crh_set_lanes(int lanes) {
  if (lanes != 0 && !crh_lanes_ok(lanes)) return 2;
  g_crh_lanes.store(lanes);
  return 0;
}
int crh_last_lanes() { return g_hash_last.read().crh_lanes; }
float hash_last_ms() { return g_hash_last.read().ms; }
int hash_last_rounds() { return g_hash_last.read().rounds; }
}  // namespace celo
