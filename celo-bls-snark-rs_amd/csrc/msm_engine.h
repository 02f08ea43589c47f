// The MSM host driver: tuning switches (MsmTuning), the engine (arena, streams, plan), run_device_windows / run_host_windows and the host epilogue.
// (part of the MSM pipeline: csrc/msm.h includes the pieces in order and carries the overview)
#pragma once

namespace celo {

// ---------------------------------------------------------------- host driver
// the IFMA Horner epilogue (host_ifma.cpp, host_cpu.cpp) exists for the two prime fields
extern "C" int celo_ifma_available();
extern "C" int celo_ifma_horner_377(const uint64_t* pts, size_t stride, const int32_t* order, int steps, uint64_t* out, int* inf);
extern "C" int celo_ifma_horner_761(const uint64_t* pts, size_t stride, const int32_t* order, int steps, uint64_t* out, int* inf);
typedef int (*ifma_horner_fn)(const uint64_t*, size_t, const int32_t*, int, uint64_t*, int*);
template <class F> struct IfmaHorner { static constexpr ifma_horner_fn fn = nullptr; };
template <> struct IfmaHorner<Fp<P377>> { static constexpr ifma_horner_fn fn = &celo_ifma_horner_377; };
template <> struct IfmaHorner<Fp<P761>> { static constexpr ifma_horner_fn fn = &celo_ifma_horner_761; };

struct MsmTimings {  // milliseconds, HIP events on the MSM's stream (last call)
  float convert = 0, sort = 0, accumulate = 0, reduce = 0, total = 0;
};

}  // namespace celo
#include "msm_ba.h"
namespace celo {
template <> struct BaCfg<G_761> { static constexpr bool enabled = true; };

// What is still read from outside, from the environment ONCE per process (not per engine, not per call); INTEGRATION.md lists both with the
// test that covers the non-default.  The A/B switches of rounds 2-6 are decided: their environment hooks went in round 6 (nobody could review a
// library with 27 switches), their run-time fields and branches after it; what they settled are the named constants below and in the engine.
struct MsmTuning {
  uint32_t host_chunks;    // host-pointer entry: index chunks of the pipelined transfer (CELO_HOST_CHUNKS; not set = 0xFFFFFFFF: the group's own default; 0 or 1 = the plain form - celo_amd_msm_set_host_chunks(1), the test hook, is what runs ONE chunk through the pipelined code)
  int batched_affine;      // CELO_BA: 0 (default) = the XYZZ chain everywhere, 1 = batched-affine pre-levels (msm_ba.h) for the groups that enable them (BW6-761); measured level with the XYZZ chain (profiles/r6_ba_ab.txt): off
  static const MsmTuning& get() {
    static const MsmTuning t = {getenv("CELO_HOST_CHUNKS") ? (uint32_t)atoi(getenv("CELO_HOST_CHUNKS")) : 0xFFFFFFFFu, getenv("CELO_BA") ? atoi(getenv("CELO_BA")) : 0};
    return t;
  }
};
// the batched-affine pre-levels' shape (profiles/r6_ba_ab.txt: the best of the variants measured): tree levels before the XYZZ chain (at most
// BA_K_MAX), waves per SIMD of k_ba_levels, and the grid = BA_ROUNDS rounds of the lanes in flight
constexpr int BA_LEVELS = 3, BA_OCC = 2;
constexpr uint32_t BA_ROUNDS = 2;

template <class G> class MsmEngine {
 public:
  typedef typename G::F F;
  typedef PointIO<F> IO;
  typedef typename HostField<F>::type HostF;
  static constexpr int SW = G::SCALAR_WORDS;

  ~MsmEngine() { release(); }
  void release() {
    if (arena) { (void)hipFree(arena); arena = nullptr; arena_bytes = 0; }
    if (fxs) { (void)hipFree(fxs); fxs = nullptr; fxs_bytes = 0; }
    free_staging();
    if (h_out) { (void)hipHostFree(h_out); h_out = nullptr; }
    if (d_side_out) { (void)hipFree(d_side_out); d_side_out = nullptr; side_out_bytes = 0; }
    if (d_fx_scalars) { (void)hipFree(d_fx_scalars); d_fx_scalars = nullptr; cap_fx = 0; }
    for (int i = 0; i < 6; i++) if (ev[i]) { (void)hipEventDestroy(ev[i]); ev[i] = nullptr; }
    for (hipEvent_t e : ev_copy) if (e) (void)hipEventDestroy(e);
    ev_copy.clear();
  }
  // Measured on the MI355X (sweep over c at n = 2^8 .. 2^20, uniform scalars, all groups): with the log-depth bucket reduction
  // the buckets are cheap and the accumulate lanes are not - few long bucket runs are pure latency - so small and mid-size
  // inputs want MORE buckets than points, and a window size that DIVIDES the scalar length wins by up to 2x because no ragged
  // top window (few, heavy buckets) is left: 253 = 11 * 23 and 377 = 13 * 29.
  //   253-bit scalars (BLS12-377): c = 11 below 2^15 points (0.34 ms at n = 256, was 0.9 with c = 4), 15 below 2^19, then 16
  //   377-bit scalars (BW6-761):   c = 13 below 2^19 points (6.9 ms at 2^18, was 7.1 with c = 14 and 8.6 with 15), then 16
  static int window_bits(size_t n) {
    if (G::SCALAR_BITS > 256) {
      if (n < 512) return 9;
      return n < (size_t(1) << 19) ? 13 : 16;
    }
    if (n < (size_t(1) << 15)) return 11;
    return n < (size_t(1) << 19) ? 15 : 16;
  }
  int force_c = 0;  // test hook / tuning: 0 = auto
  hipStream_t own_stream() { return stream_.get(); }   // this engine's non-blocking stream (host-pointer entry points)
  // big path: mixed window widths (k_digits) for the 16-bit configuration only - the large inputs, where the work is throughput
  // and a ragged top window costs folds and balance (2^20 terms: G1 3.32 -> 3.31, G2 10.85 -> 10.75, BW6-761 19.5 -> 19.0 ms).
  // Small inputs are bound by their longest bucket run, and narrower windows mean longer runs: BW6-761 at 2^14 with 18 x 13 + 12 x 12
  // bits instead of 29 x 13 (+ a carry window) 1.39 -> 1.88 ms, at 2^17 3.58 -> 3.79 ms.
  static bool narrow_top(int c) { return c == 16; }
  // big path, G1 of BLS12-377: the caller vouches for bases in the prime-order subgroup (Signature values, proving-key points): GLV split
  bool big_subgroup_points = false;
  // host-pointer entry (run_host), set by the Groth16 prover's entry points only: a base row x = 0, y = 1 is the identity (k_flag_ark_zero)
  bool ark_zero_identity = false;
  bool last_glv = false;
  // window size for the 2 n points x 127-bit halves of the split (n = the expanded count)
  // (measured, round 3: 127 = 8 x 16 - 1, so c = 16 leaves no ragged top window and wins at every size from 2^14 terms up)
  static int window_bits_glv(size_t) { return 16; }
  // batched path, G2 of BLS12-377: the caller vouches that every base lies in the prime-order subgroup (Batch::verify's public keys:
  // PublicKey values only come from checked deserialisation, secret keys and sums of such), which is what makes psi(P) = [x]P.
  // (The library never applies psi to the plain entry points' arbitrary curve points: ADVICE r3.)
  bool gls_subgroup_points = false;
  int last_gls_digits = 1;
  static constexpr int HOST_HORNER_THREADS = 4;
  static constexpr uint32_t SEG_MIN = 32;          // shortest piece of a whole MSM
  static constexpr uint32_t SEG_MIN_SHARD = 16;    // ... of a window shard (8 / 12 / 16 measure alike)
  // bucket reduction: three lanes per addition (k_bitsum_lanes) for the launches of at most this many outputs - one wave of 21 additions per
  // SIMD -, whole MSMs and window shards alike; the launches above it take k_bitsum, one lane per addition
  static constexpr uint32_t BITSUM_LANES_MAX = 21 * 1024;

  // bases/scalars/inf are DEVICE pointers (ark layout); result: Jacobian in ark Montgomery form (3*ARK64 u64) on host.
  // The shape of a call: whether the GLV split is taken, the expanded term count, the scalar length, the window size and count.
  struct Plan { bool glv; uint32_t n; int sbits, c, nw, kn; };
  // allow_glv = false: the pipelined host-pointer form, whose chunks never take the split (its expansion reads bases and scalars together)
  Plan plan(size_t n_, bool allow_glv = true) const {
    Plan p;
    // GLV split (big_subgroup_points: the caller vouches for bases in the prime-order subgroup): 2 n_ terms of sbits-bit scalars
    // (from 2^14 terms: below, the plain path's c = 11 is as fast - measured 0.53 / 0.59 ms at 2^12 / 2^13 either way)
    p.glv = allow_glv && GlvExpand<G>::AVAILABLE && big_subgroup_points && n_ >= (size_t(1) << 14);
    p.n = p.glv ? 2u * (uint32_t)n_ : (uint32_t)n_;
    p.sbits = p.glv ? GlvExpand<G>::BITS : G::SCALAR_BITS;
    p.c = force_c ? force_c : (p.glv ? window_bits_glv(p.n) : window_bits(p.n));
    p.nw = (p.sbits + p.c) / p.c;
    p.kn = narrow_top(p.c) ? p.nw * p.c - (p.sbits + 1) : 0;    // the top kn windows are c - 1 bits wide (k_digits)
    return p;
  }
  // fixed base: the pipeline runs over the table's entries - all E of them, or (digits compacted by window) the fullest window's row of Ep -
  // in NV virtual windows of 2^15 buckets
  static Plan fixed_plan(const FixedTable& T, uint32_t Ep) { return {false, Ep ? Ep : T.E(), G::SCALAR_BITS, 16, (int)T.NV, 0}; }
  // first scalar bit of window w (windows of mixed width: the top kn of the nw are c - 1 bits wide)
  static int window_bit(const Plan& p, int w) {
    const int wide = p.nw - p.kn;
    return w < wide ? w * p.c : wide * p.c + (w - wide) * (p.c - 1);
  }
  int run_device(const uint64_t* d_ark_bases, const uint8_t* d_inf, const uint32_t* d_scalars, size_t n_, uint64_t* out_jac,
                 hipStream_t stream) {
    return run_device_windows(d_ark_bases, d_inf, d_scalars, n_, 0, 0, out_jac, nullptr, stream);
  }
  // The same pipeline over the windows [win_lo, win_lo + win_cnt) of the call's plan only (win_cnt = 0: all of them): the WINDOW
  // partition of one MSM over several devices (msm_unit.h msm_multi_windows_impl; SURVEY.md section 8e "alternative partitioning").
  // The result is then the partial sum  sum_{w in range} 2^(bit(w) - bit(win_lo)) S_w  - the caller weighs it by 2^bit(win_lo).
  // out_xyzz (optional, 4 * ARK64 u64: X, Y, ZZ, ZZZ in arkworks limbs, ZZ = 0 for the identity) hands the partial over in the host
  // epilogue's own coordinates, so that the join needs no conversion.
  // fx != nullptr: the FIXED-BASE form (FixedTable above): d_ark_bases / d_inf are unused, n_ = the number of scalars (<= fx->n), the
  // pipeline runs over the table's E entries in NV virtual windows of 2^15 buckets.
  // hin != nullptr: the HOST-POINTER pipeline (round 5; VERDICT r4 item 1 - the call a drop-in caller makes: signature.rs:82-85,
  // public.rs:58-61 hand host slices to multi_scalar_mul).  d_ark_bases / d_inf / d_scalars are then the engine's staging buffers, still
  // EMPTY: scalars (and flags) and bases cross in hin->chunks index chunks while the chunks before are sorted and accumulated (enqueue_host_pipeline).
  // The stages, private members below: fixed_compact_digits | big_layout, ensure, bind | enqueue_host_pipeline or enqueue_resident |
  // enqueue_bucket_reduction | fetch_results | host_epilogue.
  struct HostIn { const uint64_t* bases; const uint8_t* inf; const uint64_t* scalars; uint32_t chunks, head_split, tail_split; bool ark_zero; };
  static constexpr uint32_t HOST_HEAD_SPLIT_DEFAULT = 1, HOST_TAIL_SPLIT_DEFAULT = 0;      // (host_chunk_plan: runtime.h)
  int run_device_windows(const uint64_t* d_ark_bases, const uint8_t* d_inf, const uint32_t* d_scalars, size_t n_, int win_lo, int win_cnt,
                         uint64_t* out_jac, uint64_t* out_xyzz, hipStream_t stream, const FixedTable* fx = nullptr, const HostIn* hin = nullptr) {
    if (n_ == 0) {
      if (out_jac) write_identity(out_jac);
      if (out_xyzz) memset(out_xyzz, 0, 4 * IO::ARK64 * 8);
      return 0;
    }
    if (n_ >= (size_t(1) << 30)) return 2;
    if (fx && (win_cnt || n_ > fx->n || fx->cf < 16 || fx->cf > 22)) return 2;
    FxDigits fxd;
    if (fx) if (const int rc = fixed_compact_digits(*fx, d_scalars, (uint32_t)n_, stream, fxd)) return rc;
    BigLayout L;
    if (const int rc = big_layout(fx ? fixed_plan(*fx, fxd.Ep) : plan(n_, !hin), (uint32_t)n_, win_lo, win_cnt, fx, fxd, hin, L)) return rc;
    if (ensure(L.bytes)) return 1;
    if (L.res_pts > H_OUT_POINTS) return 2;
    L.bind(arena);
    HIP_TRY(hipEventRecord(ev[0], stream), 1);
    if (const int rc = hin ? enqueue_host_pipeline(L, *hin, d_ark_bases, d_inf, d_scalars, stream) : enqueue_resident(L, d_ark_bases, d_inf, d_scalars, stream)) return rc;
    HIP_TRY(hipEventRecord(ev[3], stream), 1);
    if (const int rc = enqueue_bucket_reduction(L, stream)) return rc;
    if (const int rc = fetch_results(L, stream)) return rc;
    host_epilogue(L, out_jac, out_xyzz);
    return 0;
  }
  static void write_host_jacobian(const HXyzz<HostF>& pt, uint64_t* out_jac) {
    if (pt.is_identity()) { write_identity(out_jac); return; }
    (pt.X * pt.ZZ).store(out_jac);                 // (X ZZ, Y ZZZ, ZZ) is a Jacobian representative with Z = ZZ
    (pt.Y * pt.ZZZ).store(out_jac + IO::ARK64);
    pt.ZZ.store(out_jac + 2 * IO::ARK64);
  }

  // host-pointer entry: stages inputs into (cached) device buffers, then run_device
  int run_host(const uint64_t* bases, const uint8_t* inf, const uint64_t* scalars, size_t n, uint64_t* out_jac, hipStream_t stream) {
    return run_host_windows(bases, inf, scalars, n, 0, 0, out_jac, nullptr, stream);
  }
  int run_host_windows(const uint64_t* bases, const uint8_t* inf, const uint64_t* scalars, size_t n, int win_lo, int win_cnt, uint64_t* out_jac,
                       uint64_t* out_xyzz, hipStream_t stream) {
    if (n == 0) return run_device_windows(nullptr, nullptr, nullptr, 0, win_lo, win_cnt, out_jac, out_xyzz, stream);
    const HostChunks hc = host_chunk_choice(n, win_cnt);
    if (const int rc = reserve_staging(hc.need)) return rc;
    if (hc.pipelined) {
      const HostIn hin = {bases, inf, scalars, hc.chunks, hc.head_split, hc.tail_split, ark_zero_identity};
      return run_device_windows(d_in_bases, inf || ark_zero_identity ? d_in_inf : nullptr, (const uint32_t*)d_in_scalars, n, 0, 0, out_jac, out_xyzz, stream, nullptr, &hin);
    }
    // the plain form: three transfers, then the resident pipeline
    HIP_TRY(hipMemcpyAsync(d_in_bases, bases, n * 2 * IO::ARK64 * 8, hipMemcpyHostToDevice, stream), 1);
    HIP_TRY(hipMemcpyAsync(d_in_scalars, scalars, n * SW * 4, hipMemcpyHostToDevice, stream), 1);
    if (inf) HIP_TRY(hipMemcpyAsync(d_in_inf, inf, n, hipMemcpyHostToDevice, stream), 1);
    if (ark_zero_identity) {       // the prover's queries: rows (0, 1) are arkworks' encoding of the identity
      ArkCoord<IO::ARK64> one;
      F::one().to_ark(one.v);
      hipLaunchKernelGGL((k_flag_ark_zero<G>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_in_bases, inf ? d_in_inf : nullptr, d_in_inf, n, one);
    }
    return run_device_windows(d_in_bases, inf || ark_zero_identity ? d_in_inf : nullptr, (const uint32_t*)d_in_scalars, n, win_lo, win_cnt, out_jac, out_xyzz, stream);
  }

  // ---- fixed-base form (FixedTable): the scalars come from the host (staged into a buffer of their own) or are resident
  int run_fixed(const FixedTable& T, const void* scalars, size_t n_sc, int resident, uint64_t* out_jac, hipStream_t stream) {
    if (n_sc > T.n) n_sc = T.n;                                   // VariableBaseMSM zips bases with scalars: the shorter side decides
    if (n_sc == 0) { write_identity(out_jac); return 0; }
    const uint32_t* d_sc = (const uint32_t*)scalars;
    if (!resident) {
      if (n_sc > cap_fx) {
        if (d_fx_scalars) (void)hipFree(d_fx_scalars);
        d_fx_scalars = nullptr; cap_fx = 0;
        HIP_TRY(hipMalloc(&d_fx_scalars, n_sc * SW * 4), 1);
        cap_fx = n_sc;
      }
      HIP_TRY(hipMemcpyAsync(d_fx_scalars, scalars, n_sc * SW * 4, hipMemcpyHostToDevice, stream), 1);
      d_sc = (const uint32_t*)d_fx_scalars;
    }
    return run_device_windows(nullptr, nullptr, d_sc, n_sc, 0, 0, out_jac, nullptr, stream, &T);
  }
  // window size of a key's table: buckets ~ entries / 64 within [2^15, 2^19] (measured sweep: DESIGN.md section 4 "Fixed base")
  static int fixed_window_bits(size_t n) {
    int lg = 0;
    while ((size_t(1) << lg) < n * ((G::SCALAR_BITS + 16) / 16)) lg++;
    int cf = lg - 4;      // 2^21 BW6-761 terms: 21 (26.3 ms against 33.3 variable-base; 26.8 at 20); 2^20 G1 terms: 20 (3.08 against 3.3 ms; 4.75 at 21)
    // (21 only where the additions are expensive enough to pay for twice the buckets: the 28-limb fields; measured with the digits compacted
    // by virtual window - before that 20 was the optimum everywhere, profiles/r4_fixed_sweep.txt)
    const int top = sizeof(F) > 14 * sizeof(uint32_t) ? 21 : 20;
    return cf < 16 ? 16 : cf > top ? top : cf;
  }
  // builds T (device memory of the calling thread's device) from n affine bases in arkworks layout; d_* are DEVICE pointers
  static int fixed_build(const uint64_t* d_ark_bases, const uint8_t* d_inf, size_t n_, int cf, FixedTable* T, hipStream_t stream) {
    if (n_ == 0 || n_ >= (size_t(1) << 27)) return 2;
    // the pipeline's 32-bit run offsets bound a table: n W < 2^31 entries and (uncompacted form: every entry in every virtual window)
    // n W NV < 2^32.  With the automatic choice the window steps down until both hold (2^24 BW6-761 terms at the preferred cf = 21
    // are W = 18, NV = 33: 10^10 slots - the key's size the header names for the prover; cf = 19 fits); an explicit cf that does not fit is refused.
    auto fits = [&](int c_) {
      const uint64_t W_ = (uint64_t)((G::SCALAR_BITS + c_) / c_), M_ = c_ == 16 ? 32768u : 32767u, NV_ = ((uint64_t(1) << (c_ - 1)) - 1u) / M_ + 1u;
      return (uint64_t)n_ * W_ < (uint64_t(1) << 31) && (uint64_t)n_ * W_ * NV_ < (uint64_t(1) << 32);
    };
    if (cf == 0) {
      cf = fixed_window_bits(n_);
      while (cf > 16 && !fits(cf)) cf--;
    }
    if (cf < 16 || cf > 22 || !fits(cf)) return 2;
    const uint32_t n = (uint32_t)n_, W = (uint32_t)((G::SCALAR_BITS + cf) / cf);      // W cf >= SCALAR_BITS + 1: room for the signed recoding's carry
    const uint32_t M = cf == 16 ? 32768u : 32767u, NV = ((1u << (cf - 1)) - 1u) / M + 1u;
    const size_t E = (size_t)n * W;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_TRY(hipEventCreate(&e0), 1); HIP_TRY(hipEventCreate(&e1), 1);
    T->n = n; T->W = W; T->NV = NV; T->M = M; T->cf = cf; T->device = api_device();
    T->bytes = E * IO::AFF_WORDS * 4 + E;
    HIP_TRY(hipMalloc(&T->table, E * IO::AFF_WORDS * 4), 1);
    HIP_TRY(hipMalloc(&T->tinf, E), 1);
    HIP_TRY(hipEventRecord(e0, stream), 1);
    hipLaunchKernelGGL((k_convert_bases<G>), dim3((n + 255) / 256), dim3(256), 0, stream, d_ark_bases, T->table, (size_t)n);
    hipLaunchKernelGGL((k_fixed_first_flags<G>), dim3((n + 255) / 256), dim3(256), 0, stream, d_inf, T->tinf, n);
    for (uint32_t j = 1; j < W; j++)
      hipLaunchKernelGGL((k_fixed_next<G>), dim3((n + 127) / 128), dim3(128), 0, stream, T->table + (size_t)(j - 1) * n * IO::AFF_WORDS, T->tinf + (size_t)(j - 1) * n,
                         T->table + (size_t)j * n * IO::AFF_WORDS, T->tinf + (size_t)j * n, n, cf);
    HIP_TRY(hipEventRecord(e1, stream), 1);
    HIP_TRY(hipStreamSynchronize(stream), 1);
    HIP_TRY(hipGetLastError(), 1);
    (void)hipEventElapsedTime(&T->build_ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return 0;
  }

  // ---- batched small MSMs (host pointers).  offsets[m+1]; every instance must have <= 1024 points (larger instances go
  // through run_host one by one).  out: m Jacobian results (arkworks form).
  static constexpr uint32_t BATCH_MAX_N = 1024;
  MsmTimings tm_batch;
  int batch_bits = 0;   // length of the longest scalar of the last batched call
  // bits_hint > 0: the length of the longest scalar of the NEXT batched call, measured by the caller on the same scalars (spares the
  // k_scalar_or round trip: with the chip full of another engine's accumulation that small kernel and its synchronisation waited 16 ms
  // inside batch_verify_strict, and the G1 leg was enqueued only then); measured_bits: what the last call used (bits from SCALAR_BITS up not counted)
  int bits_hint = 0, measured_bits = 0;
  int run_batch_host(const uint64_t* bases, const uint8_t* inf, const uint64_t* scalars, const uint32_t* offsets, size_t m,
                     uint64_t* out, hipStream_t stream) {
    return run_batch(bases, inf, scalars, 0, offsets, m, out, nullptr, stream);
  }
  // resident = 0: bases / inf / scalars are HOST pointers (staged into the arena); 1: DEVICE pointers (used in place).
  // out: host buffer for the m Jacobian results, or nullptr to leave them on the device: *d_out_ret then points at them (in this
  // engine's arena, valid until its next call) and the call returns with the work ENQUEUED on `stream`, not finished - the
  // caller chains its consumer behind it (batch verification: normalise + pairing inputs without a host round trip).
  int run_batch(const uint64_t* bases, const uint8_t* inf, const uint64_t* scalars, int resident, const uint32_t* offsets, size_t m,
                uint64_t* out, uint64_t** d_out_ret, hipStream_t stream) {
    measured_bits = 0;                                     // stays 0 on the paths that do not measure (no hint to hand on)
    if (m == 0) return 0;
    const uint32_t total_pts = offsets[m];
    uint32_t max_n = 0;
    for (size_t p = 0; p < m; p++) {
      uint32_t k = offsets[p + 1] - offsets[p];
      if (k > max_n) max_n = k;
    }
    if (max_n > BATCH_MAX_N || total_pts == 0) {
      // An instance beyond the per-workgroup sort (or a call whose instances are all empty): every instance goes through the big
      // pipeline, one after the other (still the GPU; Batch::verify takes any number of signers and accepts an empty batch,
      // crates/bls-crypto/src/bls/batch.rs:44-84).  The big pipeline carves this engine's arena, so in the chained form the m
      // results are collected on the host and put into a buffer of their own; the call is then synchronous, which the chained
      // contract allows (the consumer waits on the stream either way).
      std::vector<uint64_t> hres;
      uint64_t* dst = out;
      if (!out) { hres.resize(m * 3 * IO::ARK64); dst = hres.data(); }
      for (size_t p = 0; p < m; p++) {
        const uint32_t lo = offsets[p], k = offsets[p + 1] - lo;
        const uint8_t* pi = inf ? inf + lo : nullptr;
        const int rc = resident ? run_device(bases + (size_t)lo * 2 * IO::ARK64, pi, (const uint32_t*)scalars + (size_t)lo * SW, k, dst + p * 3 * IO::ARK64, stream)
                                : run_host(bases + (size_t)lo * 2 * IO::ARK64, pi, scalars + (size_t)lo * (SW / 2), k, dst + p * 3 * IO::ARK64, stream);
        if (rc) return rc;
      }
      tm_batch = tm;
      if (!out) {
        const size_t bytes = m * 3 * IO::ARK64 * 8;
        if (bytes > side_out_bytes) {
          if (d_side_out) (void)hipFree(d_side_out);
          d_side_out = nullptr; side_out_bytes = 0;
          HIP_TRY(hipMalloc(&d_side_out, bytes), 1);
          side_out_bytes = bytes;
        }
        HIP_TRY(hipMemcpyAsync(d_side_out, hres.data(), bytes, hipMemcpyHostToDevice, stream), 1);
        HIP_TRY(hipStreamSynchronize(stream), 1);
        if (d_out_ret) *d_out_ret = d_side_out;
        side_path = true;
      }
      return 0;
    }
    side_path = false;
    // window size ~ log2(n) - 3 (measured on 4096 x 256, 136-bit exponents: c = 5 beats 6 and 7; the per-(instance,window)
    // running sums and the per-instance Horner are latency-bound, so fewer buckets per window win)
    auto window_for = [&](uint32_t inst_n) {
      int c_ = force_c ? force_c : 3;
      if (!force_c) { while (c_ < 7 && (16u << c_) <= inst_n) c_++; }
      if (c_ > 7) c_ = 7;
      if (c_ < 3) c_ = 3;
      return c_;
    };
    // GLS split (G2 of BLS12-377, subgroup points only: gls_subgroup_points): k = d0 + d1 x + d2 x^2 + d3 x^3 in base x, the curve
    // parameter, and [x]P = psi(P) - so an instance of n points with b-bit scalars becomes one of nd n points psi^j(P) with 64-bit
    // scalars, nd = 2 (b <= 126), 3 (b <= 189: Batch::verify's 136-bit exponents) or 4.  Same group element; what changes is the
    // shape: a quarter to a half of the windows (13 x 5 bits instead of 28) over a larger instance, which takes a wider window
    // (c = 6 for 768 points: 11 windows) - 14 % fewer mixed additions, less than half the per-(instance, window) running sums and
    // a Horner chain of 66 doublings instead of 140.
    const int gls_max = (GlsExpand<G>::AVAILABLE && gls_subgroup_points) ? 4 : 1;
    auto gls_digits = [&](int bits) {
      if (gls_max == 1 || bits <= 64) return 1;
      const int nd_ = bits <= 126 ? 2 : bits <= 189 ? 3 : 4;
      return (size_t)nd_ * max_n <= BATCH_MAX_N ? nd_ : 1;
    };
    // stage the inputs at the front of the arena, then let the scalars decide the number of windows: bits = length of the longest
    // scalar present.  The arena is sized for the worst layout (full-length scalars, or the largest split that fits) beforehand.
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~size_t(255); return o; };
    const size_t o_in_b = take(resident ? 0 : (size_t)total_pts * 2 * IO::ARK64 * 8), o_in_s = take(resident ? 0 : (size_t)total_pts * SW * 4),
                 o_in_i = take(resident ? 0 : total_pts + 8);
    const size_t o_off = take((m + 1) * 4), o_or = take(64 * 4);
    const size_t front = off;
    auto rest = [&](int c_, int nw_, int nd_, size_t* o) {     // the part of the arena that depends on the layout; returns its end
      size_t save = off;
      off = front;
      const uint32_t B_ = 1u << (c_ - 1);
      const size_t tot = (size_t)nd_ * total_pts;
      const size_t nvw_ = m * (size_t)nw_, nb = nvw_ * B_, en = tot * nw_;
      o[0] = take(tot * IO::AFF_WORDS * 4); o[1] = take(en * 4 + 16);
      o[2] = take(nb * 4); o[3] = take(nb * 4); o[4] = take(nb * 4);
      o[5] = take((size_t)SIZE_BINS * 4 + 256); o[6] = take(nb * IO::XYZZ_WORDS * 4);
      o[7] = take(nvw_ * IO::XYZZ_WORDS * 4); o[8] = take(m * 3 * IO::ARK64 * 8);
      o[9] = take(nd_ > 1 ? tot * 16 : 0); o[10] = take(nd_ > 1 ? tot + 8 : 0); o[11] = take(nd_ > 1 ? (m + 1) * 4 : 0);
      const size_t end = off;
      off = save;
      return end;
    };
    size_t o[12];
    {
      const int c1 = window_for(max_n);
      const int nw1 = (G::SCALAR_BITS + c1) / c1;
      if (m * (size_t)nw1 * (size_t(1) << (c1 - 1)) >= (size_t(1) << 31) || (size_t)total_pts * nw1 >= (size_t(1) << 32)) return 2;
      size_t need = rest(c1, nw1, 1, o);
      for (int nd_ = 2; nd_ <= gls_max; nd_++) {
        if ((size_t)nd_ * max_n > BATCH_MAX_N) break;
        const int c2 = window_for((uint32_t)nd_ * max_n);
        const size_t e2 = rest(c2, (64 + c2) / c2, nd_, o);
        if (e2 > need) need = e2;
      }
      if (ensure(need)) return 1;
    }
    {
      char* A0 = arena;
      if (!resident) HIP_TRY(hipMemcpyAsync(A0 + o_in_s, scalars, (size_t)total_pts * SW * 4, hipMemcpyHostToDevice, stream), 1);
      int bits = 1;
      if (bits_hint > 0) bits = bits_hint;          // the caller measured these very scalars already (batch verification: the other leg's engine)
      else {
        HIP_TRY(hipMemsetAsync(A0 + o_or, 0, 64 * 4, stream), 1);
        hipLaunchKernelGGL((k_scalar_or<SW>), dim3(2048), dim3(256), 0, stream, resident ? (const uint32_t*)scalars : (const uint32_t*)(A0 + o_in_s),
                           (size_t)total_pts * SW, (uint32_t*)(A0 + o_or));
        uint32_t h_or[SW];
        HIP_TRY(hipMemcpyAsync(h_or, A0 + o_or, SW * 4, hipMemcpyDeviceToHost, stream), 1);
        HIP_TRY(hipStreamSynchronize(stream), 1);
        static_assert(BatchTopWord<SW>::MASK == (1u << (G::SCALAR_BITS - 32 * (SW - 1))) - 1u, "the container's bits from SCALAR_BITS up");
        h_or[SW - 1] &= BatchTopWord<SW>::MASK;     // not part of any scalar (msm_batch.h): they neither add windows nor switch the split off
        for (int k = SW - 1; k >= 0; k--) if (h_or[k]) { bits = 32 * k + 32 - __builtin_clz(h_or[k]); break; }
      }
      if (bits > G::SCALAR_BITS) bits = G::SCALAR_BITS;     // (a caller's hint)
      measured_bits = bits;
      batch_bits = bits;
    }
    const int nd = gls_digits(batch_bits);
    const uint32_t eff_max_n = (uint32_t)nd * max_n, eff_total = (uint32_t)nd * total_pts;
    const int eff_bits = nd > 1 ? 64 : batch_bits;
    const int c = window_for(eff_max_n);
    const uint32_t B = 1u << (c - 1);
    const int nw = (eff_bits + c) / c;
    const size_t nvw = m * (size_t)nw, nbuckets = nvw * B;
    if (nbuckets >= (size_t(1) << 31) || (size_t)eff_total * nw >= (size_t(1) << 32)) return 2;
    (void)rest(c, nw, nd, o);
    char* A = arena;
    const uint64_t* d_in_b = resident ? bases : (const uint64_t*)(A + o_in_b);
    const uint32_t* d_in_s = resident ? (const uint32_t*)scalars : (const uint32_t*)(A + o_in_s);
    const uint8_t* d_in_i = resident ? inf : (const uint8_t*)(A + o_in_i);
    uint32_t* d_off = (uint32_t*)(A + o_off);
    uint32_t* d_bases = (uint32_t*)(A + o[0]); uint32_t* d_sorted = (uint32_t*)(A + o[1]);
    uint32_t* d_pstart = (uint32_t*)(A + o[2]); uint32_t* d_plen = (uint32_t*)(A + o[3]); uint32_t* d_order = (uint32_t*)(A + o[4]);
    uint32_t* d_bins = (uint32_t*)(A + o[5]); uint32_t* d_nwork = d_bins + SIZE_BINS;
    uint32_t* d_partials = (uint32_t*)(A + o[6]); uint32_t* d_wsum = (uint32_t*)(A + o[7]); uint64_t* d_out = (uint64_t*)(A + o[8]);
    if (!resident) {
      HIP_TRY(hipMemcpyAsync(A + o_in_b, bases, (size_t)total_pts * 2 * IO::ARK64 * 8, hipMemcpyHostToDevice, stream), 1);
      if (inf) HIP_TRY(hipMemcpyAsync(A + o_in_i, inf, total_pts, hipMemcpyHostToDevice, stream), 1);
    }
    HIP_TRY(hipMemcpyAsync(d_off, offsets, (m + 1) * 4, hipMemcpyHostToDevice, stream), 1);
    HIP_TRY(hipEventRecord(ev[0], stream), 1);
    HIP_TRY(hipMemsetAsync(d_bins, 0, (size_t)SIZE_BINS * 4 + 256, stream), 1);
    if (nd > 1) {
      uint32_t* d_sc2 = (uint32_t*)(A + o[9]);
      uint8_t* d_inf2 = (uint8_t*)(A + o[10]);
      uint32_t* d_off2 = (uint32_t*)(A + o[11]);
      gls_off.resize(m + 1);
      for (size_t p = 0; p <= m; p++) gls_off[p] = (uint32_t)nd * offsets[p];
      HIP_TRY(hipMemcpyAsync(d_off2, gls_off.data(), (m + 1) * 4, hipMemcpyHostToDevice, stream), 1);
      GlsExpand<G>::launch(d_in_b, inf ? d_in_i : nullptr, d_in_s, d_off, (uint32_t)m, max_n, nd, batch_bits, d_bases, d_sc2, inf ? d_inf2 : nullptr, stream);
      HIP_TRY(hipEventRecord(ev[1], stream), 1);
      if (launch_batch_sort<4>(c, eff_max_n, d_sc2, inf ? d_inf2 : nullptr, d_off2, d_sorted, d_pstart, d_plen, (uint32_t)m, nw, stream)) return 3;
    } else {
      hipLaunchKernelGGL((k_convert_bases<G>), dim3((total_pts + 255) / 256), dim3(256), 0, stream, d_in_b, d_bases, (size_t)total_pts);
      HIP_TRY(hipEventRecord(ev[1], stream), 1);
      if (launch_batch_sort<SW>(c, max_n, d_in_s, inf ? d_in_i : nullptr, d_off, d_sorted, d_pstart, d_plen, (uint32_t)m, nw, stream)) return 3;
    }
    last_gls_digits = nd;
    const uint32_t slots = (uint32_t)nbuckets;
    hipLaunchKernelGGL((k_size_hist<G>), dim3(slots / 256 < 2048 ? (slots + 255) / 256 : 2048), dim3(256), 0, stream, d_plen, d_bins, slots);
    hipLaunchKernelGGL((k_size_scan<G>), dim3(1), dim3(1024), 0, stream, d_bins, d_nwork);
    hipLaunchKernelGGL((k_size_scatter<G>), dim3((slots + 4095) / 4096), dim3(1024), 0, stream, d_plen, d_bins, d_order, slots);
    HIP_TRY(hipEventRecord(ev[2], stream), 1);
    launch_accumulate<G>(slots, stream, d_bases, d_sorted, d_pstart, d_plen, d_order, d_nwork, d_partials);
    HIP_TRY(hipEventRecord(ev[3], stream), 1);
    hipLaunchKernelGGL((k_batch_reduce<G>), dim3(((uint32_t)nvw + 127) / 128), dim3(128), 0, stream, d_partials, d_plen, d_wsum, B, (uint32_t)nvw);
    BatchHornerLanes<G>::launch(d_wsum, d_out, (uint32_t)nw, (uint32_t)c, (uint32_t)m, stream);      // three (G2: six) lanes per instance
    HIP_TRY(hipEventRecord(ev[4], stream), 1);
    if (out) HIP_TRY(hipMemcpyAsync(out, d_out, m * 3 * IO::ARK64 * 8, hipMemcpyDeviceToHost, stream), 1);
    HIP_TRY(hipEventRecord(ev[5], stream), 1);
    last_c = c; last_nw = nw; last_buckets = (uint32_t)nbuckets;
    if (d_out_ret) *d_out_ret = d_out;
    if (!out) { HIP_TRY(hipGetLastError(), 1); return 0; }     // chained form: the caller synchronises and may call collect_batch_timings()
    HIP_TRY(hipStreamSynchronize(stream), 1);
    HIP_TRY(hipGetLastError(), 1);
    collect_batch_timings();
    return 0;
  }
  void collect_batch_timings() {     // after the stream has drained
    if (!side_path) read_timings(tm_batch);
    tm = tm_batch;
  }
  void read_timings(MsmTimings& t) {     // the stages' times between the call's events ev[0..5]
    (void)hipEventElapsedTime(&t.convert, ev[0], ev[1]);
    (void)hipEventElapsedTime(&t.sort, ev[1], ev[2]);
    (void)hipEventElapsedTime(&t.accumulate, ev[2], ev[3]);
    (void)hipEventElapsedTime(&t.reduce, ev[3], ev[4]);
    (void)hipEventElapsedTime(&t.total, ev[0], ev[5]);
  }

  MsmTimings tm;
  int last_c = 0, last_nw = 0;
  uint32_t last_buckets = 0;

  static void write_identity(uint64_t* out) {      // arkworks GroupProjective::zero() = (0, 1, 0); only z == 0 is significant
    F::zero().to_ark(out);
    F::one().to_ark(out + IO::ARK64);
    F::zero().to_ark(out + 2 * IO::ARK64);
  }

 private:
  char* arena = nullptr;  // one device allocation, carved per call (sizes depend on n and the window size)
  size_t arena_bytes = 0;
  uint64_t* d_in_bases = nullptr;
  uint64_t* d_in_scalars = nullptr;
  uint8_t* d_in_inf = nullptr;
  uint32_t* h_out = nullptr;
  uint64_t* d_fx_scalars = nullptr;    // staged scalars of the fixed-base form (run_fixed)
  size_t cap_fx = 0;
  uint8_t* fxs = nullptr;              // fixed base: the per-entry (window id, digit) records and the windows' counts, taken before the arena is laid out
  size_t fxs_bytes = 0;
  uint64_t* d_side_out = nullptr;      // results of a chained batch call that went through the big pipeline (run_batch)
  size_t side_out_bytes = 0;
  bool side_path = false;
  static constexpr size_t H_OUT_POINTS = 17 * 64;   // pinned result buffer: (LB + 1) * windows points; checked per call
  OwnedStream stream_;
  OwnedStream side_stream_;            // the host-pointer pipeline's copy stream
  OwnedStream sort_stream_;            // host-pointer pipeline: digits + sort + schedule of chunk k beside the accumulation of chunk k - 1
  std::vector<hipEvent_t> ev_copy;     // host-pointer pipeline: per chunk - scalars sent, bases sent, sorted; + one for the per-call fills
  std::vector<int32_t> horner_steps;   // the host epilogue's step list (host64.h), rebuilt per call
  std::vector<uint32_t> gls_off;       // instance offsets of the expanded (GLS) batch
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  size_t cap_in = 0;

  // ---- the big path's call shape
  // fixed base, digits compacted by virtual window (k_fixed_digits_c): Ep = the row length the pipeline is sized by, 0 = the uncompacted form
  struct FxDigits { uint32_t Ep = 0; uint8_t* v8 = nullptr; uint16_t* dg = nullptr; uint32_t* cnt = nullptr; };
  static constexpr size_t BINS_STRIDE = SIZE_BINS + 64;       // words: the size bins + nwork, nbig, nmid; one set per chunk (host-pointer pipeline)
  // The shape of one call and its arena: the mode, every derived size, the arena's offsets and total, and - after bind() - the typed device
  // pointers.  big_layout() computes it; the stages below only read it.
  struct BigLayout {
    const FixedTable* fx; FxDigits fxd; bool hin, shard;    // fixed base (+ its compacted digits) | host-pointer pipeline | window shard
    Plan pl;
    uint32_t n_in;                       // the caller's term count (pl.n: the pipeline's - GLV-expanded, or the fixed-base entries)
    int w0, nw, LB;                      // first window and window count of THIS call (everything below the digits is sized by nw); bucket-index bits
    uint32_t B, total;                   // buckets per window, of the call
    uint32_t K, cm, clen[HOST_CHUNKS_MAX];                   // host-pointer pipeline: K index chunks of cm points (lengths clen)
    uint32_t ns, nws, vw, npad, total_s; // the sort's view: ns entries in each of nws (virtual) windows
    uint32_t SEG, PW, slots;             // piece length, static piece region per window, all piece slots
    uint32_t res_pts, half_pts;          // bucket reduction: result points, most outputs of one launch
    uint32_t HIB, NBIN, KB2, chunk2, ts_threads, TILE, max_tiles;      // two-level sort
    bool use_ba; uint32_t ba_lanes, ba_pref_slots;           // batched-affine pre-levels
    size_t o_bases, o_sc2, o_digits, o_remap, o_sorted, o_blockcnt, o_binstart, o_tileprefix, o_recidx, o_reckey, o_counts, o_starts, o_piecesof, o_plen, o_bins,
        o_zero_end, o_pfirst, o_big, o_mid, o_pbucket, o_carrier, o_pstart, o_order, o_partials, o_work, o_ba_pts, o_ba_pref, bytes;
    uint32_t *d_bases, *d_sc2, *d_sorted, *d_blockcnt, *d_binstart, *d_recidx, *d_tileprefix, *d_counts, *d_starts, *d_pfirst, *d_piecesof, *d_big, *d_mid, *d_pstart, *d_plen,
        *d_order, *d_bins, *d_nwork, *d_nbig, *d_nmid, *d_partials, *d_work, *d_pbucket, *d_carrier, *d_remap, *d_ba_pts, *d_ba_pref;
    uint16_t *d_digits_all, *d_digits;   // every window's digits; this call's windows
    uint8_t* d_reckey;
    void bind(char* A) {
      auto u32 = [A](size_t o) { return (uint32_t*)(A + o); };
      d_bases = fx ? fx->table : u32(o_bases); d_sc2 = u32(o_sc2); d_remap = fxd.Ep ? u32(o_remap) : nullptr;
      d_digits_all = (uint16_t*)(A + o_digits); d_digits = d_digits_all + (size_t)w0 * pl.n;
      d_sorted = u32(o_sorted); d_blockcnt = u32(o_blockcnt); d_binstart = u32(o_binstart); d_tileprefix = u32(o_tileprefix); d_recidx = u32(o_recidx); d_reckey = (uint8_t*)(A + o_reckey);
      d_counts = u32(o_counts); d_starts = u32(o_starts); d_piecesof = u32(o_piecesof); d_plen = u32(o_plen); d_bins = u32(o_bins);      // (the zeroed group)
      d_nwork = d_bins + SIZE_BINS; d_nbig = d_nwork + 1; d_nmid = d_nwork + 2;
      d_pfirst = u32(o_pfirst); d_big = u32(o_big); d_mid = u32(o_mid); d_pstart = u32(o_pstart); d_order = u32(o_order); d_partials = u32(o_partials); d_work = u32(o_work);
      d_pbucket = hin ? u32(o_pbucket) : nullptr; d_carrier = hin ? u32(o_carrier) : nullptr;
      d_ba_pts = u32(o_ba_pts); d_ba_pref = u32(o_ba_pref);
    }
  };
  // Sizes and arena of a call from its plan and mode.  Returns 2 for a shape the pipeline refuses.
  int big_layout(const Plan& pl, uint32_t n_in, int win_lo, int win_cnt, const FixedTable* fx, const FxDigits& fxd, const HostIn* hin_, BigLayout& L) {
    if (hin_ && (fx || win_cnt || hin_->chunks < 1 || hin_->chunks > 64 || !side_stream_.get() || !sort_stream_.get())) return 2;
    L.fx = fx; L.fxd = fxd; L.hin = hin_ != nullptr; L.shard = win_cnt != 0; L.pl = pl; L.n_in = n_in;
    const uint32_t n = pl.n;
    const int c = pl.c, nw_all = pl.nw;
    const bool hin = L.hin;
    if (win_cnt < 0 || win_lo < 0 || (win_cnt && win_lo + win_cnt > nw_all)) return 2;
    L.w0 = win_cnt ? win_lo : 0;
    const int nw = L.nw = win_cnt ? win_cnt : nw_all;
    if ((uint64_t)n * (uint64_t)nw_all >= (uint64_t(1) << 32)) return 2;  // run offsets are 32-bit (n*windows < 2^32: n <= 2^27 at c = 16)
    const uint32_t B = L.B = 1u << (c - 1);
    L.total = (uint32_t)nw * B;
    // the sort's view: ns entries in each of nws windows - the call's own, or (host-pointer pipeline) the K index chunks of cm points
    // times the windows, chunk-major: virtual window k nw + w
    L.K = 0; L.cm = n;
    if (hin) L.K = host_chunk_plan(n, hin_->chunks, hin_->head_split, hin_->tail_split, L.cm, L.clen);
    const uint32_t K = L.K;
    const uint32_t ns = L.ns = hin ? L.cm : n, nws = L.nws = hin ? K * (uint32_t)nw : (uint32_t)nw;
    L.vw = hin ? (uint32_t)nw : 0u;
    const uint32_t npad = L.npad = hin ? K * L.cm : n;
    if ((uint64_t)npad * (uint64_t)nw_all >= (uint64_t(1) << 32)) return 2;
    const uint32_t total_s = L.total_s = nws * B;
    // piece length: twice the average bucket, within [SEG_MIN, SIZE_BINS-1]
    // (the split's buckets are twice as long - 64 points at 2^20 - and fewer: pieces of 1.5 mean buckets balance its last round better:
    // accumulate 2.64 -> 2.46 ms at 2^20; the plain path is flat between 1.5 and 3)
    const int seg_h = pl.glv ? 3 : 4;           // in half mean-bucket lengths
    uint32_t SEG = (uint32_t)seg_h * ((fx && !fxd.Ep ? n / (uint32_t)nw_all : ns) / B + 1) / 2;      // (fixed base: a virtual window holds E / NV of the entries; compacted: its row)
    uint32_t seg_min = SEG_MIN;
    const uint32_t lanes = (sizeof(F) <= 14 * sizeof(uint32_t)) ? 131072u : 65536u;      // in flight: 2 waves (14-limb field) or 1 per SIMD x 64 lanes x 1024 SIMDs
    if (win_cnt) {
      // a call that owns FEW windows (a window shard) has fewer additions than the chip has lanes x the usual piece length: a lane is
      // one addition per ~17 us whatever its neighbours do, so pieces of twice the mean bucket leave most SIMDs with nothing after the
      // first round.  Pieces as long as the additions per lane in flight (ACC_LANES) fill one round; the buckets cut in two or three
      // are folded by k_combine_mid_lanes.  Measured at 2^20 terms, 2 of 16 windows: accumulate 0.55 -> see DESIGN.md section 9.
      const uint64_t adds = (uint64_t)n * (uint64_t)nw;
      const uint32_t occ = (uint32_t)((adds + lanes - 1) / lanes);
      if (occ < SEG) { SEG = occ; seg_min = SEG_MIN_SHARD; }
    }
    if (fx) {
      // fixed base: few virtual windows hold all n W entries (one at cf = 16: mean bucket 1536) - pieces of twice the mean bucket would be
      // fewer than the chip has lanes; eight rounds of the lanes in flight bound the piece length instead (cf = 16: 72.9 -> see DESIGN.md)
      const uint32_t occ = fx->E() / (lanes * 8u) + 1u;
      if (occ < SEG) SEG = occ;
    }
    if (SEG < seg_min) SEG = seg_min;
    if (SEG > SIZE_BINS - 1) SEG = SIZE_BINS - 1;
    L.SEG = SEG;
    const uint32_t PW = L.PW = B + ns / SEG + 1;       // static piece region per window
    const uint32_t slots = L.slots = nws * PW;
    const int LB = L.LB = c - 1;                                   // bucket-index bits (c >= 4)
    L.res_pts = (uint32_t)(LB + 1) * (uint32_t)nw;                 // results: [0] = node(0,0), [l] = O_l, nw points each
    L.half_pts = (uint32_t)nw * (B / 2 + B / 4);                   // most outputs of one launch (the first)
    // two-level sort: NBIN bins per window by the low HIB bucket bits (<= 8 key bits above), KB2 blocks per window in the partition pass
    const uint32_t HIB = L.HIB = LB < 8 ? 0u : (uint32_t)LB - 8u, NBIN = L.NBIN = 1u << HIB;
    uint32_t KB2 = ns / (64 * NBIN > 4096 ? 64 * NBIN : 4096);
    if (KB2 < 1) KB2 = 1;
    if (KB2 > 64) KB2 = 64;
    L.KB2 = KB2;
    L.chunk2 = (ns + KB2 - 1) / KB2;
    // mean region ns / NBIN: the smallest workgroup whose tile capacity (TILE_EPT entries per lane) holds it with 20 % to spare
    const uint32_t region = ns / NBIN;
    L.ts_threads = region <= 2048 ? 256u : region <= 4096 ? 512u : 1024u;
    L.TILE = TILE_EPT * L.ts_threads; L.max_tiles = NBIN + ns / L.TILE + 1;
    // batched-affine pre-levels (msm_ba.h): the resident variable-base path of the groups that enable them, from mean runs of 8 points up
    const int ba_ovr = batched_affine_override().load();
    const bool use_ba = L.use_ba = BaCfg<G>::enabled && !hin && !fx && (ba_ovr >= 0 ? ba_ovr != 0 : MsmTuning::get().batched_affine != 0) && ns / B >= 8;
    uint32_t ba_lanes = use_ba ? BA_LANES_OCC1 * (uint32_t)BA_OCC * BA_ROUNDS : 0;       // the grid: whole rounds of the lanes in flight
    if (use_ba && ba_lanes > (slots + 255) / 256 * 256) ba_lanes = (slots + 255) / 256 * 256;
    L.ba_lanes = ba_lanes;
    L.ba_pref_slots = use_ba ? ((slots + ba_lanes - 1) / ba_lanes) * (SEG / 2) : 0;            // pairs of a lane's pieces, at most

    // ---- workspace arena
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~size_t(255); return o; };
    L.o_bases = take(fx ? 0 : (size_t)npad * IO::AFF_WORDS * 4);       // (npad > n: the host-pointer pipeline's virtual indices)
    L.o_sc2 = take(pl.glv ? (size_t)n * 16 : 0);
    L.o_digits = take((size_t)npad * nw_all * 2);
    L.o_remap = take(fxd.Ep ? (size_t)n * nw_all * 4 : 0);
    L.o_sorted = take((size_t)ns * nws * 4);
    L.o_blockcnt = take((size_t)nws * NBIN * KB2 * 4);
    L.o_binstart = take((size_t)nws * (NBIN + 1) * 4);
    L.o_tileprefix = take((size_t)nws * (NBIN + 1) * 4);
    L.o_recidx = take((size_t)ns * nws * 4);
    L.o_reckey = take((size_t)ns * nws);
    // zeroed per call, adjacent so that ONE fill (d_counts, o_zero_end - o_counts) covers them: bucket counts, the tiles' run cursors
    // (`starts`), the folded-bucket flags, the piece lengths (unused slots stay 0) and the size bins with their counters
    L.o_counts = take((size_t)total_s * 4);
    L.o_starts = take((size_t)total_s * 4);
    L.o_piecesof = take((size_t)total_s * 4);
    L.o_plen = take((size_t)slots * 4);
    L.o_bins = take(BINS_STRIDE * 4 * (hin ? K : 1u));
    L.o_zero_end = off;
    L.o_pfirst = take((size_t)total_s * 4);
    L.o_big = take((size_t)total_s * 4);
    L.o_mid = take((size_t)total_s * 4);
    L.o_pbucket = take(hin ? (size_t)slots * 4 : 0);
    L.o_carrier = take(hin ? (size_t)L.total * IO::XYZZ_WORDS * 4 : 0);
    L.o_pstart = take((size_t)slots * 4);
    L.o_order = take((size_t)slots * 4);
    L.o_partials = take((size_t)slots * IO::XYZZ_WORDS * 4);
    L.o_work = take(((size_t)L.res_pts + 2 * (size_t)L.half_pts + 64) * IO::XYZZ_WORDS * 4);
    L.o_ba_pts = take(use_ba ? (size_t)ns * nws * IO::AFF_WORDS * 4 : 0);
    L.o_ba_pref = take(use_ba ? (size_t)L.ba_pref_slots * ba_lanes * F::WORDS * 4 : 0);
    L.bytes = off;
    return 0;
  }

  // ---- the big path's stages.  Each enqueues on the stream(s) it is given and returns the call's error code (0 = fine).
  // Fixed base with several virtual windows: the digits are taken first, compacted by window (k_fixed_digits_c), and the pipeline is
  // sized by the fullest window's row, Ep, instead of by all E entries per window.  (Synchronises: the rows' counts decide the layout.)
  int fixed_compact_digits(const FixedTable& T, const uint32_t* d_scalars, uint32_t n_in, hipStream_t stream, FxDigits& fxd) {
    if (T.NV <= 2 || T.NV > 128) return 0;
    const size_t E = T.E();
    const size_t o_dg = (E + 255) & ~size_t(255), o_cnt = o_dg + ((E * 2 + 255) & ~size_t(255)), need = o_cnt + 256 * 4;
    if (need > fxs_bytes) {
      if (fxs) (void)hipFree(fxs);
      fxs = nullptr; fxs_bytes = 0;
      HIP_TRY(hipMalloc((void**)&fxs, need + need / 8), 1);
      fxs_bytes = need + need / 8;
    }
    fxd.v8 = fxs; fxd.dg = (uint16_t*)(fxs + o_dg); fxd.cnt = (uint32_t*)(fxs + o_cnt);
    HIP_TRY(hipMemsetAsync(fxd.cnt, 0, 256 * 4, stream), 1);
    hipLaunchKernelGGL((k_fixed_digits_c<SW, G::SCALAR_BITS>), dim3((T.n + 255) / 256), dim3(256), 0, stream, d_scalars, T.tinf, fxd.v8, fxd.dg, fxd.cnt, T.n,
                       n_in, T.cf, T.W, T.NV, T.M);
    uint32_t h_cnt[128];
    HIP_TRY(hipMemcpyAsync(h_cnt, fxd.cnt, T.NV * 4, hipMemcpyDeviceToHost, stream), 1);
    HIP_TRY(hipStreamSynchronize(stream), 1);
    uint32_t mx = 0;
    for (uint32_t v = 0; v < T.NV; v++) mx = h_cnt[v] > mx ? h_cnt[v] : mx;
    const uint64_t ep = ((uint64_t)mx + 4095) & ~uint64_t(4095);
    if (ep >= 4096 && ep * 2 <= E) fxd.Ep = (uint32_t)ep;       // (a window that holds most entries - tiny scalars - gains nothing: the uncompacted form)
    return 0;
  }
  // the two-level sort of the windows [wb, wb + wn) (all of them, or one pass of the host-pointer pipeline)
  void sort_windows(const BigLayout& L, uint32_t wb, uint32_t wn, hipStream_t st) {
    hipLaunchKernelGGL((k_part_hist<G>), dim3(L.KB2, wn), dim3(1024), 0, st, L.d_digits, L.d_blockcnt, L.ns, L.chunk2, L.NBIN, wb);
    hipLaunchKernelGGL((k_part_scan<G>), dim3(wn), dim3(1024), 0, st, L.d_blockcnt, L.d_binstart, L.d_tileprefix, L.NBIN, L.KB2, L.TILE, wb);
    hipLaunchKernelGGL((k_part_scatter<G>), dim3(L.KB2, wn), dim3(1024), 0, st, L.d_digits, L.d_blockcnt, L.d_recidx, L.d_reckey, L.ns, L.chunk2, L.HIB, L.NBIN, (const uint32_t*)L.d_remap, L.vw, wb);
    hipLaunchKernelGGL((k_tile_count<G>), dim3(L.max_tiles, wn), dim3(L.ts_threads), 0, st, L.d_reckey, L.d_binstart, L.d_tileprefix, L.d_counts, L.ns, L.B, L.HIB, L.NBIN, wb);
    hipLaunchKernelGGL((k_tile_sort<G>), dim3(L.max_tiles, wn), dim3(L.ts_threads), 0, st, L.d_recidx, L.d_reckey, L.d_binstart, L.d_tileprefix, L.d_counts,
                       L.d_starts, L.d_sorted, L.d_pfirst, L.d_pstart, L.d_plen, L.d_big, L.d_nbig, L.d_mid, L.d_nmid, L.ns, L.B, L.HIB, L.NBIN, L.SEG, L.PW, L.d_pbucket, L.vw, wb);
  }
  // Host-pointer pipeline.  Three streams.  Transfers on the copy stream, in this order (a pageable hipMemcpyAsync holds the
  // calling thread until its bytes have left, so every launch below is issued before the NEXT transfer starts):
  //   scalars (+ flags) of chunk 0 | bases of chunk 0 | scalars of chunk 1 | bases of chunk 1 | ...
  // behind each chunk's scalars, on the SORT stream: digits + two-level sort + longest-first schedule of the chunk's virtual windows
  // (the sort's scratch is indexed by virtual window: passes of different chunks share nothing) - it runs beside the accumulation
  // of the chunk before; behind each chunk's bases and its sort, on the call's stream: conversion + k_accumulate_chunk.  The
  // accumulation is the longer side of every stage from chunk 0 on (2^20 G1 terms: 0.61 ms per quarter against 0.58 ms of
  // transfers), so what the call pays on top of the resident pipeline is the first chunk's transfer.
  int enqueue_host_pipeline(const BigLayout& L, const HostIn& hin, const uint64_t* d_ark_bases, const uint8_t* d_inf, const uint32_t* d_scalars, hipStream_t stream) {
    hipStream_t cs = side_stream_.get(), ss = sort_stream_.get();
    //  an error return inside the chunk loop must not leave the copy and sort streams reading the caller's host buffers and the arena
    struct Drain { hipStream_t a, b, c; bool armed; ~Drain() { if (armed) { (void)hipStreamSynchronize(a); (void)hipStreamSynchronize(b); (void)hipStreamSynchronize(c); } } } drain{cs, ss, stream, true};
    const uint32_t K = L.K, cm = L.cm, nw = (uint32_t)L.nw;
    if (ev_copy.size() < 3 * (size_t)K + 1) {
      const size_t have = ev_copy.size();
      ev_copy.resize(3 * (size_t)K + 1, nullptr);
      for (size_t i = have; i < ev_copy.size(); i++) HIP_TRY(hipEventCreateWithFlags(&ev_copy[i], hipEventDisableTiming), 1);
    }
    hipEvent_t* ev_sc = ev_copy.data();             // [k]: chunk k's scalars are on the device
    hipEvent_t* ev_bs = ev_copy.data() + K;         // [k]: chunk k's bases are
    hipEvent_t* ev_so = ev_copy.data() + 2 * K;     // [k]: chunk k's runs, pieces and schedule are ready
    HIP_TRY(hipMemsetAsync(L.d_counts, 0, L.o_zero_end - L.o_counts, stream), 1);       // (the per-call fills run under the first transfer)
    HIP_TRY(hipMemsetAsync(L.d_carrier, 0, (size_t)L.total * IO::XYZZ_WORDS * 4, stream), 1);
    HIP_TRY(hipEventRecord(ev_copy[3 * K], stream), 1);
    HIP_TRY(hipStreamWaitEvent(ss, ev_copy[3 * K], 0), 1);
    constexpr size_t PT_BYTES = 2 * (size_t)IO::ARK64 * 8;
    const uint32_t cslots = nw * L.PW;
    ArkCoord<IO::ARK64> ark_one;
    F::one().to_ark(ark_one.v);
    if (hin.ark_zero && d_inf != d_in_inf) return 2;       // (the flags are written into the engine's own buffer)
    size_t hlo = 0;                                  // the chunk's first point in the caller's arrays
    for (uint32_t k = 0; k < K; hlo += L.clen[k], k++) {
      const size_t lo = (size_t)k * cm, cnt = L.clen[k];      // ... and on the device (virtual index)
      // (the prover's queries - hin.ark_zero: a base row (0, 1) is the identity - need the chunk's bases before its digits: bases first)
      if (hin.ark_zero) {
        HIP_TRY(hipMemcpyAsync((char*)d_ark_bases + lo * PT_BYTES, (const char*)hin.bases + hlo * PT_BYTES, cnt * PT_BYTES, hipMemcpyHostToDevice, cs), 1);
        HIP_TRY(hipEventRecord(ev_bs[k], cs), 1);
      }
      // scalars -> digits, sort, schedule (sort stream)
      HIP_TRY(hipMemcpyAsync((char*)d_scalars + lo * SW * 4, (const char*)hin.scalars + hlo * SW * 4, cnt * SW * 4, hipMemcpyHostToDevice, cs), 1);
      if (hin.inf) HIP_TRY(hipMemcpyAsync((char*)d_inf + lo, hin.inf + hlo, cnt, hipMemcpyHostToDevice, cs), 1);
      HIP_TRY(hipEventRecord(ev_sc[k], cs), 1);
      HIP_TRY(hipStreamWaitEvent(ss, ev_sc[k], 0), 1);
      if (hin.ark_zero) {
        HIP_TRY(hipStreamWaitEvent(ss, ev_bs[k], 0), 1);
        hipLaunchKernelGGL((k_flag_ark_zero<G>), dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, ss, d_ark_bases + lo * 2 * IO::ARK64,
                           hin.inf ? d_inf + lo : nullptr, d_in_inf + lo, cnt, ark_one);
      }
      if (launch_digits<SW, G::SCALAR_BITS>(L.pl.c, d_scalars, d_inf, L.d_digits_all, (uint32_t)(lo + cnt), ss, cm, (k + 1) * cm, k * cm)) return 3;    // (lanes behind the chunk's last point: "no digit")
      sort_windows(L, k * nw, nw, ss);
      uint32_t* bins_k = L.d_bins + (size_t)k * BINS_STRIDE;       // longest-first schedule over the chunk's own slots (its virtual windows are adjacent)
      hipLaunchKernelGGL((k_size_hist<G>), dim3(cslots / 256 < 512 ? (cslots + 255) / 256 : 512), dim3(256), 0, ss, L.d_plen + (size_t)k * cslots, bins_k, cslots);
      hipLaunchKernelGGL((k_size_scan<G>), dim3(1), dim3(1024), 0, ss, bins_k, bins_k + SIZE_BINS);
      hipLaunchKernelGGL((k_size_scatter<G>), dim3((cslots + 4095) / 4096), dim3(1024), 0, ss, L.d_plen + (size_t)k * cslots, bins_k, L.d_order + (size_t)k * cslots, cslots);
      HIP_TRY(hipEventRecord(ev_so[k], ss), 1);
      if (k == 0) {
        HIP_TRY(hipStreamWaitEvent(stream, ev_so[0], 0), 1);
        HIP_TRY(hipEventRecord(ev[1], stream), 1);      // ("convert" = chunk 0's scalars, digits, sort and schedule; "sort" is empty on this path;
        HIP_TRY(hipEventRecord(ev[2], stream), 1);      //  "accumulate" = everything from here to the last chunk's end)
      }
      // bases -> conversion, accumulation (the call's stream)
      if (!hin.ark_zero) {
        HIP_TRY(hipMemcpyAsync((char*)d_ark_bases + lo * PT_BYTES, (const char*)hin.bases + hlo * PT_BYTES, cnt * PT_BYTES, hipMemcpyHostToDevice, cs), 1);
        HIP_TRY(hipEventRecord(ev_bs[k], cs), 1);
      }
      HIP_TRY(hipStreamWaitEvent(stream, ev_bs[k], 0), 1);
      if (k) HIP_TRY(hipStreamWaitEvent(stream, ev_so[k], 0), 1);
      hipLaunchKernelGGL((k_convert_bases<G>), dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, stream, d_ark_bases + lo * 2 * IO::ARK64, L.d_bases + lo * IO::AFF_WORDS, cnt);
      hipLaunchKernelGGL((k_accumulate_chunk<G>), dim3((cslots + 255) / 256), dim3(256), 0, stream, L.d_bases, L.d_sorted, L.d_pstart + (size_t)k * cslots, L.d_plen + (size_t)k * cslots,
                         L.d_order + (size_t)k * cslots, bins_k + SIZE_BINS, L.d_partials + (size_t)k * cslots * IO::XYZZ_WORDS, L.d_pbucket + (size_t)k * cslots, L.d_carrier, k ? 1u : 0u);
    }
    drain.armed = false;
    return 0;
  }
  // Inputs resident on the device: conversion (or GLV expansion; fixed base: nothing - the table is in device form), digits in one of
  // four forms, the sort, the longest-first schedule, the accumulation (XYZZ chain, or batched-affine pre-levels first).
  // (Measured level twice and gone - round 4 for window shards, round 6 for whole MSMs: the conversion on a second stream beside the sort.)
  int enqueue_resident(const BigLayout& L, const uint64_t* d_ark_bases, const uint8_t* d_inf, const uint32_t* d_scalars, hipStream_t stream) {
    const FixedTable* fx = L.fx;
    const uint32_t n = L.pl.n, slots = L.slots;
    const int c = L.pl.c, nw_all = L.pl.nw;
    if (L.pl.glv) GlvExpand<G>::launch(d_ark_bases, d_inf, d_scalars, L.n_in, L.d_bases, L.d_sc2, stream);
    else if (!fx) hipLaunchKernelGGL((k_convert_bases<G>), dim3((n + 255) / 256), dim3(256), 0, stream, d_ark_bases, L.d_bases, (size_t)n);
    HIP_TRY(hipEventRecord(ev[1], stream), 1);
    // ---- sort
    if (fx && L.fxd.Ep) {
      HIP_TRY(hipMemsetAsync(L.d_digits_all, 0xFF, (size_t)n * nw_all * 2, stream), 1);             // every slot "no digit" until a record lands in it
      HIP_TRY(hipMemsetAsync(L.fxd.cnt + 128, 0, 128 * 4, stream), 1);                               // the rows' cursors
      const uint32_t E32 = (uint32_t)fx->E();
      hipLaunchKernelGGL((k_fixed_place<G>), dim3((E32 + 1023) / 1024 < 4096 ? (E32 + 1023) / 1024 : 4096), dim3(1024), 0, stream, L.fxd.v8, L.fxd.dg, L.fxd.cnt + 128, L.d_digits_all,
                         L.d_remap, E32, n, fx->NV);
    } else if (fx) hipLaunchKernelGGL((k_fixed_digits<SW, G::SCALAR_BITS>), dim3((fx->n + 255) / 256), dim3(256), 0, stream, d_scalars, fx->tinf, L.d_digits_all, fx->n, L.n_in,
                               fx->cf, fx->W, fx->NV, fx->M);
    else if (L.pl.glv) { if (launch_digits<4, GlvExpand<G>::BITS>(c, (const uint32_t*)L.d_sc2, nullptr, L.d_digits_all, n, stream)) return 3; }
    else if (launch_digits<SW, G::SCALAR_BITS>(c, d_scalars, d_inf, L.d_digits_all, n, stream)) return 3;
    HIP_TRY(hipMemsetAsync(L.d_counts, 0, L.o_zero_end - L.o_counts, stream), 1);
    sort_windows(L, 0, (uint32_t)L.nw, stream);
    // ---- work items, longest first
    hipLaunchKernelGGL((k_size_hist<G>), dim3(slots / 256 < 512 ? (slots + 255) / 256 : 512), dim3(256), 0, stream, L.d_plen, L.d_bins, slots);
    hipLaunchKernelGGL((k_size_scan<G>), dim3(1), dim3(1024), 0, stream, L.d_bins, L.d_nwork);
    hipLaunchKernelGGL((k_size_scatter<G>), dim3((slots + 4095) / 4096), dim3(1024), 0, stream, L.d_plen, L.d_bins, L.d_order, slots);
    HIP_TRY(hipEventRecord(ev[2], stream), 1);
    // ---- accumulate (grid covers every slot; lanes beyond the number of non-empty pieces exit)
    if constexpr (BaCfg<G>::enabled) if (L.use_ba) {
      hipLaunchKernelGGL((k_ba_levels<G, BA_OCC>), dim3(L.ba_lanes / 256), dim3(256), 0, stream, L.d_bases, L.d_sorted, L.d_pstart, L.d_plen, L.d_order, L.d_nwork, L.d_ba_pts,
                         L.d_ba_pref, L.ba_lanes, BA_LEVELS, L.ba_pref_slots);
      hipLaunchKernelGGL((k_accumulate_ba<G>), dim3((slots + 255) / 256), dim3(256), 0, stream, L.d_ba_pts, L.d_pstart, L.d_plen, L.d_order, L.d_nwork, L.d_partials, BA_LEVELS);
    }
    if (!L.use_ba) launch_accumulate<G>(slots, stream, L.d_bases, L.d_sorted, L.d_pstart, L.d_plen, L.d_order, L.d_nwork, L.d_partials);
    return 0;
  }
  // Bucket reduction: the buckets cut into pieces are folded (k_combine_mid_lanes, k_combine_big; host-pointer pipeline: the pieces join
  // the carrier table, k_merge_carried), then the bit-sliced reduction's LB launches (msm_reduce.h) and the results' conversion.
  int enqueue_bucket_reduction(const BigLayout& L, hipStream_t stream) {
    const uint32_t total = L.total, SEG = L.SEG, B = L.B, res_pts = L.res_pts, nw = (uint32_t)L.nw;
    const int LB = L.LB;
    // (a window shard cuts EVERY bucket in two or three: one group of lanes per bucket of the call, not 21504 groups striding over them)
    const uint32_t mid_blocks = L.shard ? (total + 20) / 21 < 16384 ? (total + 20) / 21 : 16384 : 1024;
    const uint32_t cfirst = L.hin ? 1u : 0u;      // host-pointer pipeline: a bucket's first piece is its carrier and stays out of the folds
    hipLaunchKernelGGL((k_combine_mid_lanes<G>), dim3(mid_blocks), dim3(64), 0, stream, L.d_mid, L.d_nmid, L.d_counts, L.d_pfirst, L.d_partials, L.d_piecesof, SEG, cfirst);
    hipLaunchKernelGGL((k_combine_big<G>), dim3(256), dim3(256), 0, stream, L.d_big, L.d_nbig, L.d_counts, L.d_pfirst, L.d_partials, L.d_piecesof, SEG, cfirst);
    // the leaves of the reduction: the buckets' pieces, or (host-pointer pipeline) the carrier table, one slot per bucket
    const uint32_t* d_leaf = L.d_partials;
    const uint32_t* d_leaf_counts = L.d_counts;
    if (L.hin) {
      hipLaunchKernelGGL((k_merge_carried<G>), dim3((total + 127) / 128), dim3(128), 0, stream, L.d_counts, L.d_pfirst, L.d_partials, L.d_carrier, total, L.K, SEG);
      d_leaf = L.d_carrier; d_leaf_counts = nullptr;
    }
    // work area (in points): [0, res_pts) results, then two launch-alternating halves of half_pts
    struct Arr { uint32_t at, per_window; bool born; int level; };  // `born`: odd list not yet halved (read strided from its level)
    uint32_t half_at[2] = {res_pts, res_pts + L.half_pts};
    Arr tree = {0, B, true, LB};            // current tree level (level LB = the buckets themselves)
    std::vector<Arr> lists;                 // pending odd lists
    for (int t = 1; t <= LB; t++) {
      BitsumJobs jobs;
      jobs.njobs = 0;
      uint32_t cursor = half_at[t & 1], total_out = 0;
      auto push = [&](uint32_t src, uint32_t outs_per_window, uint32_t mode, int result_slot) -> uint32_t {
        const uint32_t outs = outs_per_window * nw;
        uint32_t dst;
        if (result_slot >= 0) dst = (uint32_t)result_slot * nw;
        else { dst = cursor; cursor += outs; }
        const int j = (int)jobs.njobs++;
        total_out += outs;
        jobs.end[j] = total_out; jobs.src[j] = src; jobs.dst[j] = dst; jobs.mode[j] = mode;
        return dst;
      };
      std::vector<Arr> next_lists;
      // the odd list of the current tree level is born now (level >= 2: at least two odd nodes per window)
      if (tree.level >= 2) {
        const uint32_t outs = tree.per_window / 4;
        const uint32_t dst = push(tree.at, outs, tree.level == LB ? 3u : 1u, outs == 1 ? tree.level : -1);
        if (outs > 1) next_lists.push_back({dst, outs, false, tree.level});
      } else {  // level 1: O_1 = node(1, 1)
        push(tree.at, 1, 4u, 1);
      }
      for (const Arr& A : lists) {
        const uint32_t outs = A.per_window / 2;
        const uint32_t dst = push(A.at, outs, 0u, outs == 1 ? A.level : -1);
        if (outs > 1) next_lists.push_back({dst, outs, false, A.level});
      }
      {  // next tree level
        const uint32_t outs = tree.per_window / 2;
        const uint32_t dst = push(tree.at, outs, tree.level == LB ? 2u : 0u, outs == 1 ? 0 : -1);
        tree = {dst, outs, true, tree.level - 1};
      }
      lists.swap(next_lists);
      // the late levels - launches of few outputs, i.e. latency - on three lanes per addition
      if (total_out <= BITSUM_LANES_MAX)
        hipLaunchKernelGGL((k_bitsum_lanes<G>), dim3((total_out + 20) / 21), dim3(64), 0, stream, d_leaf, d_leaf_counts, L.d_pfirst, L.d_piecesof, SEG, L.d_work, jobs);
      else
        hipLaunchKernelGGL((k_bitsum<G>), dim3((total_out + 127) / 128), dim3(128), 0, stream, d_leaf, d_leaf_counts, L.d_pfirst, L.d_piecesof, SEG,
                           L.d_work, jobs);
    }
    hipLaunchKernelGGL((k_results_to_ark<G>), dim3((4 * res_pts + 63) / 64), dim3(64), 0, stream, L.d_work, res_pts);
    return 0;
  }
  // the results to the pinned host buffer; waits for the call's device work and takes its timings
  int fetch_results(const BigLayout& L, hipStream_t stream) {
    HIP_TRY(hipEventRecord(ev[4], stream), 1);
    HIP_TRY(hipMemcpyAsync(h_out, L.d_work, (size_t)L.res_pts * IO::XYZZ_WORDS * 4, hipMemcpyDeviceToHost, stream), 1);
    HIP_TRY(hipEventRecord(ev[5], stream), 1);
    HIP_TRY(hipStreamSynchronize(stream), 1);
    HIP_TRY(hipGetLastError(), 1);
    read_timings(tm);
    last_c = L.pl.c; last_nw = L.nw; last_buckets = L.total; last_glv = L.pl.glv;
    return 0;
  }

  // ---- host epilogue: total = sum_w 2^(c w) (node_w + sum_l 2^(LB-l) O_{w,l}): one Horner pass, c doublings and c additions per
  // window (the results arrive as arkworks limbs), as a list of steps: on AVX-512 IFMA where the CPU has it (host_ifma.cpp: the
  // products of one point operation eight at a time, 0.24 -> ~0.1 ms for 253-bit scalars), else - or if that path meets equal or
  // opposite operands, which it does not handle - on 64-bit limbs (host64.h)
  void build_horner_steps(const BigLayout& L) {
    const int nw = L.nw, LB = L.LB;
    horner_steps.clear();
    if (L.fx) {
      // total = sum_v c_v node_v + sum_l 2^(15 - l) (sum_v O_{v,l}) + sum_v node_v,  c_v = v M: ONE chain over the bit positions t from the top
      // of the largest c_v down to 0 - at step t the accumulator doubles, then takes node_v of every v with bit t of c_v set and, for
      // t <= 14, the O_{v, 15 - t} of every virtual window
      const uint32_t M = L.fx->M;
      int top = LB - 1;
      while (((uint64_t)(nw - 1) * M) >> (top + 1)) top++;
      for (int t = top; t >= 0; t--) {
        horner_steps.push_back(-1);
        for (int v = 0; v < nw; v++) if ((((uint64_t)v * M) >> t) & 1) horner_steps.push_back(v | HORNER_NODBL);
        if (t <= LB - 1) for (int v = 0; v < nw; v++) horner_steps.push_back(((LB - t) * nw + v) | HORNER_NODBL);
      }
      for (int v = 0; v < nw; v++) horner_steps.push_back(v | HORNER_NODBL);
      return;
    }
    const int narrow_from = L.pl.nw - L.pl.kn;                   // the top kn of the plan's windows are c - 1 bits wide (k_digits)
    for (int w = nw - 1; w >= 0; w--) {
      horner_steps.push_back(-1);
      for (int l = (L.w0 + w >= narrow_from ? 2 : 1); l <= LB; l++) horner_steps.push_back(l * nw + w);
      horner_steps.push_back(w | HORNER_NODBL);
    }
  }
  HXyzz<HostF> run_horner_steps(const int32_t* steps, int count) const {
    const uint64_t* h64 = reinterpret_cast<const uint64_t*>(h_out);
    constexpr size_t PT64 = (size_t)IO::XYZZ_WORDS / 2;
    if (IfmaHorner<F>::fn && celo_ifma_available()) {
      uint64_t r[4 * IO::ARK64];
      int inf = 0;
      if (IfmaHorner<F>::fn(h64, PT64, steps, count, r, &inf) == 0) return inf ? HXyzz<HostF>::identity() : HXyzz<HostF>::load(r, IO::ARK64);
    }
    return host64_horner<HostF>(h64, PT64, IO::ARK64, steps, count);
  }
  // The pass is linear in its windows: a group of windows run from the identity gives P_j, and the whole is ((P_0 2^d1 + P_1) 2^d2 +
  // P_2) ... with d_j the doublings of group j's steps.  For the fields whose host products are slow - Fq2 (three 6-limb products and
  // their reductions per product: 0.65 ms of every G2 call) and the 12-limb field of BW6-761 (0.6-0.8 ms) - the window groups run on
  // HOST_HORNER_THREADS threads side by side and only the joining doublings stay serial: 0.65 -> 0.3 ms per G2 MSM, more than a
  // quarter of a call below 2^16 terms.  The 6-limb prime field stays on one thread (0.15 ms: the joins would cost what the split saves).
  static constexpr int HT = (sizeof(HostF) > 6 * 8) ? HOST_HORNER_THREADS : 1;
  // the step list cut into HT groups [start[j], start[j + 1])
  void split_horner_steps(bool fixed, int nw, int* start) const {
    const int count = (int)horner_steps.size();
    int g = 0;
    start[0] = 0;
    if (fixed) {
      // fixed base (late round 4): the chain over the bit positions is linear in them too - a group of consecutive positions run from
      // the identity gives P_j and the join is the same.  Cut BEFORE a doubling step, balancing the additions (the 15 positions that
      // take every virtual window's level sums carry most of them): 0.8 -> 0.4 ms of BW6-761 host work per call at cf = 20.
      int adds_total = 0, adds = 0;
      for (int k = 0; k < count; k++) adds_total += horner_steps[k] >= 0 ? 1 : 0;
      for (int k = 0; k < count; k++) {
        if (horner_steps[k] < 0 && g + 1 < HT && k > start[g] && adds * HT >= (g + 1) * adds_total) start[++g] = k;
        adds += horner_steps[k] >= 0 ? 1 : 0;
      }
      while (g + 1 < HT) start[++g] = count;       // (fewer cuts than threads: empty groups, the identity)
    } else {   // window boundaries in the step list: a window's steps end with its NODBL entry
      int wdone = 0;
      for (int k = 0; k < count; k++) {
        if (horner_steps[k] >= 0 && (horner_steps[k] & HORNER_NODBL)) {
          wdone++;
          if (wdone == (g + 1) * nw / HT && g + 1 < HT) start[++g] = k + 1;
        }
      }
    }
    start[HT] = count;
  }
  void host_epilogue(const BigLayout& L, uint64_t* out_jac, uint64_t* out_xyzz) {
    build_horner_steps(L);
    HXyzz<HostF> total_pt;
    if (HT > 1 && (L.fx ? horner_steps.size() >= 64 : L.nw >= 2 * HT)) {
      int start[HT + 1], dbls[HT];
      split_horner_steps(L.fx != nullptr, L.nw, start);
      for (int j = 0; j < HT; j++) {
        dbls[j] = 0;
        for (int k = start[j]; k < start[j + 1]; k++) if (horner_steps[k] < 0 || !(horner_steps[k] & HORNER_NODBL)) dbls[j]++;
      }
      HXyzz<HostF> part[HT];
      std::thread th[HT - 1];
      bool started[HT - 1];
      for (int j = 1; j < HT; j++) {
        started[j - 1] = true;
        try { th[j - 1] = std::thread([&, j] { part[j] = run_horner_steps(horner_steps.data() + start[j], start[j + 1] - start[j]); }); }
        catch (const std::system_error&) { started[j - 1] = false; }      // no thread to be had: that group runs here, serially
      }
      part[0] = run_horner_steps(horner_steps.data() + start[0], start[1] - start[0]);
      for (int j = 1; j < HT; j++) {
        if (started[j - 1]) th[j - 1].join();
        else part[j] = run_horner_steps(horner_steps.data() + start[j], start[j + 1] - start[j]);
      }
      total_pt = part[0];
      for (int j = 1; j < HT; j++) {
        for (int d = 0; d < dbls[j]; d++) total_pt = hxyzz_dbl(total_pt);
        hxyzz_add(total_pt, part[j]);
      }
    } else {
      total_pt = run_horner_steps(horner_steps.data(), (int)horner_steps.size());
    }
    if (out_xyzz) {
      if (total_pt.is_identity()) memset(out_xyzz, 0, 4 * IO::ARK64 * 8);
      else { total_pt.X.store(out_xyzz); total_pt.Y.store(out_xyzz + IO::ARK64); total_pt.ZZ.store(out_xyzz + 2 * IO::ARK64); total_pt.ZZZ.store(out_xyzz + 3 * IO::ARK64); }
    }
    if (out_jac) write_host_jacobian(total_pt, out_jac);
  }

  // ---- host-pointer entry: the pipelined form (run_device_windows' HostIn) from 2^18 terms up, in chunks of at least 2^17 points (the prover's
  // entry points - ark_zero_identity: the flags come from the bases - send a chunk's bases before its scalars); the GLV split (its expansion
  // reads bases and scalars together) and window shards keep the plain form: three transfers, then the resident pipeline
  struct HostChunks { bool pipelined; uint32_t chunks, head_split, tail_split; size_t need; };     // need: staging capacity in points
  HostChunks host_chunk_choice(size_t n, int win_cnt) const {
    const int ovr = host_chunks_override().load();
    // chunk count by size: about 2^18 points per chunk within [4, 16] ([8, 16] BW6-761; 2^19 within [4, 8] for the Fq2 group) - the sweeps behind
    // these bounds: DESIGN.md section 4 "Host-pointer pipeline: chunk-count measurements"
    const bool fq2_group = sizeof(F) > 14 * sizeof(uint32_t) && G::SCALAR_BITS <= 256;
    uint32_t by_size = (uint32_t)(n >> (fq2_group ? 19 : 18));
    const uint32_t lo_k = G::SCALAR_BITS > 256 ? 8u : 4u, hi_k = fq2_group ? 8u : 16u;
    by_size = by_size < lo_k ? lo_k : by_size > hi_k ? hi_k : by_size;
    HostChunks hc;
    hc.chunks = ovr >= 0 ? (uint32_t)(ovr & 0xFF) : MsmTuning::get().host_chunks != 0xFFFFFFFFu ? MsmTuning::get().host_chunks : by_size;
    // how often the first / the last chunk is cut in halves: celo_amd_msm_set_host_chunks carries them, else the defaults
    const bool head_set = ovr >= 0 && ((ovr >> 8) & 15), tail_set = ovr >= 0 && ((ovr >> 12) & 15);
    hc.head_split = head_set ? (uint32_t)((ovr >> 8) & 15) - 1u : HOST_HEAD_SPLIT_DEFAULT;
    hc.tail_split = tail_set ? (uint32_t)((ovr >> 12) & 15) - 1u : HOST_TAIL_SPLIT_DEFAULT;
    if (hc.chunks > 64) hc.chunks = 64;
    // chunks of at least 2^17 points (2^16 when the count was set by hand - tests): a chunk's sort pass and the accumulation's last round are
    // fixed costs of ~0.08 ms (same DESIGN subsection)
    const size_t min_chunk_log = ovr >= 0 ? 16 : 17;
    if (hc.chunks > (n >> min_chunk_log)) hc.chunks = (uint32_t)(n >> min_chunk_log);
    // (the prover's four concurrent MSMs hide each other's transfers: pipelined only from 2^21 rows per query; the subgroup entry's GLV split
    // reads bases and scalars together and is not pipelined: from 2^19 terms a host-pointer call takes the pipelined PLAIN form instead - same
    // group element; both measured, same DESIGN subsection)
    const bool glv_plan = plan(n).glv;
    const bool glv_off = glv_plan && !ark_zero_identity && !win_cnt && n >= (size_t(1) << 19);
    // (the default head split only where its halves keep 2^17 points)
    if (!head_set && hc.chunks && n / hc.chunks < (size_t(1) << 18)) hc.head_split = 0;
    hc.pipelined = hc.chunks >= (ovr >= 0 ? 1u : 2u) && !win_cnt && (!glv_plan || glv_off) && n < (size_t(1) << 30) && (!ark_zero_identity || ovr >= 0 || n >= (size_t(1) << 21));
    hc.need = n;
    if (hc.pipelined) {      // the pipelined form addresses chunk k at k cm
      uint32_t cm, clen[HOST_CHUNKS_MAX];
      hc.need = (size_t)host_chunk_plan(n, hc.chunks, hc.head_split, hc.tail_split, cm, clen) * cm;
      // (the pipelined run takes no GLV split - the window count checked here is the one it will use; the holes would overflow the
      // 32-bit run offsets: plain form)
      if ((uint64_t)hc.need * (uint64_t)plan(n, false).nw >= (uint64_t(1) << 32)) { hc.pipelined = false; hc.need = n; }
    }
    return hc;
  }
  // the (cached) staging buffers of the host-pointer entry, for `need` points
  void free_staging() {
    for (void* p : {(void*)d_in_bases, (void*)d_in_scalars, (void*)d_in_inf}) if (p) (void)hipFree(p);
    d_in_bases = nullptr; d_in_scalars = nullptr; d_in_inf = nullptr; cap_in = 0;
  }
  int reserve_staging(size_t need) {
    if (need <= cap_in) return 0;
    free_staging();
    HIP_TRY(hipMalloc(&d_in_bases, need * 2 * IO::ARK64 * 8), 1);
    HIP_TRY(hipMalloc(&d_in_scalars, need * SW * 4), 1);
    HIP_TRY(hipMalloc(&d_in_inf, need), 1);
    cap_in = need;
    return 0;
  }

  int ensure(size_t bytes) {
    if (!ev[0]) for (int i = 0; i < 6; i++) HIP_TRY(hipEventCreate(&ev[i]), 1);
    if (!h_out) HIP_TRY(hipHostMalloc(&h_out, H_OUT_POINTS * IO::XYZZ_WORDS * 4), 1);
    if (bytes > arena_bytes) {
      if (arena) (void)hipFree(arena);
      arena = nullptr; arena_bytes = 0;
      HIP_TRY(hipMalloc(&arena, bytes), 1);
      arena_bytes = bytes;
    }
    return 0;
  }

  template <int SWX, int CB, int PT> int launch_batch_sort_cp(const uint32_t* sc, const uint8_t* inf, const uint32_t* off, uint32_t* sorted,
                                                     uint32_t* pstart, uint32_t* plen, uint32_t m, int nw, hipStream_t st) {
    hipLaunchKernelGGL((k_batch_sort<SWX, CB, PT>), dim3(m), dim3(256), 0, st, sc, inf, off, sorted, pstart, plen, nw);
    return 0;
  }
  template <int SWX, int CB> int launch_batch_sort_c(uint32_t max_n, const uint32_t* sc, const uint8_t* inf, const uint32_t* off, uint32_t* sorted,
                                            uint32_t* pstart, uint32_t* plen, uint32_t m, int nw, hipStream_t st) {
    if (max_n <= 256) return launch_batch_sort_cp<SWX, CB, 1>(sc, inf, off, sorted, pstart, plen, m, nw, st);
    if (max_n <= 512) return launch_batch_sort_cp<SWX, CB, 2>(sc, inf, off, sorted, pstart, plen, m, nw, st);
    return launch_batch_sort_cp<SWX, CB, 4>(sc, inf, off, sorted, pstart, plen, m, nw, st);
  }
  template <int SWX> int launch_batch_sort(int c, uint32_t max_n, const uint32_t* sc, const uint8_t* inf, const uint32_t* off, uint32_t* sorted,
                        uint32_t* pstart, uint32_t* plen, uint32_t m, int nw, hipStream_t st) {
    switch (c) {
      case 3: return launch_batch_sort_c<SWX, 3>(max_n, sc, inf, off, sorted, pstart, plen, m, nw, st);
      case 4: return launch_batch_sort_c<SWX, 4>(max_n, sc, inf, off, sorted, pstart, plen, m, nw, st);
      case 5: return launch_batch_sort_c<SWX, 5>(max_n, sc, inf, off, sorted, pstart, plen, m, nw, st);
      case 6: return launch_batch_sort_c<SWX, 6>(max_n, sc, inf, off, sorted, pstart, plen, m, nw, st);
      case 7: return launch_batch_sort_c<SWX, 7>(max_n, sc, inf, off, sorted, pstart, plen, m, nw, st);
      default: return 1;
    }
  }
  template <int SWX, int BITS, int CB> int launch_digits_c(const uint32_t* sc, const uint8_t* inf, uint16_t* digits, uint32_t n, hipStream_t st, uint32_t m, uint32_t npad, uint32_t ibase) {
    constexpr int NW = (BITS + CB) / CB;
    constexpr int KN = NW * CB - (BITS + 1);     // 0 <= KN < CB <= NW for every window size in use
    if constexpr (KN > 0 && KN < NW) {
      if (narrow_top(CB)) { hipLaunchKernelGGL((k_digits<SWX, CB, NW, KN, BITS>), dim3((npad - ibase + 255) / 256), dim3(256), 0, st, sc, inf, digits, n, m, npad, ibase); return 0; }
    }
    hipLaunchKernelGGL((k_digits<SWX, CB, NW, 0, BITS>), dim3((npad - ibase + 255) / 256), dim3(256), 0, st, sc, inf, digits, n, m, npad, ibase);
    return 0;
  }
  // m, npad: the chunked layout (k_digits); 0 = plain
  template <int SWX, int BITS> int launch_digits(int c, const uint32_t* sc, const uint8_t* inf, uint16_t* digits, uint32_t n, hipStream_t st, uint32_t m = 0, uint32_t npad = 0, uint32_t ibase = 0) {
    if (!m) { m = n; npad = n; }
    switch (c) {
      case 4: return launch_digits_c<SWX, BITS, 4>(sc, inf, digits, n, st, m, npad, ibase);
      case 5: return launch_digits_c<SWX, BITS, 5>(sc, inf, digits, n, st, m, npad, ibase);
      case 6: return launch_digits_c<SWX, BITS, 6>(sc, inf, digits, n, st, m, npad, ibase);
      case 7: return launch_digits_c<SWX, BITS, 7>(sc, inf, digits, n, st, m, npad, ibase);
      case 8: return launch_digits_c<SWX, BITS, 8>(sc, inf, digits, n, st, m, npad, ibase);
      case 9: return launch_digits_c<SWX, BITS, 9>(sc, inf, digits, n, st, m, npad, ibase);
      case 10: return launch_digits_c<SWX, BITS, 10>(sc, inf, digits, n, st, m, npad, ibase);
      case 11: return launch_digits_c<SWX, BITS, 11>(sc, inf, digits, n, st, m, npad, ibase);
      case 12: return launch_digits_c<SWX, BITS, 12>(sc, inf, digits, n, st, m, npad, ibase);
      case 13: return launch_digits_c<SWX, BITS, 13>(sc, inf, digits, n, st, m, npad, ibase);
      case 14: return launch_digits_c<SWX, BITS, 14>(sc, inf, digits, n, st, m, npad, ibase);
      case 15: return launch_digits_c<SWX, BITS, 15>(sc, inf, digits, n, st, m, npad, ibase);
      case 16: return launch_digits_c<SWX, BITS, 16>(sc, inf, digits, n, st, m, npad, ibase);
      default: return 1;
    }
  }
};


}  // namespace celo
