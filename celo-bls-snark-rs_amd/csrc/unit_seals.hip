// Translation unit: masked segmented point sums (aggregate.h) for BLS12-377 G1 and G2 - the aggregated key of every seal of a batch from
// its signer bitmap - normalised to affine rows on the device, and aggregated seals to verdicts on top of them: sums -> signatures decoded
// and subgroup-checked (unit_wire.hip) -> message hashes (unit_hash.hip) -> pairs packed into the pairing engine's slots -> products.
// DESIGN.md section 6j.
#include "aggregate.h"
#include "groth16_verify.h"
#include "normalize.h"
#include <hip/hip_runtime.h>
#include <cstring>
#include <mutex>
#include <vector>
#include "runtime.h"
#include "units.h"

namespace celo {

// calls from several host threads are serialised per process (bulk calls: one fills the GPU).  Guards the settings g_agg_lanes and g_agg_complement
static std::mutex agg_mu;
static int g_agg_lanes = 0;                  // 0 = the rule (agg_pick_lanes), else 1, 2, 4, .. 64 (celo_amd_aggregate_set_lanes)
static int g_agg_complement = -1;            // -1 = the rule (agg_side), 0 never, 1 always on the shared-set form (celo_amd_aggregate_set_complement)
static constexpr int AGG_BLOCK = 64;         // one wave per workgroup: 64 / L sums each
// the last call's record (celo_amd_seals_last): the times of include/celo_bls_amd.h, tag[0] the path, tag[1] the lane width; published on every exit
static Last<CallTimes> g_agg_last;

// where seal i reads: per-seal sets (shared_n == ~0u) rows and bytes [off[i], off[i+1]); the shared set rows off[0] .. and bytes i n ..
struct AggSpan { uint32_t row0, n; size_t bit0; };
__device__ __forceinline__ AggSpan agg_span(const uint32_t* __restrict__ off, uint32_t shared, uint32_t i) {
  if (shared) return {off[0], off[1] - off[0], (size_t)i * (off[1] - off[0])};
  return {off[i], off[i + 1] - off[i], (size_t)off[i]};
}

// lane i -> seal i: its count, its side, and into info[0] the largest number of rows a seal adds, into info[1] whether any seal took the
// complement (the set's total is computed only then)
__global__ void __launch_bounds__(256) k_seal_count(const uint32_t* __restrict__ off, uint32_t shared, const uint8_t* __restrict__ bits, uint32_t m, int mode,
                                                    uint32_t* __restrict__ count, uint8_t* __restrict__ side, uint32_t* __restrict__ info) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const AggSpan sp = agg_span(off, shared, i);
  const uint32_t c = agg_count(bits + sp.bit0, sp.n);
  const bool neg = agg_side(c, sp.n, mode, shared != 0);
  count[i] = c;
  side[i] = neg ? 1 : 0;
  atomicMax(&info[0], neg ? sp.n - c : c);
  if (neg) atomicOr(&info[1], 1u);
}

// L lanes per sum, 64 / L sums per workgroup (aggregate.h).  side == null: every row of rows [off[0], off[1]) into ONE sum (the set's
// total; m = 1).  out: m XYZZ points of 4 F::WORDS words.  The fold buffer is the dynamic LDS: 64 slots of agg_slot_words<F>() words (L > 1).
template <class F>
__global__ void __launch_bounds__(AGG_BLOCK) k_masked_sum(const uint64_t* __restrict__ xy, const uint8_t* __restrict__ inf, const uint32_t* __restrict__ off,
                                                          uint32_t shared, const uint8_t* __restrict__ bits, const uint8_t* __restrict__ side,
                                                          const uint32_t* __restrict__ total, uint32_t m, uint32_t L, uint32_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t agg_lds[];
  constexpr int A = F::ARK64, FW = F::WORDS;
  const uint32_t lane = threadIdx.x & (L - 1), i = blockIdx.x * (AGG_BLOCK / L) + threadIdx.x / L;
  const bool live = i < m;
  bool neg = false;
  Xyzz<F> acc = Xyzz<F>::identity();
  if (live) {
    const AggSpan sp = agg_span(off, shared, i);
    neg = side && side[i];
    acc = agg_lane_sum<F>(xy + (size_t)sp.row0 * 2 * A, inf ? inf + sp.row0 : nullptr, side ? bits + sp.bit0 : nullptr, sp.n, lane, L, neg);
  }
  if (L > 1) {                                // every lane of the workgroup walks the rounds: the barriers are outside the lane tests
    uint32_t* mine = agg_lds + (size_t)threadIdx.x * agg_slot_words<F>();
    agg_store<F>(mine, acc);
    for (uint32_t s = L >> 1; s; s >>= 1) {
      __syncthreads();
      if (lane < s) {
        agg_fold_step<F>(acc, mine, 0, s);    // `mine` is slot `lane` of this sum: its partner is s slots on
        if (s > 1) agg_store<F>(mine, acc);   // read this round: slots [s, 2 s); written: slots [0, s)
      }
    }
  }
  if (live && lane == 0) {
    agg_finish<F>(acc, neg, total);
    agg_store<F>(out + (size_t)i * 4 * FW, acc);
  }
}

// ---- one group.  Everything but `offsets` on the device, enqueued on s; returns after the stream has drained (one round trip in the
// middle: the lane width follows the counts).  d_count: m words (the counts stay there for the caller).
template <class F> struct Agg {
  static constexpr int A = F::ARK64, FW = F::WORDS;
  static int run(const uint64_t* d_xy, const uint8_t* d_inf, const uint32_t* offsets, size_t n_sets, const uint8_t* d_bits, size_t m, uint64_t* d_out, uint8_t* d_oinf,
                 uint32_t* d_count, hipStream_t s, EvLog* log, int* lanes_used) {
    CallScope cs(s);
    const uint32_t shared = n_sets == 1 ? 1u : 0u;        // (m == 1 with one set: the two forms coincide; it runs as the shared form)
    uint32_t *d_off, *d_info, *d_tmp, *d_total;
    uint8_t* d_side;
    HIP_TRY(cs.alloc(&d_off, (n_sets + 1) * 4), 10);
    HIP_TRY(cs.alloc(&d_info, 8), 10);
    HIP_TRY(cs.alloc(&d_side, m), 10);
    HIP_TRY(cs.alloc(&d_tmp, m * 4 * FW * 4), 10);
    HIP_TRY(cs.alloc(&d_total, 4 * FW * 4), 10);
    HIP_TRY(hipMemcpyAsync(d_off, offsets, (n_sets + 1) * 4, hipMemcpyHostToDevice, s), 10);
    HIP_TRY(hipMemsetAsync(d_info, 0, 8, s), 10);
    hipEvent_t e0 = log->open();
    hipLaunchKernelGGL(k_seal_count, dim3(((uint32_t)m + 255) / 256), dim3(256), 0, s, d_off, shared, d_bits, (uint32_t)m, g_agg_complement, d_count, d_side, d_info);
    log->close(7, e0);
    HIP_TRY(hipGetLastError(), 10);
    uint32_t info[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(info, d_info, 8, hipMemcpyDeviceToHost, s), 10);
    HIP_TRY(hipStreamSynchronize(s), 10);
    const uint32_t L = g_agg_lanes ? (uint32_t)g_agg_lanes : agg_pick_lanes(info[0], m);
    const size_t slot_bytes = (size_t)agg_slot_words<F>() * 4;
    e0 = log->open();
    if (info[1])
      hipLaunchKernelGGL((k_masked_sum<F>), dim3(1), dim3(AGG_BLOCK), AGG_BLOCK * slot_bytes, s, d_xy, d_inf, d_off, 1u, nullptr, nullptr, nullptr, 1u, AGG_MAX_LANES, d_total);
    hipLaunchKernelGGL((k_masked_sum<F>), dim3(((uint32_t)m + AGG_BLOCK / L - 1) / (AGG_BLOCK / L)), dim3(AGG_BLOCK), L > 1 ? AGG_BLOCK * slot_bytes : 0, s, d_xy, d_inf, d_off,
                       shared, d_bits, d_side, d_total, (uint32_t)m, L, d_tmp);
    normalize_xyzz<F, false>(d_tmp, d_out, d_oinf, (uint32_t)m, 0, s);
    log->close(0, e0);
    HIP_TRY(hipGetLastError(), 10);
    HIP_TRY(hipStreamSynchronize(s), 10);
    *lanes_used = (int)L;
    return 0;
  }
};

// what needs no device: 2 for a refused argument
static int agg_refuse(const void* xy, const uint32_t* offsets, size_t n_sets, const void* bits, size_t m, const void* out_xy, const void* out_inf) {
  if (!xy || !offsets || !bits || !out_xy || !out_inf || m > AGG_MAX_SEALS || (n_sets != 1 && n_sets != m)) return 2;
  for (size_t i = 0; i < n_sets; i++) if (offsets[i + 1] < offsets[i]) return 2;
  return 0;
}

// Host or device pointers (runtime.h, the call frame); offsets stays a host pointer in both forms.  The rows, bytes and flags carry 8
// bytes of slack on the device.
template <class F>
static int agg_call(const void* xy, const void* inf, const uint32_t* offsets, size_t n_sets, const void* bits, size_t m, void* out_xy, void* out_inf, void* out_count,
                    int dev, void* stream_) {
  constexpr size_t RW = 2 * Agg<F>::A;
  if (m == 0) return 0;
  if (int rc = agg_refuse(xy, offsets, n_sets, bits, m, out_xy, out_inf)) return rc;
  if (int rc0 = api_enter()) return rc0;
  std::lock_guard<std::mutex> lk(agg_mu);
  TimedCall call(g_agg_last, 6);
  CallScope cs;
  HIP_TRY(cs.open(dev, stream_), 10);
  EvLog log(cs.stream());
  const size_t rows = offsets[n_sets], n_bits = n_sets == 1 ? m * (size_t)(offsets[1] - offsets[0]) : rows;
  uint64_t *d_xy, *d_out;
  uint8_t *d_inf, *d_bits, *d_oinf;
  uint32_t* d_count;
  HIP_TRY(cs.in(&d_xy, xy, rows * RW * 8, dev, 8), 10);
  HIP_TRY(cs.in(&d_bits, bits, n_bits, dev, 8), 10);
  HIP_TRY(cs.in(&d_inf, inf, rows, dev, 8), 10);
  HIP_TRY(cs.out(&d_out, out_xy, m * RW * 8, dev), 10);
  HIP_TRY(cs.out(&d_oinf, out_inf, m, dev), 10);
  HIP_TRY(cs.out(&d_count, out_count, m * 4, dev), 10);
  if (!d_count) HIP_TRY(cs.alloc(&d_count, m * 4), 10);            // the counts are optional to the caller, not to the sums
  if (int rcr = Agg<F>::run(d_xy, d_inf, offsets, n_sets, d_bits, m, d_out, d_oinf, d_count, cs.stream(), &log, &call.t.tag[1])) return rcr;
  HIP_TRY(cs.copy_back(), 10);
  HIP_TRY(hipStreamSynchronize(cs.stream()), 10);
  log.sum(call.t.ms);
  call.t.ms[0] += call.t.ms[7];
  return 0;
}

// group 0 / 1: BLS12-377 G1 / G2
int aggregate_by_bitmap(int group, const void* xy, const void* inf, const uint32_t* offsets, size_t n_sets, const void* bits, size_t m, void* out_xy, void* out_inf,
                        void* out_count, int dev, void* stream) {
  switch (group) {
    case 0: return agg_call<Fp<P377>>(xy, inf, offsets, n_sets, bits, m, out_xy, out_inf, out_count, dev, stream);
    case 1: return agg_call<Fp2<P377>>(xy, inf, offsets, n_sets, bits, m, out_xy, out_inf, out_count, dev, stream);
    default: return 2;
  }
}
// ---- aggregated seals to verdicts.  Status per seal, the first that applies: 1 too few signers (or none), 2 the signature does not decode
// or lies outside G1, 3 the hash found no counter, 4 the product is not one (set on the host from the engine's verdicts).
struct SealNegG2 { uint64_t xy[24]; };       // -g2, affine, arkworks Montgomery limbs
// wire: the decoder's status (0 decoded, 1 the identity's encoding, 2 / 3 refused); siginf: the signature is the identity
__global__ void __launch_bounds__(256) k_seal_status(const uint32_t* __restrict__ count, const uint32_t* __restrict__ min_signers, const uint8_t* __restrict__ wire,
                                                     const uint8_t* __restrict__ attempts, uint32_t m, uint8_t* __restrict__ status, uint8_t* __restrict__ siginf) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  uint8_t st = 0;
  if (count[i] == 0 || (min_signers && count[i] < min_signers[i])) st = 1;
  else if (wire[i] >= 2) st = 2;
  else if (attempts[i] == 255) st = 3;
  status[i] = st;
  siginf[i] = wire[i] == 1 ? 1 : 0;
}
// r4: the 4 x u64 the block kernel wrote per seal; sc: the exponent r_i of groth16_verify.h in 4 u64, zero for a seal whose status is set
__global__ void __launch_bounds__(256) k_seal_exponents(const uint64_t* __restrict__ r4, const uint8_t* __restrict__ status, uint32_t m, uint64_t* __restrict__ sc) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  uint64_t lo, hi;
  g16_exponent(r4[(size_t)i * 4], r4[(size_t)i * 4 + 1], lo, hi);
  const uint64_t keep = status[i] ? 0 : ~0ull;
  uint64_t* o = sc + (size_t)i * 4;
  o[0] = lo & keep; o[1] = hi & keep; o[2] = 0; o[3] = 0;
}
// "each": product i = (sig_i, -g2), (H_i, apk_i); one lane per (seal, u64 of a G2 row).  A seal whose status is set has both G1 sides
// flagged: its pairs contribute 1 and none is evaluated.
__global__ void __launch_bounds__(256) k_pack_seal_pairs(const uint64_t* __restrict__ sig, const uint8_t* __restrict__ siginf, const uint64_t* __restrict__ hash,
                                                         const uint64_t* __restrict__ apk, const uint8_t* __restrict__ apkinf, const uint8_t* __restrict__ status,
                                                         SealNegG2 ng2, uint32_t m, uint64_t* __restrict__ g1, uint64_t* __restrict__ g2, uint8_t* __restrict__ i1,
                                                         uint8_t* __restrict__ i2) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t i = t / 24;
  const uint32_t w = (uint32_t)(t % 24);
  if (i >= m) return;
  if (w < 12) { g1[(2 * i) * 12 + w] = sig[i * 12 + w]; g1[(2 * i + 1) * 12 + w] = hash[i * 12 + w]; }
  g2[(2 * i) * 24 + w] = ng2.xy[w];
  g2[(2 * i + 1) * 24 + w] = apk[i * 24 + w];
  if (w == 0) {
    const uint8_t bad = status[i] ? 1 : 0;
    i1[2 * i] = siginf[i] | bad; i1[2 * i + 1] = bad;
    i2[2 * i] = 0; i2[2 * i + 1] = apkinf[i];
  }
}
// "combined": pairs 0 .. m - 1 = ([r_i] H_i, apk_i), and the G2 side of pair m, -g2 (its G1 row, sum r_i sig_i, comes from the host)
__global__ void __launch_bounds__(256) k_pack_seal_combined(const uint64_t* __restrict__ rh, const uint8_t* __restrict__ rhinf, const uint64_t* __restrict__ apk,
                                                            const uint8_t* __restrict__ apkinf, const uint8_t* __restrict__ status, SealNegG2 ng2, uint32_t m,
                                                            uint64_t* __restrict__ g1, uint64_t* __restrict__ g2, uint8_t* __restrict__ i1, uint8_t* __restrict__ i2) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t i = t / 24;
  const uint32_t w = (uint32_t)(t % 24);
  if (i > m) return;
  if (i < m) {
    if (w < 12) g1[i * 12 + w] = rh[i * 12 + w];
    g2[i * 24 + w] = apk[i * 24 + w];
    if (w == 0) { i1[i] = rhinf[i] | (status[i] ? 1 : 0); i2[i] = apkinf[i]; }
  } else {
    g2[i * 24 + w] = ng2.xy[w];
    if (w == 0) i2[i] = 0;
  }
}

struct SealDev { uint64_t *sig, *hash, *apk; uint8_t *siginf, *apkinf, *status; };

// m products of two pairs behind the producer stream of cs; is_one: m host bytes
static int seals_run_each(const SealDev& d, const SealNegG2& ng2, size_t m, CallScope& cs, uint8_t* is_one, float* ms_pair) {
  StagedProduct<Pairing377> g;
  if (int rc = g.stage((uint32_t)(2 * m), m)) return rc;
  if (int rc = g.after(cs)) return rc;
  hipLaunchKernelGGL(k_pack_seal_pairs, dim3((unsigned)((m * 24 + 255) / 256)), dim3(256), 0, g.ps.stream, d.sig, d.siginf, d.hash, d.apk, d.apkinf, d.status, ng2, (uint32_t)m,
                     g.ps.d_g1, g.ps.d_g2, g.ps.d_i1, g.ps.d_i2);
  HIP_TRY(hipGetLastError(), 10);
  std::vector<uint32_t> off(m + 1);
  for (size_t p = 0; p <= m; p++) off[p] = (uint32_t)(2 * p);
  return g.run(off.data(), m, is_one, ms_pair);
}

int verify_aggregated_seals_377(const uint64_t* pk_xy, const uint8_t* pk_inf, const uint32_t* offsets, size_t n_sets, const uint8_t* bits, const uint32_t* min_signers,
                                const uint8_t* domain, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* extras, const uint64_t* extra_off, int hash_mode,
                                const uint8_t* sig48, const uint64_t neg_g2_xy[24], size_t m, int mode, const uint32_t* key, uint8_t* out_ok, uint8_t* out_status) {
  if (m == 0) return 0;
  if (!domain || !msgs || !msg_off || !sig48 || !neg_g2_xy || !out_ok || (hash_mode != 0 && hash_mode != 2 && hash_mode != 3) || (mode != 0 && mode != 1)) return 2;
  if (int rc = agg_refuse(pk_xy, offsets, n_sets, bits, m, pk_xy, pk_xy)) return rc;
  if (int rc0 = api_enter()) return rc0;
  TimedCall call(g_agg_last, 6);
  float* const ms = call.t.ms;
  // the message hashes: the hash unit hands its rows back on the host, as in sign_batch
  std::vector<uint64_t> hxy(m * 12);
  std::vector<uint8_t> att(m);
  if (int rc = hash_to_g1_direct_run(domain, msgs, msg_off, extras, extra_off, m, hxy.data(), att.data(), hash_mode, 0, nullptr, &ms[2])) return rc;
  SealNegG2 ng2;
  for (int q = 0; q < 24; q++) ng2.xy[q] = neg_g2_xy[q];
  std::vector<uint8_t> h_status(m), is_one(m, 0);
  std::lock_guard<std::mutex> lk(agg_mu);
  int path = 0;
  const int rc = [&]() -> int {
    CallScope cs;
    HIP_TRY(cs.open(0, nullptr), 10);
    const hipStream_t s = cs.stream();
    EvLog log(s);
    const uint32_t m32 = (uint32_t)m;
    const size_t rows = offsets[n_sets], n_bits = n_sets == 1 ? m * (size_t)(offsets[1] - offsets[0]) : rows;
    uint64_t* d_xy;
    uint8_t *d_inf, *d_bits, *d_sig48, *d_wire, *d_att;
    uint32_t *d_count, *d_min;
    SealDev d;
    HIP_TRY(cs.alloc(&d_wire, m), 10);
    HIP_TRY(cs.alloc(&d_count, m * 4), 10);
    HIP_TRY(cs.alloc(&d.sig, m * 96), 10);
    HIP_TRY(cs.alloc(&d.apk, m * 192), 10);
    HIP_TRY(cs.alloc(&d.siginf, m), 10);
    HIP_TRY(cs.alloc(&d.apkinf, m), 10);
    HIP_TRY(cs.alloc(&d.status, m), 10);
    hipEvent_t e0 = log.open();
    HIP_TRY(cs.in(&d_xy, pk_xy, rows * 192, 0, 8), 10);
    HIP_TRY(cs.in(&d_bits, bits, n_bits, 0, 8), 10);
    HIP_TRY(cs.in(&d_sig48, sig48, m * 48, 0), 10);
    HIP_TRY(cs.in(&d.hash, hxy.data(), m * 96, 0), 10);
    HIP_TRY(cs.in(&d_att, att.data(), m, 0), 10);
    HIP_TRY(cs.in(&d_inf, pk_inf, rows, 0, 8), 10);
    HIP_TRY(cs.in(&d_min, min_signers, m * 4, 0), 10);
    log.close(5, e0);
    if (int rcr = Agg<Fp2<P377>>::run(d_xy, d_inf, offsets, n_sets, d_bits, m, d.apk, d.apkinf, d_count, s, &log, &call.t.tag[1])) return rcr;
    if (int rcw = wire_decompress(0, d_sig48, m, 1, d.sig, d_wire, 1, s, &ms[1])) return rcw;
    hipLaunchKernelGGL(k_seal_status, dim3((m32 + 255) / 256), dim3(256), 0, s, d_count, d_min, d_wire, d_att, m32, d.status, d.siginf);
    HIP_TRY(hipGetLastError(), 10);
    e0 = log.open();
    HIP_TRY(hipMemcpyAsync(h_status.data(), d.status, m, hipMemcpyDeviceToHost, s), 10);
    log.close(5, e0);
    HIP_TRY(hipStreamSynchronize(s), 10);
    size_t clean = 0;
    for (size_t i = 0; i < m; i++) clean += h_status[i] == 0;
    if (clean == 0) { path = mode; log.sum(ms); return 0; }            // no product to check: every verdict is its status
    if (mode == 1) {
      uint32_t k8[8];
      if (key) memcpy(k8, key, sizeof k8);
      else if (!os_random(k8, sizeof k8)) return 1;         // 32 bytes from the operating system per call, as the Groth16 verifier's exponent stream
      const WallMs wall_msm;
      uint64_t *d_r4, *d_sc, *d_rh;
      uint32_t* d_off;
      uint8_t* d_rhinf;
      const uint32_t off2[2] = {0, m32};
      HIP_TRY(cs.alloc(&d_r4, m * 32), 10);
      HIP_TRY(cs.alloc(&d_sc, m * 32), 10);
      HIP_TRY(cs.alloc(&d_rh, m * 96), 10);
      HIP_TRY(cs.alloc(&d_rhinf, m), 10);
      HIP_TRY(cs.alloc(&d_off, 8), 10);
      HIP_TRY(hipMemcpyAsync(d_off, off2, 8, hipMemcpyHostToDevice, s), 10);
      if (int rcd = bv_draw_exponents(k8, d_off, 1, m, d_r4, s)) return rcd;
      hipLaunchKernelGGL(k_seal_exponents, dim3((m32 + 255) / 256), dim3(256), 0, s, d_r4, d.status, m32, d_sc);
      HIP_TRY(hipGetLastError(), 10);
      // [r_i] H_i on the subgroup path (a hash is cofactor-cleared; a seal whose status is set has r_i = 0 and comes out as the identity),
      // then sum r_i sig_i: one m-term MSM over the decoded signatures (elements of G1: the decoder checked)
      if (int rcm = scalar_mul_batch(0, 1, d.hash, nullptr, d_sc, m, m, d_rh, d_rhinf, 1, s)) return rcm;
      uint64_t jac[18], tail[12];
      uint8_t tinf = 0;
      if (int rcm = MsmApi<G1_377>::dev(d.sig, d.siginf, d_sc, m, 1, jac, s)) return rcm;
      HIP_TRY(hipStreamSynchronize(s), 10);
      if (int rcn = wire_normalize(0, jac, 1, tail, &tinf)) return rcn;
      ms[3] = wall_msm.ms();
      uint8_t v = 0;
      {
        StagedProduct<Pairing377> g;
        if (int rcs = g.stage(m32 + 1, 1)) return rcs;
        hipLaunchKernelGGL(k_pack_seal_combined, dim3((unsigned)(((m + 1) * 24 + 255) / 256)), dim3(256), 0, g.ps.stream, d_rh, d_rhinf, d.apk, d.apkinf, d.status, ng2, m32,
                           g.ps.d_g1, g.ps.d_g2, g.ps.d_i1, g.ps.d_i2);
        HIP_TRY(hipGetLastError(), 10);
        HIP_TRY(hipMemcpyAsync(g.ps.d_g1 + m * 12, tail, sizeof tail, hipMemcpyHostToDevice, g.ps.stream), 10);
        HIP_TRY(hipMemcpyAsync(g.ps.d_i1 + m, &tinf, 1, hipMemcpyHostToDevice, g.ps.stream), 10);
        const uint32_t off[2] = {0, m32 + 1};
        if (int rcp = g.run(off, 1, &v, &ms[4])) return rcp;
      }
      if (v) {
        for (size_t i = 0; i < m; i++) is_one[i] = 1;
        path = 1;
        log.sum(ms);
        return 0;
      }
      path = 2;
    }
    if (int rce = seals_run_each(d, ng2, m, cs, is_one.data(), &ms[4])) return rce;
    log.sum(ms);
    return 0;
  }();
  ms[0] += ms[7];
  call.t.tag[0] = path;
  if (rc) return rc;
  for (size_t i = 0; i < m; i++) {
    const uint8_t st = h_status[i] ? h_status[i] : is_one[i] ? 0 : 4;
    out_ok[i] = st == 0 ? 1 : 0;
    if (out_status) out_status[i] = st;
  }
  return 0;
}

int aggregate_set_lanes(int lanes) {
  if (lanes != 0 && !agg_lanes_ok(lanes)) return 2;
  std::lock_guard<std::mutex> lk(agg_mu);
  g_agg_lanes = lanes;
  return 0;
}
int aggregate_set_complement(int mode) {
  if (mode < -1 || mode > 1) return 2;
  std::lock_guard<std::mutex> lk(agg_mu);
  g_agg_complement = mode;
  return 0;
}
void seals_last(int* path, int* lanes, float ms[8]) {
  const CallTimes t = g_agg_last.read();
  *path = t.tag[0];
  *lanes = t.tag[1];
  for (int i = 0; i < 8; i++) ms[i] = t.ms[i];
}

}  // namespace celo
