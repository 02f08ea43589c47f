// Groth16 verification for m proofs under one verifying key (ark_groth16::prepare_verifying_key + verify_proof), from the inputs to the
// verdict bytes on the device: the kernels and the host code, one template over the curve description C of groth16_verify.h.
// unit_groth16_verify.hip instantiates it for BW6-761 (crates/epoch-snark/src/api/verifier.rs:35) and holds what the curves share (the
// handle registry, the last call's record, the exponent draw); unit_groth16_verify377.hip instantiates it for BLS12-377 (the hash-helper
// proof of crates/epoch-snark/src/api/prover.rs:83-118).  DESIGN.md section 6h.
//
//   key load     -alpha, beta, -gamma, -delta and one signed-digit window table per input base (unit_setup.hip's k_fbm_bases / k_fbm_table)
//   k_g16_inputs one lane per proof: the range test of its inputs and acc = abc_0 + sum_j x_j abc_j from the tables; k_normalize
//   k_g16_inputs_lanes   BLS12-377 keys of more than 64 inputs (the wide loaders): L lanes per proof, each summing the inputs j = l mod L, folded
//                through LDS; L by g16_pick_lanes or celo_amd_groth16_set_input_lanes
//   each         k_g16_pack_each writes (A, B), (acc, -gamma), (C, -delta), (-alpha, beta) per proof into the pairing engine's input
//                slots: m products of four pairs, m verdicts
//   combined     exponents r_i from ChaCha20 (unit_batchverify.hip's block kernel), k_g16_scale: r_i A_i by a 128-bit ladder, two
//                m-term MSMs for sum r_i acc_i and sum r_i C_i, (sum r_i) alpha on the host; one product of m + 3 pairs.  A rejected
//                combination falls back to `each`.
// The serialized entry decodes A | B | C with the curve's checked decoders (unit_wire761.hip, unit_wire.hip) into the rows the kernels read.
#pragma once
#include "groth16_verify.h"
#include "normalize.h"
#include <hip/hip_runtime.h>
#include <cstring>
#include <memory>
#include <vector>
#include "runtime.h"
#include "units.h"

namespace celo {

static_assert(VK_MAX_INPUTS == G16_MAX_INPUTS && VK_MAX_INPUTS_WIDE == G16_MAX_INPUTS_WIDE, "units.h and groth16_verify.h name one pair of limits");

struct VerifyingKey {
  int curve = 0;                     // C::ID: an entry of the other curve refuses the handle
  int device = 0;
  uint32_t n_in = 0;                 // public inputs: n_abc - 1
  int c = 0, W = 0;                  // window bits and windows of the input tables
  uint64_t* d_key = nullptr;         // 4 x G16_KW u64: -alpha, beta, -gamma, -delta (affine arkworks limbs)
  uint32_t kinf = 0;                 // bit q: row q of d_key is the identity
  uint32_t* d_abc0 = nullptr;        // gamma_abc[0] as a table entry
  bool abc0_inf = false;
  uint32_t* d_table = nullptr;       // n_in tables of W 2^(c-1) entries, base-major
  uint8_t* d_tinf = nullptr;
  uint64_t neg_alpha[G16_KW] = {};   // the host's copy for (sum r_i) alpha
  ~VerifyingKey() {
    for (void* p : {(void*)d_key, (void*)d_abc0, (void*)d_table, (void*)d_tinf}) if (p) (void)hipFree(p);
  }
};

// ---- the device side of a curve: its MSM group, pairing engine, decoder and table builder, and the occupancy of its lane kernels - one wave
// per SIMD for the 28-limb field, as the other 28-limb lane kernels (unit_wire761.hip: the XYZZ accumulator, the point and the addition's
// temporaries); two for the 14-limb field, as unit_wire.hip's
template <class C> struct G16Dev;
template <> struct G16Dev<G16Bw6> : Pairing761 {
  typedef G_761 Group;
  static constexpr int WAVES = 1;
  static int decode(int g2, const uint8_t* in, size_t n, uint64_t* out, uint8_t* status, void* stream) { return wire761_decode(g2, 1, in, n, 1, out, status, 1, stream); }
};
template <> struct G16Dev<G16Bls> : Pairing377 {
  typedef G1_377 Group;
  static constexpr int WAVES = 2;
  static int decode(int g2, const uint8_t* in, size_t n, uint64_t* out, uint8_t* status, void* stream) { return wire_decompress(g2, in, n, 1, out, status, 1, stream); }
};

// ---- kernels
template <class C>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(G16Dev<C>::WAVES, G16Dev<C>::WAVES)))
k_g16_inputs(const uint64_t* __restrict__ inputs, uint32_t m, uint32_t n_in, const uint32_t* __restrict__ abc0, int abc0_inf, const uint32_t* __restrict__ table,
             const uint8_t* __restrict__ tinf, int c, int W, uint32_t* __restrict__ xyzz, uint8_t* __restrict__ status) {
  typedef typename C::F F;
  constexpr int FW = F::WORDS;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  uint32_t bad = 0;
  const Xyzz<F> a = g16_input_row<C>(inputs + (size_t)i * n_in * C::N64, n_in, abc0, abc0_inf != 0, table, tinf, c, W, &bad);
  uint32_t* o = xyzz + (size_t)i * 4 * FW;
  a.X.store(o); a.Y.store(o + FW); a.ZZ.store(o + 2 * FW); a.ZZZ.store(o + 3 * FW);
  if (bad) status[i] = 1;
}
// L lanes per proof (groth16_verify.h: g16_lane_sum and the fold), L a power of two from 2 to 256, in workgroups of max(64, L) lanes: 64 / L
// proofs per workgroup below 64, one from there.  Dynamic LDS: blockDim.x / 2 slots of agg_slot_words<F>() words - the L / 2 slots of each
// of the workgroup's proofs one after the other (34 KiB at 256 lanes of the 14-limb field).  Every lane of the workgroup walks the rounds:
// the barriers are outside the lane tests.  The output is k_g16_inputs's.
template <class C>
__global__ void __launch_bounds__(G16_MAX_LANES) __attribute__((amdgpu_waves_per_eu(G16Dev<C>::WAVES, G16Dev<C>::WAVES)))
k_g16_inputs_lanes(const uint64_t* __restrict__ inputs, uint32_t m, uint32_t n_in, const uint32_t* __restrict__ abc0, int abc0_inf, const uint32_t* __restrict__ table,
                   const uint8_t* __restrict__ tinf, int c, int W, uint32_t L, uint32_t* __restrict__ xyzz, uint8_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) uint32_t g16_lds[];
  typedef typename C::F F;
  constexpr int FW = F::WORDS;
  const uint32_t lane = threadIdx.x & (L - 1), q = threadIdx.x / L, i = blockIdx.x * (blockDim.x / L) + q;
  const bool live = i < m;
  uint32_t bad = 0;
  Xyzz<F> acc = Xyzz<F>::identity();
  if (live) acc = g16_lane_sum<C>(inputs + (size_t)i * n_in * C::N64, n_in, lane, L, abc0, abc0_inf != 0, table, tinf, c, W, &bad);
  uint32_t* slots = g16_lds + (size_t)q * (L >> 1) * agg_slot_words<F>();
  for (uint32_t s = L >> 1; s; s >>= 1) {
    __syncthreads();                            // the reads of the round before, from the slots this round writes
    if (lane >= s && lane < 2 * s) g16_fold_put<F>(slots, acc, lane, s);
    __syncthreads();
    if (lane < s) g16_fold_take<F>(acc, slots, lane);
  }
  if (!live) return;
  if (bad) status[i] = 1;                       // (several lanes may write the same byte)
  if (lane == 0) {
    uint32_t* o = xyzz + (size_t)i * 4 * FW;
    acc.X.store(o); acc.Y.store(o + FW); acc.ZZ.store(o + 2 * FW); acc.ZZZ.store(o + 3 * FW);
  }
}
// r4: the 4 x u64 the block kernel wrote per proof; sc: N64 x u64 scalars for the MSMs (zero for a proof whose status is set)
template <int N64>
__global__ void __launch_bounds__(256) k_g16_exponents(const uint64_t* __restrict__ r4, const uint8_t* __restrict__ status, uint32_t m, uint64_t* __restrict__ sc) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  uint64_t lo, hi;
  g16_exponent(r4[(size_t)i * 4], r4[(size_t)i * 4 + 1], lo, hi);
  const uint64_t keep = status && status[i] ? 0 : ~0ull;
  uint64_t* o = sc + (size_t)i * N64;
  o[0] = lo & keep; o[1] = hi & keep;
#pragma unroll
  for (int k = 2; k < N64; k++) o[k] = 0;
}
template <class C>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(G16Dev<C>::WAVES, G16Dev<C>::WAVES)))
k_g16_scale(const uint64_t* __restrict__ a_xy, const uint8_t* __restrict__ a_inf, const uint8_t* __restrict__ status, const uint64_t* __restrict__ sc, uint32_t m,
            uint32_t* __restrict__ xyzz) {
  typedef typename C::F F;
  constexpr int FW = F::WORDS;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  uint32_t* o = xyzz + (size_t)i * 4 * FW;
  if (a_inf[i] || status[i]) {
    for (int q = 0; q < 4 * FW; q++) o[q] = 0;
    return;
  }
  const uint64_t* src = a_xy + (size_t)i * C::G1W;
  const Affine<F> p = {F::norm(F::from_ark(src)), F::norm(F::from_ark(src + F::ARK64))};
  const Xyzz<F> a = g16_scale128(p, sc[(size_t)i * C::N64], sc[(size_t)i * C::N64 + 1]);
  a.X.store(o); a.Y.store(o + FW); a.ZZ.store(o + 2 * FW); a.ZZZ.store(o + 3 * FW);
}
// one lane per (proof, u64 of the wider row).  key: the four rows of VerifyingKey::d_key; W1 / W2: u64 of a G1 / G2 row
template <class C>
__global__ void __launch_bounds__(256)
k_g16_pack_each(const uint64_t* __restrict__ a, const uint8_t* __restrict__ ainf, const uint64_t* __restrict__ b, const uint8_t* __restrict__ binf,
                const uint64_t* __restrict__ c, const uint8_t* __restrict__ cinf, const uint64_t* __restrict__ acc, const uint8_t* __restrict__ accinf,
                const uint8_t* __restrict__ status, const uint64_t* __restrict__ key, uint32_t kinf, uint32_t m, uint64_t* __restrict__ g1, uint64_t* __restrict__ g2,
                uint8_t* __restrict__ i1, uint8_t* __restrict__ i2) {
  constexpr int W1 = C::G1W, W2 = C::G2W, WL = W1 > W2 ? W1 : W2, KW = G16_KW;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t i = t / WL;
  const uint32_t w = (uint32_t)(t % WL);
  if (i >= m) return;
  if (w < W1) {
    uint64_t* o1 = g1 + i * 4 * W1 + w;
    o1[0] = a[i * W1 + w]; o1[W1] = acc[i * W1 + w]; o1[2 * W1] = c[i * W1 + w]; o1[3 * W1] = key[w];
  }
  if (w < W2) {
    uint64_t* o2 = g2 + i * 4 * W2 + w;
    o2[0] = b[i * W2 + w]; o2[W2] = key[2 * KW + w];     o2[2 * W2] = key[3 * KW + w];   o2[3 * W2] = key[KW + w];
  }
  if (w == 0) {
    const uint8_t bad = status[i] ? 1 : 0;            // (its verdict is 0 whatever the product: no pair of it is evaluated)
    i1[4 * i] = ainf[i] | bad; i1[4 * i + 1] = accinf[i] | bad; i1[4 * i + 2] = cinf[i] | bad; i1[4 * i + 3] = (uint8_t)(kinf & 1u) | bad;
    i2[4 * i] = binf[i]; i2[4 * i + 1] = (kinf >> 2) & 1u; i2[4 * i + 2] = (kinf >> 3) & 1u; i2[4 * i + 3] = (kinf >> 1) & 1u;
  }
}
// pairs 0 .. m - 1: (r_i A_i, B_i); the G2 side of pairs m, m + 1, m + 2: -gamma, -delta, beta (their G1 rows come from the host)
template <class C>
__global__ void __launch_bounds__(256)
k_g16_pack_combined(const uint64_t* __restrict__ ra, const uint8_t* __restrict__ rainf, const uint64_t* __restrict__ b, const uint8_t* __restrict__ binf,
                    const uint8_t* __restrict__ status, const uint64_t* __restrict__ key, uint32_t kinf, uint32_t m, uint64_t* __restrict__ g1,
                    uint64_t* __restrict__ g2, uint8_t* __restrict__ i1, uint8_t* __restrict__ i2) {
  constexpr int W1 = C::G1W, W2 = C::G2W, WL = W1 > W2 ? W1 : W2, KW = G16_KW;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t i = t / WL;
  const uint32_t w = (uint32_t)(t % WL);
  if (i >= (size_t)m + 3) return;
  if (i < m) {
    if (w < W1) g1[i * W1 + w] = ra[i * W1 + w];
    if (w < W2) g2[i * W2 + w] = b[i * W2 + w];
    if (w == 0) { i1[i] = rainf[i] | (status[i] ? 1 : 0); i2[i] = binf[i]; }
  } else {
    const uint32_t q = i == m ? 2u : i == (size_t)m + 1 ? 3u : 1u;
    if (w < W2) g2[i * W2 + w] = key[q * KW + w];
    if (w == 0) i2[i] = (kinf >> q) & 1u;
  }
}
// m serialized proofs (A | B | C, compressed) -> the G1 encodings (A of every proof, then C of every proof) and the G2 encodings; one lane
// per (proof, u64)
template <class C>
__global__ void __launch_bounds__(256) k_g16_split(const uint64_t* __restrict__ proofs, uint32_t m, uint64_t* __restrict__ g1b, uint64_t* __restrict__ g2b) {
  constexpr int S1 = C::G1_BYTES / 8, S2 = C::G2_BYTES / 8, SP = 2 * S1 + S2;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t i = t / SP;
  const uint32_t q = (uint32_t)(t % SP);
  if (i >= m) return;
  const uint64_t v = proofs[i * SP + q];
  if (q < S1) g1b[i * S1 + q] = v;
  else if (q < S1 + S2) g2b[i * S2 + (q - S1)] = v;
  else g1b[((size_t)m + i) * S1 + (q - S1 - S2)] = v;
}
// decoder statuses (wire.h: 0 ok, 1 infinity, 2 invalid, 3 outside the subgroup) -> identity flags and the proof's status
template <class C>
__global__ void __launch_bounds__(256) k_g16_fold(const uint8_t* __restrict__ st_ac, const uint8_t* __restrict__ st_b, uint32_t m, uint8_t* __restrict__ ainf,
                                                  uint8_t* __restrict__ binf, uint8_t* __restrict__ cinf, uint8_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint8_t sa = st_ac[i], sc = st_ac[(size_t)m + i], sb = st_b[i];
  ainf[i] = sa == WIRE_INFINITY; binf[i] = sb == WIRE_INFINITY; cinf[i] = sc == WIRE_INFINITY;
  status[i] = (sa >= WIRE_INVALID || sb >= WIRE_INVALID || sc >= WIRE_INVALID) ? 1 : 0;
}

// a status per proof that the caller brings (the epoch unit's: a block that does not decode) joins the decoder's
template <class C> __global__ void __launch_bounds__(256) k_g16_merge_status(const uint8_t* __restrict__ pre, uint32_t m, uint8_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m && pre[i]) status[i] = 1;
}

template <class C> struct G16Impl {
  typedef typename C::F F;
  typedef typename C::F2 F2;
  typedef G16Dev<C> D;
  static constexpr int FW = F::WORDS, A = F::ARK64, W1 = C::G1W, W2 = C::G2W, KW = G16_KW, N64 = C::N64;
  static constexpr int WL = W1 > W2 ? W1 : W2;
  static constexpr size_t PROOF_BYTES = 2 * C::G1_BYTES + C::G2_BYTES;

  // ---- key load
  static int vk_build(const uint64_t* rows /* alpha, beta, gamma, delta, abc[n_abc]: KW u64 each */, const uint8_t* inf /* or NULL */, size_t n_abc, VerifyingKey** out) {
    if (int rc0 = api_enter()) return rc0;
    std::unique_ptr<VerifyingKey> vk(new VerifyingKey);
    vk->curve = C::ID;
    vk->device = api_device();
    vk->n_in = (uint32_t)(n_abc - 1);
    vk->c = g16_window_bits<C>(vk->n_in);
    vk->W = fb_windows(C::SCALAR_BITS, vk->c);
    uint64_t key[4 * KW];
    memcpy(key, rows, sizeof key);
    std::vector<uint8_t> rinf(4 + n_abc);
    for (size_t i = 0; i < 4 + n_abc; i++) {
      const bool g2 = i >= 1 && i <= 3;
      rinf[i] = (inf && inf[i]) || (g2 ? g16_row_is_identity<F2>(rows + i * KW) : g16_row_is_identity<F>(rows + i * KW));
    }
    for (int q = 0; q < 4; q++) {
      if (rinf[q]) { memset(key + q * KW, 0, KW * 8); vk->kinf |= 1u << q; }
      else if (q == 0) g16_negate_row<F>(key);                                 // -alpha, beta, -gamma, -delta
      else if (q != 1) g16_negate_row<F2>(key + q * KW);
    }
    memcpy(vk->neg_alpha, key, sizeof vk->neg_alpha);
    uint32_t abc0[2 * FW] = {};
    vk->abc0_inf = rinf[4] != 0;
    if (!vk->abc0_inf) fb_store_entry(abc0, Affine<F>{F::norm(F::from_ark(rows + 4 * KW)), F::norm(F::from_ark(rows + 4 * KW + A))});
    const size_t E = (size_t)vk->W << (vk->c - 1);
    HIP_TRY(hipMalloc(&vk->d_key, sizeof key), 10);
    HIP_TRY(hipMalloc(&vk->d_abc0, sizeof abc0), 10);
    HIP_TRY(hipMalloc(&vk->d_table, (vk->n_in ? vk->n_in : 1) * E * 2 * FW * 4), 10);
    HIP_TRY(hipMalloc(&vk->d_tinf, (vk->n_in ? vk->n_in : 1) * E), 10);
    {
      CallScope cs;
      HIP_TRY(cs.open(0, nullptr), 10);
      HIP_TRY(hipMemcpyAsync(vk->d_key, key, sizeof key, hipMemcpyHostToDevice, cs.stream()), 10);
      HIP_TRY(hipMemcpyAsync(vk->d_abc0, abc0, sizeof abc0, hipMemcpyHostToDevice, cs.stream()), 10);
      std::vector<uint64_t> bases((size_t)vk->n_in * W1);                      // the input bases as rows of their own width
      for (size_t j = 0; j < vk->n_in; j++) memcpy(bases.data() + j * W1, rows + (5 + j) * KW, W1 * 8);
      if (int rc = fixed_base_tables<F>(bases.data(), rinf.data() + 5, vk->n_in, C::SCALAR_BITS, vk->c, vk->d_table, vk->d_tinf, cs.stream())) return rc;
      HIP_TRY(hipStreamSynchronize(cs.stream()), 10);
    }
    groth16_vk_adopt(vk.get());
    *out = vk.release();
    return 0;
  }

  // ---- host pieces of the combined check
  static void jac_to_row(const uint64_t* jac, uint64_t* row, uint8_t* inf) {
    const F Z = F::norm(F::from_ark(jac + 2 * A));
    *inf = Z.is_zero_mod_p() ? 1 : 0;
    for (int q = 0; q < W1; q++) row[q] = 0;
    if (*inf) return;
    const F zi = F::norm(F::inv(Z)), zi2 = F::norm(F::sqr(zi));
    F::mul(F::from_ark(jac), zi2).to_ark(row);
    F::mul(F::from_ark(jac + A), F::norm(F::mul(zi2, zi))).to_ark(row + A);
  }
  // k P for k of three little-endian u64 (a sum of at most 2^24 exponents of 128 bits), P affine arkworks limbs: MSB-first over XYZZ
  static void mul_row(const uint64_t* xy, const uint64_t k[3], uint64_t* row, uint8_t* inf) {
    const Affine<F> p = {F::norm(F::from_ark(xy)), F::norm(F::from_ark(xy + A))};
    Xyzz<F> acc = Xyzz<F>::identity();
    for (int i = 191; i >= 0; i--) {
      acc = xyzz_dbl(acc);
      if ((k[i >> 6] >> (i & 63)) & 1) xyzz_madd(acc, p);
    }
    Affine<F> r = {F::zero(), F::zero()};
    for (int q = 0; q < W1; q++) row[q] = 0;
    *inf = fb_to_affine(acc, r) ? 0 : 1;
    if (!*inf) { r.x.to_ark(row); r.y.to_ark(row + A); }
  }

  struct DevProofs { uint64_t *a, *b, *c, *inputs, *acc; uint8_t *ainf, *binf, *cinf, *accinf, *status; };

  // m products of four pairs; is_one: m host bytes.  The producer stream s is chained in front of the engine's by an event.
  static int run_each(const VerifyingKey* vk, const DevProofs& d, size_t m, CallScope& cs, uint8_t* is_one, float* ms_pair) {
    StagedProduct<D> g;
    if (int rc = g.stage((uint32_t)(4 * m), m)) return rc;
    if (int rc = g.after(cs)) return rc;
    hipLaunchKernelGGL((k_g16_pack_each<C>), dim3((unsigned)((m * WL + 255) / 256)), dim3(256), 0, g.ps.stream, d.a, d.ainf, d.b, d.binf, d.c, d.cinf, d.acc, d.accinf,
                       d.status, vk->d_key, vk->kinf, (uint32_t)m, g.ps.d_g1, g.ps.d_g2, g.ps.d_i1, g.ps.d_i2);
    HIP_TRY(hipGetLastError(), 10);
    std::vector<uint32_t> off(m + 1);
    for (size_t p = 0; p <= m; p++) off[p] = (uint32_t)(4 * p);
    return g.run(off.data(), m, is_one, ms_pair);
  }

  // Everything after the proofs' rows, identity flags, statuses and inputs are on the device (stream cs.stream()).
  static int verify_core(const VerifyingKey* vk, DevProofs& d, size_t m, int mode, const uint32_t* key, uint8_t* out_ok, CallScope& cs, EvLog& log, float* ms, int* path,
                         int* lanes, uint8_t* out_refused = nullptr /* m host bytes: the statuses the verdicts were masked with */) {
    const hipStream_t s = cs.stream();
    const uint32_t m32 = (uint32_t)m, wblocks = (m32 + 63) / 64;
    uint32_t* d_xyzz;
    std::vector<uint8_t> h_status(m), is_one(m);
    HIP_TRY(cs.alloc(&d_xyzz, m * 4 * FW * 4), 10);
    HIP_TRY(cs.alloc(&d.acc, m * W1 * 8), 10);
    HIP_TRY(cs.alloc(&d.accinf, m), 10);
    // the lanes per input sum: one (k_g16_inputs) on BW6-761 and for every narrow key under the rule; BLS12-377: the rule or the forced width
    uint32_t L = 1;
    if constexpr (C::ID == 1) { const int forced = groth16_input_lanes(); L = forced ? (uint32_t)forced : g16_pick_lanes(vk->n_in, m); }
    hipEvent_t e0 = log.open();
    if (L == 1) {
      hipLaunchKernelGGL((k_g16_inputs<C>), dim3(wblocks), dim3(64), 0, s, d.inputs, m32, vk->n_in, vk->d_abc0, vk->abc0_inf ? 1 : 0, vk->d_table, vk->d_tinf, vk->c, vk->W,
                         d_xyzz, d.status);
    } else if constexpr (C::ID == 1) {
      const uint32_t block = L < 64 ? 64 : L, per = block / L;
      hipLaunchKernelGGL((k_g16_inputs_lanes<C>), dim3((m32 + per - 1) / per), dim3(block), (size_t)(block / 2) * agg_slot_words<F>() * 4, s, d.inputs, m32, vk->n_in,
                         vk->d_abc0, vk->abc0_inf ? 1 : 0, vk->d_table, vk->d_tinf, vk->c, vk->W, L, d_xyzz, d.status);
    }
    *lanes = (int)L;
    normalize_xyzz<F, true>(d_xyzz, d.acc, d.accinf, m32, 0, s);
    log.close(1, e0);
    HIP_TRY(hipGetLastError(), 10);
    HIP_TRY(hipMemcpyAsync(h_status.data(), d.status, m, hipMemcpyDeviceToHost, s), 10);
    *path = 0;
    if (mode == 1) {
      uint32_t k8[8];
      if (key) memcpy(k8, key, sizeof k8);
      else if (!os_random(k8, sizeof k8)) return 1;         // 32 bytes from the operating system per call, as batch_verify_strict's exponent stream
      uint64_t *d_r4, *d_sc, *d_ra;
      uint32_t* d_off;
      uint8_t* d_rainf;
      const uint32_t off2[2] = {0, m32};
      std::vector<uint64_t> h_r4(m * 4);
      HIP_TRY(cs.alloc(&d_r4, m * 32), 10);
      HIP_TRY(cs.alloc(&d_sc, m * N64 * 8), 10);
      HIP_TRY(cs.alloc(&d_ra, m * W1 * 8), 10);
      HIP_TRY(cs.alloc(&d_rainf, m), 10);
      HIP_TRY(cs.alloc(&d_off, 8), 10);
      HIP_TRY(hipMemcpyAsync(d_off, off2, 8, hipMemcpyHostToDevice, s), 10);
      e0 = log.open();
      // block i of the stream, its first 16 bytes: one "batch" of m signers makes the block kernel keep (128 + log2 m + 7) / 8 >= 16 bytes
      if (int rc = bv_draw_exponents(k8, d_off, 1, m, d_r4, s)) return rc;
      hipLaunchKernelGGL((k_g16_exponents<N64>), dim3((m32 + 255) / 256), dim3(256), 0, s, d_r4, d.status, m32, d_sc);
      hipLaunchKernelGGL((k_g16_scale<C>), dim3(wblocks), dim3(64), 0, s, d.a, d.ainf, d.status, d_sc, m32, d_xyzz);
      normalize_xyzz<F, true>(d_xyzz, d_ra, d_rainf, m32, 0, s);
      log.close(2, e0);
      HIP_TRY(hipGetLastError(), 10);
      HIP_TRY(hipMemcpyAsync(h_r4.data(), d_r4, m * 32, hipMemcpyDeviceToHost, s), 10);
      // sum r_i acc_i, sum r_i C_i: the variable-base MSM over the rows where they lie, the same scalars (zero for a proof whose status is set)
      const WallMs wall_msm;
      uint64_t jac[2][3 * 12], tail[3 * W1];
      uint8_t tinf[3];
      if (int rc = MsmApi<typename D::Group>::dev(d.acc, d.accinf, d_sc, m, 0, jac[0], s)) return rc;
      if (int rc = MsmApi<typename D::Group>::dev(d.c, d.cinf, d_sc, m, 0, jac[1], s)) return rc;
      HIP_TRY(hipStreamSynchronize(s), 10);                 // (the MSM calls return their sums to the host: s has drained already)
      jac_to_row(jac[0], tail, &tinf[0]);
      jac_to_row(jac[1], tail + W1, &tinf[1]);
      uint64_t sum[3] = {0, 0, 0};
      for (size_t i = 0; i < m; i++) {
        if (h_status[i]) continue;
        uint64_t lo, hi;
        g16_exponent(h_r4[i * 4], h_r4[i * 4 + 1], lo, hi);
        const unsigned __int128 t = (unsigned __int128)sum[0] + lo;
        const unsigned __int128 u = (unsigned __int128)sum[1] + hi + (uint64_t)(t >> 64);
        sum[0] = (uint64_t)t; sum[1] = (uint64_t)u; sum[2] += (uint64_t)(u >> 64);
      }
      if (vk->kinf & 1u) { memset(tail + 2 * W1, 0, W1 * 8); tinf[2] = 1; }
      else mul_row(vk->neg_alpha, sum, tail + 2 * W1, &tinf[2]);
      ms[3] = wall_msm.ms();
      int one = 0;
      {
        StagedProduct<D> g;
        if (int rc = g.stage(m32 + 3, 1)) return rc;
        hipLaunchKernelGGL((k_g16_pack_combined<C>), dim3((unsigned)(((m + 3) * WL + 255) / 256)), dim3(256), 0, g.ps.stream, d_ra, d_rainf, d.b, d.binf, d.status,
                           vk->d_key, vk->kinf, m32, g.ps.d_g1, g.ps.d_g2, g.ps.d_i1, g.ps.d_i2);
        HIP_TRY(hipGetLastError(), 10);
        HIP_TRY(hipMemcpyAsync(g.ps.d_g1 + m * W1, tail, sizeof tail, hipMemcpyHostToDevice, g.ps.stream), 10);
        HIP_TRY(hipMemcpyAsync(g.ps.d_i1 + m, tinf, 3, hipMemcpyHostToDevice, g.ps.stream), 10);
        const uint32_t off[2] = {0, m32 + 3};
        uint8_t v = 0;
        if (int rc = g.run(off, 1, &v, &ms[4])) return rc;
        one = v;
      }
      if (one) {
        for (size_t i = 0; i < m; i++) out_ok[i] = h_status[i] ? 0 : 1;
        if (out_refused) memcpy(out_refused, h_status.data(), m);
        *path = 1;
        return 0;
      }
      *path = 2;
    }
    if (int rc = run_each(vk, d, m, cs, is_one.data(), &ms[4])) return rc;
    for (size_t i = 0; i < m; i++) out_ok[i] = (is_one[i] && !h_status[i]) ? 1 : 0;
    if (out_refused) memcpy(out_refused, h_status.data(), m);
    return 0;
  }
};

template <class C>
int G16Api<C>::vk_load(const uint64_t* alpha_g1, const uint64_t* beta_g2, const uint64_t* gamma_g2, const uint64_t* delta_g2, const uint64_t* gamma_abc_g1, size_t n_abc,
                       VerifyingKey** out, size_t max_inputs) {
  constexpr int W1 = C::G1W, W2 = C::G2W, KW = G16_KW;
  if (!out) return 2;
  *out = nullptr;
  if (!alpha_g1 || !beta_g2 || !gamma_g2 || !delta_g2 || !gamma_abc_g1 || n_abc == 0) return 2;
  if (n_abc - 1 > max_inputs) return G16_ERR_INPUTS;
  std::vector<uint64_t> rows((4 + n_abc) * KW, 0);
  memcpy(rows.data(), alpha_g1, W1 * 8); memcpy(rows.data() + KW, beta_g2, W2 * 8); memcpy(rows.data() + 2 * KW, gamma_g2, W2 * 8);
  memcpy(rows.data() + 3 * KW, delta_g2, W2 * 8);
  for (size_t j = 0; j < n_abc; j++) memcpy(rows.data() + (4 + j) * KW, gamma_abc_g1 + j * W1, W1 * 8);
  return G16Impl<C>::vk_build(rows.data(), nullptr, n_abc, out);
}
template <class C> int G16Api<C>::vk_load_serialized(const uint8_t* bytes, size_t len, VerifyingKey** out, size_t max_inputs) {
  if (!out) return 2;
  *out = nullptr;
  std::vector<uint64_t> rows;
  std::vector<uint8_t> inf;
  if (int rc = g16_vk_parse<C>(bytes, len, rows, inf, nullptr, max_inputs)) return rc;
  return G16Impl<C>::vk_build(rows.data(), inf.data(), inf.size() - 4, out);
}

// proofs != NULL: the serialized entry (m x PROOF_BYTES, a_xy .. c_inf unused); else the limb entry.  d_inputs != NULL (verify_staged): the
// inputs are on the device already, complete in stream order for a new stream (the caller has synchronised); d_pre: m device bytes, a proof
// whose byte is set is treated as one that did not decode; out_refused: m host bytes, the statuses the verdicts were masked with
template <class C>
static int g16_verify_call(const VerifyingKey* vk, const uint64_t* a_xy, const uint8_t* a_inf, const uint64_t* b_xy, const uint8_t* b_inf, const uint64_t* c_xy,
                           const uint8_t* c_inf, const uint8_t* proofs, const uint64_t* inputs, const uint64_t* d_inputs, const uint8_t* d_pre, size_t m, int mode,
                           const uint32_t* key, uint8_t* out_ok, uint8_t* out_refused) {
  typedef G16Impl<C> I;
  typedef G16Dev<C> D;
  constexpr int W1 = C::G1W, W2 = C::G2W, S1 = C::G1_BYTES, S2 = C::G2_BYTES;
  constexpr size_t PB = I::PROOF_BYTES;
  if (m == 0) return 0;
  if (!vk || !out_ok || (mode != 0 && mode != 1) || m > (size_t(1) << 24)) return 2;
  if (!proofs && (!a_xy || !b_xy || !c_xy)) return 2;
  if (!groth16_vk_is_live(vk, C::ID)) return 2;
  if (vk->n_in && !inputs && !d_inputs) return 2;
  if (int rc0 = api_enter()) return rc0;
  if (vk->device != api_device()) return 101;
  const WallMs wall;
  float ms[8] = {};
  int path = 0, lanes = 1;
  const int rc = [&]() -> int {
    CallScope cs;
    HIP_TRY(cs.open(0, nullptr), 10);
    const hipStream_t s = cs.stream();
    EvLog log(s);
    typename I::DevProofs d = {};
    uint64_t* d_rows;
    uint8_t* d_flags;
    const size_t in_bytes = m * vk->n_in * C::N64 * 8;
    HIP_TRY(cs.alloc(&d_rows, m * (2 * W1 + W2) * 8), 10);
    HIP_TRY(cs.alloc(&d_flags, 4 * m), 10);
    if (d_inputs) d.inputs = const_cast<uint64_t*>(d_inputs);
    else HIP_TRY(cs.alloc(&d.inputs, in_bytes ? in_bytes : 8), 10);
    d.a = d_rows; d.c = d_rows + m * W1; d.b = d_rows + 2 * m * W1;          // (A and C adjacent: one decoder call serves both)
    d.ainf = d_flags; d.cinf = d_flags + m; d.binf = d_flags + 2 * m; d.status = d_flags + 3 * m;
    hipEvent_t e0 = log.open();
    HIP_TRY(hipMemsetAsync(d_flags, 0, 4 * m, s), 10);
    if (in_bytes && !d_inputs) HIP_TRY(hipMemcpyAsync(d.inputs, inputs, in_bytes, hipMemcpyHostToDevice, s), 10);
    if (proofs) {
      uint64_t *d_bytes, *d_g1b, *d_g2b;
      uint8_t* d_st;
      HIP_TRY(cs.alloc(&d_g1b, 2 * m * S1), 10);
      HIP_TRY(cs.alloc(&d_g2b, m * S2), 10);
      HIP_TRY(cs.alloc(&d_st, 3 * m), 10);
      HIP_TRY(cs.in(&d_bytes, proofs, m * PB, 0), 10);
      log.close(6, e0);
      e0 = log.open();
      hipLaunchKernelGGL((k_g16_split<C>), dim3((unsigned)((m * (PB / 8) + 255) / 256)), dim3(256), 0, s, d_bytes, (uint32_t)m, d_g1b, d_g2b);
      HIP_TRY(hipGetLastError(), 10);
      if (int rcd = D::decode(0, (const uint8_t*)d_g1b, 2 * m, d.a, d_st, s)) return rcd;
      if (int rcd = D::decode(1, (const uint8_t*)d_g2b, m, d.b, d_st + 2 * m, s)) return rcd;
      hipLaunchKernelGGL((k_g16_fold<C>), dim3(((uint32_t)m + 255) / 256), dim3(256), 0, s, d_st, d_st + 2 * m, (uint32_t)m, d.ainf, d.binf, d.cinf, d.status);
      HIP_TRY(hipGetLastError(), 10);
      log.close(0, e0);
    } else {
      HIP_TRY(hipMemcpyAsync(d.a, a_xy, m * W1 * 8, hipMemcpyHostToDevice, s), 10);
      HIP_TRY(hipMemcpyAsync(d.b, b_xy, m * W2 * 8, hipMemcpyHostToDevice, s), 10);
      HIP_TRY(hipMemcpyAsync(d.c, c_xy, m * W1 * 8, hipMemcpyHostToDevice, s), 10);
      if (a_inf) HIP_TRY(hipMemcpyAsync(d.ainf, a_inf, m, hipMemcpyHostToDevice, s), 10);
      if (b_inf) HIP_TRY(hipMemcpyAsync(d.binf, b_inf, m, hipMemcpyHostToDevice, s), 10);
      if (c_inf) HIP_TRY(hipMemcpyAsync(d.cinf, c_inf, m, hipMemcpyHostToDevice, s), 10);
      log.close(6, e0);
    }
    if (d_pre) {
      hipLaunchKernelGGL((k_g16_merge_status<C>), dim3(((uint32_t)m + 255) / 256), dim3(256), 0, s, d_pre, (uint32_t)m, d.status);
      HIP_TRY(hipGetLastError(), 10);
    }
    const int rcv = I::verify_core(vk, d, m, mode, key, out_ok, cs, log, ms, &path, &lanes, out_refused);
    HIP_TRY(hipStreamSynchronize(s), 10);
    log.sum(ms);
    return rcv;
  }();
  ms[5] = wall.ms();
  if (!rc) groth16_verify_note(path, vk->c, ms, lanes, (int)vk->n_in);
  return rc;
}
template <class C>
int G16Api<C>::verify(const VerifyingKey* vk, const uint64_t* a_xy, const uint8_t* a_inf, const uint64_t* b_xy, const uint8_t* b_inf, const uint64_t* c_xy,
                      const uint8_t* c_inf, const uint8_t* proofs, const uint64_t* inputs, size_t m, int mode, const uint32_t* key, uint8_t* out_ok) {
  return g16_verify_call<C>(vk, a_xy, a_inf, b_xy, b_inf, c_xy, c_inf, proofs, inputs, nullptr, nullptr, m, mode, key, out_ok, nullptr);
}
template <class C>
int G16Api<C>::verify_staged(const VerifyingKey* vk, const uint8_t* proofs, const uint64_t* d_inputs, const uint8_t* d_pre, size_t m, int mode, const uint32_t* key,
                             uint8_t* out_ok, uint8_t* out_refused) {
  if (m && (!proofs || !d_inputs)) return 2;
  return g16_verify_call<C>(vk, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, proofs, nullptr, d_inputs, d_pre, m, mode, key, out_ok, out_refused);
}

}  // namespace celo
