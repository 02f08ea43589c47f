// Translation unit: Groth16 verification over BW6-761 for m proofs under one verifying key (ark_groth16::prepare_verifying_key +
// verify_proof, crates/epoch-snark/src/api/verifier.rs:35), from the inputs to the verdict bytes on the device.  DESIGN.md section 6h.
//
//   key load     -alpha, beta, -gamma, -delta and one signed-digit window table per input base (unit_setup.hip's k_fbm_bases / k_fbm_table)
//   k_g16_inputs one lane per proof: the range test of its inputs and acc = abc_0 + sum_j x_j abc_j from the tables; k_normalize
//   each         k_g16_pack_each writes (A, B), (acc, -gamma), (C, -delta), (-alpha, beta) per proof into the pairing engine's input
//                slots: m products of four pairs, m verdicts
//   combined     exponents r_i from ChaCha20 (unit_batchverify.hip's block kernel), k_g16_scale: r_i A_i by a 128-bit ladder, two
//                m-term MSMs for sum r_i acc_i and sum r_i C_i, (sum r_i) alpha on the host; one product of m + 3 pairs.  A rejected
//                combination falls back to `each`.
// The serialized entry decodes A | B | C with the checked BW6-761 decoders (unit_wire761.hip) into the rows the kernels read.
#include "groth16_verify.h"
#include "normalize.h"
#include <hip/hip_runtime.h>
#include <sys/random.h>
#include <chrono>
#include <cstring>
#include <mutex>
#include <set>
#include <vector>
#include "runtime.h"
#include "units.h"

// one wave per SIMD, as the other 28-limb lane kernels (unit_wire761.hip): the XYZZ accumulator, the point and the addition's temporaries
#define G16_OCC __attribute__((amdgpu_waves_per_eu(1, 1)))

namespace celo {
typedef Fw761 F;
constexpr int FW = F::WORDS;

struct VerifyingKey {
  int device = 0;
  uint32_t n_in = 0;                 // public inputs: n_abc - 1
  int c = 0, W = 0;                  // window bits and windows of the input tables
  uint64_t* d_key = nullptr;         // 4 x 24 u64: -alpha, beta, -gamma, -delta (affine arkworks limbs)
  uint32_t kinf = 0;                 // bit q: row q of d_key is the identity
  uint32_t* d_abc0 = nullptr;        // gamma_abc[0] as a table entry
  bool abc0_inf = false;
  uint32_t* d_table = nullptr;       // n_in tables of W 2^(c-1) entries, base-major
  uint8_t* d_tinf = nullptr;
  uint64_t neg_alpha[24] = {};       // the host's copy for (sum r_i) alpha
  ~VerifyingKey() {
    for (void* p : {(void*)d_key, (void*)d_abc0, (void*)d_table, (void*)d_tinf}) if (p) (void)hipFree(p);
  }
};
// the handles that are alive: a freed or foreign pointer is refused, not followed
static std::mutex g_vk_mu;
static std::set<const VerifyingKey*>& vk_live() { static auto* s = new std::set<const VerifyingKey*>(); return *s; }
static bool vk_is_live(const VerifyingKey* vk) { std::lock_guard<std::mutex> lk(g_vk_mu); return vk_live().count(vk) != 0; }

// the last call: path 0 = each, 1 = combined accepted, 2 = combined rejected then each; ms: [0] decoding, [1] input sums, [2] exponents
// and ladders, [3] the two MSMs and (sum r) alpha (wall), [4] pairing products (HIP events of the engine, both passes of path 2),
// [5] wall, [6] transfers to the device
static std::mutex g_last_mu;
static struct { int path = -1, c = 0; float ms[8] = {}; } g_last;

// ---- kernels
__global__ void __launch_bounds__(64) G16_OCC
k_g16_inputs(const uint64_t* __restrict__ inputs, uint32_t m, uint32_t n_in, const uint32_t* __restrict__ abc0, int abc0_inf, const uint32_t* __restrict__ table,
             const uint8_t* __restrict__ tinf, int c, int W, uint32_t* __restrict__ xyzz, uint8_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  uint32_t bad = 0;
  const Xyzz<F> a = g16_input_row<F, 6>(inputs + (size_t)i * n_in * 6, n_in, abc0, abc0_inf != 0, table, tinf, c, W, &bad);
  uint32_t* o = xyzz + (size_t)i * 4 * FW;
  a.X.store(o); a.Y.store(o + FW); a.ZZ.store(o + 2 * FW); a.ZZZ.store(o + 3 * FW);
  if (bad) status[i] = 1;
}
// r4: the 4 x u64 the block kernel wrote per proof; sc: 6 x u64 scalars for the MSMs (zero for a proof whose status is set)
__global__ void __launch_bounds__(256) k_g16_exponents(const uint64_t* __restrict__ r4, const uint8_t* __restrict__ status, uint32_t m, uint64_t* __restrict__ sc) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  uint64_t lo, hi;
  g16_exponent(r4[(size_t)i * 4], r4[(size_t)i * 4 + 1], lo, hi);
  const uint64_t keep = status && status[i] ? 0 : ~0ull;
  uint64_t* o = sc + (size_t)i * 6;
  o[0] = lo & keep; o[1] = hi & keep; o[2] = 0; o[3] = 0; o[4] = 0; o[5] = 0;
}
__global__ void __launch_bounds__(64) G16_OCC
k_g16_scale(const uint64_t* __restrict__ a_xy, const uint8_t* __restrict__ a_inf, const uint8_t* __restrict__ status, const uint64_t* __restrict__ sc, uint32_t m,
            uint32_t* __restrict__ xyzz) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  uint32_t* o = xyzz + (size_t)i * 4 * FW;
  if (a_inf[i] || status[i]) {
    for (int q = 0; q < 4 * FW; q++) o[q] = 0;
    return;
  }
  const uint64_t* src = a_xy + (size_t)i * 24;
  const Affine<F> p = {F::norm(F::from_ark(src)), F::norm(F::from_ark(src + 12))};
  const Xyzz<F> a = g16_scale128(p, sc[(size_t)i * 6], sc[(size_t)i * 6 + 1]);
  a.X.store(o); a.Y.store(o + FW); a.ZZ.store(o + 2 * FW); a.ZZZ.store(o + 3 * FW);
}
// one lane per (proof, u64 of a row).  key: the four rows of VerifyingKey::d_key
__global__ void __launch_bounds__(256)
k_g16_pack_each(const uint64_t* __restrict__ a, const uint8_t* __restrict__ ainf, const uint64_t* __restrict__ b, const uint8_t* __restrict__ binf,
                const uint64_t* __restrict__ c, const uint8_t* __restrict__ cinf, const uint64_t* __restrict__ acc, const uint8_t* __restrict__ accinf,
                const uint8_t* __restrict__ status, const uint64_t* __restrict__ key, uint32_t kinf, uint32_t m, uint64_t* __restrict__ g1, uint64_t* __restrict__ g2,
                uint8_t* __restrict__ i1, uint8_t* __restrict__ i2) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t i = t / 24;
  const uint32_t w = (uint32_t)(t % 24);
  if (i >= m) return;
  uint64_t* o1 = g1 + i * 96 + w;
  uint64_t* o2 = g2 + i * 96 + w;
  o1[0] = a[i * 24 + w]; o1[24] = acc[i * 24 + w]; o1[48] = c[i * 24 + w]; o1[72] = key[w];
  o2[0] = b[i * 24 + w]; o2[24] = key[48 + w];     o2[48] = key[72 + w];   o2[72] = key[24 + w];
  if (w == 0) {
    const uint8_t bad = status[i] ? 1 : 0;            // (its verdict is 0 whatever the product: no pair of it is evaluated)
    i1[4 * i] = ainf[i] | bad; i1[4 * i + 1] = accinf[i] | bad; i1[4 * i + 2] = cinf[i] | bad; i1[4 * i + 3] = (uint8_t)(kinf & 1u) | bad;
    i2[4 * i] = binf[i]; i2[4 * i + 1] = (kinf >> 2) & 1u; i2[4 * i + 2] = (kinf >> 3) & 1u; i2[4 * i + 3] = (kinf >> 1) & 1u;
  }
}
// pairs 0 .. m - 1: (r_i A_i, B_i); the G2 side of pairs m, m + 1, m + 2: -gamma, -delta, beta (their G1 rows come from the host)
__global__ void __launch_bounds__(256)
k_g16_pack_combined(const uint64_t* __restrict__ ra, const uint8_t* __restrict__ rainf, const uint64_t* __restrict__ b, const uint8_t* __restrict__ binf,
                    const uint8_t* __restrict__ status, const uint64_t* __restrict__ key, uint32_t kinf, uint32_t m, uint64_t* __restrict__ g1,
                    uint64_t* __restrict__ g2, uint8_t* __restrict__ i1, uint8_t* __restrict__ i2) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t i = t / 24;
  const uint32_t w = (uint32_t)(t % 24);
  if (i >= (size_t)m + 3) return;
  if (i < m) {
    g1[i * 24 + w] = ra[i * 24 + w];
    g2[i * 24 + w] = b[i * 24 + w];
    if (w == 0) { i1[i] = rainf[i] | (status[i] ? 1 : 0); i2[i] = binf[i]; }
  } else {
    const uint32_t q = i == m ? 2u : i == (size_t)m + 1 ? 3u : 1u;
    g2[i * 24 + w] = key[q * 24 + w];
    if (w == 0) i2[i] = (kinf >> q) & 1u;
  }
}
// m proofs of 288 B (A | B | C) -> the G1 encodings (A of every proof, then C of every proof) and the G2 encodings, 96 B each;
// one lane per (proof, u64)
__global__ void __launch_bounds__(256) k_g16_split(const uint64_t* __restrict__ proofs, uint32_t m, uint64_t* __restrict__ g1b, uint64_t* __restrict__ g2b) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t i = t / 36;
  const uint32_t q = (uint32_t)(t % 36);
  if (i >= m) return;
  const uint64_t v = proofs[i * 36 + q];
  if (q < 12) g1b[i * 12 + q] = v;
  else if (q < 24) g2b[i * 12 + (q - 12)] = v;
  else g1b[((size_t)m + i) * 12 + (q - 24)] = v;
}
// decoder statuses (wire.h: 0 ok, 1 infinity, 2 invalid, 3 outside the subgroup) -> identity flags and the proof's status
__global__ void __launch_bounds__(256) k_g16_fold(const uint8_t* __restrict__ st_ac, const uint8_t* __restrict__ st_b, uint32_t m, uint8_t* __restrict__ ainf,
                                                  uint8_t* __restrict__ binf, uint8_t* __restrict__ cinf, uint8_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint8_t sa = st_ac[i], sc = st_ac[(size_t)m + i], sb = st_b[i];
  ainf[i] = sa == WIRE_INFINITY; binf[i] = sb == WIRE_INFINITY; cinf[i] = sc == WIRE_INFINITY;
  status[i] = (sa >= WIRE_INVALID || sb >= WIRE_INVALID || sc >= WIRE_INVALID) ? 1 : 0;
}

// ---- key load
static int vk_build(const uint64_t* rows /* alpha, beta, gamma, delta, abc[n_abc]: 24 u64 each */, const uint8_t* inf /* or NULL */, size_t n_abc, VerifyingKey** out) {
  if (int rc0 = api_enter()) return rc0;
  std::unique_ptr<VerifyingKey> vk(new VerifyingKey);
  vk->device = api_device();
  vk->n_in = (uint32_t)(n_abc - 1);
  vk->c = g16_window_bits(vk->n_in);
  vk->W = fb_windows(G16_SCALAR_BITS, vk->c);
  uint64_t key[4 * 24];
  memcpy(key, rows, sizeof key);
  std::vector<uint8_t> rinf(4 + n_abc);
  for (size_t i = 0; i < 4 + n_abc; i++) rinf[i] = (inf && inf[i]) || g16_row_is_identity(rows + i * 24);
  for (int q = 0; q < 4; q++) {
    if (rinf[q]) { memset(key + q * 24, 0, 24 * 8); vk->kinf |= 1u << q; }
    else if (q != 1) g16_negate_row(key + q * 24);                          // -alpha, beta, -gamma, -delta
  }
  memcpy(vk->neg_alpha, key, sizeof vk->neg_alpha);
  uint32_t abc0[2 * FW] = {};
  vk->abc0_inf = rinf[4] != 0;
  if (!vk->abc0_inf) fb_store_entry(abc0, Affine<F>{F::norm(F::from_ark(rows + 96)), F::norm(F::from_ark(rows + 108))});
  const size_t E = (size_t)vk->W << (vk->c - 1);
  HIP_TRY(hipMalloc(&vk->d_key, sizeof key), 10);
  HIP_TRY(hipMalloc(&vk->d_abc0, sizeof abc0), 10);
  HIP_TRY(hipMalloc(&vk->d_table, (vk->n_in ? vk->n_in : 1) * E * 2 * FW * 4), 10);
  HIP_TRY(hipMalloc(&vk->d_tinf, (vk->n_in ? vk->n_in : 1) * E), 10);
  {
    CallScope cs(nullptr);
    HIP_TRY(cs.create_stream(), 10);
    HIP_TRY(hipMemcpyAsync(vk->d_key, key, sizeof key, hipMemcpyHostToDevice, cs.stream()), 10);
    HIP_TRY(hipMemcpyAsync(vk->d_abc0, abc0, sizeof abc0, hipMemcpyHostToDevice, cs.stream()), 10);
    if (int rc = fixed_base_tables_761(rows + 5 * 24, rinf.data() + 5, vk->n_in, vk->c, vk->d_table, vk->d_tinf, cs.stream())) return rc;
    HIP_TRY(hipStreamSynchronize(cs.stream()), 10);
  }
  { std::lock_guard<std::mutex> lk(g_vk_mu); vk_live().insert(vk.get()); }
  *out = vk.release();
  return 0;
}
int groth16_vk_load_761(const uint64_t* alpha_g1, const uint64_t* beta_g2, const uint64_t* gamma_g2, const uint64_t* delta_g2, const uint64_t* gamma_abc_g1, size_t n_abc,
                        VerifyingKey** out) {
  if (!out) return 2;
  *out = nullptr;
  if (!alpha_g1 || !beta_g2 || !gamma_g2 || !delta_g2 || !gamma_abc_g1 || n_abc == 0) return 2;
  if (n_abc - 1 > G16_MAX_INPUTS) return G16_ERR_INPUTS;
  std::vector<uint64_t> rows((4 + n_abc) * 24);
  memcpy(rows.data(), alpha_g1, 192); memcpy(rows.data() + 24, beta_g2, 192); memcpy(rows.data() + 48, gamma_g2, 192); memcpy(rows.data() + 72, delta_g2, 192);
  memcpy(rows.data() + 96, gamma_abc_g1, n_abc * 192);
  return vk_build(rows.data(), nullptr, n_abc, out);
}
int groth16_vk_load_761_serialized(const uint8_t* bytes, size_t len, VerifyingKey** out) {
  if (!out) return 2;
  *out = nullptr;
  std::vector<uint64_t> rows;
  std::vector<uint8_t> inf;
  if (int rc = g16_vk_parse(bytes, len, rows, inf, nullptr)) return rc;
  return vk_build(rows.data(), inf.data(), inf.size() - 4, out);
}
int groth16_vk_release(VerifyingKey* vk) {
  if (!vk) return 2;
  {
    std::lock_guard<std::mutex> lk(g_vk_mu);
    if (!vk_live().erase(vk)) return 2;
  }
  delete vk;
  return 0;
}

// ---- host pieces of the combined check
static void jac_to_row(const uint64_t* jac, uint64_t* row, uint8_t* inf) {
  const F Z = F::norm(F::from_ark(jac + 24));
  *inf = Z.is_zero_mod_p() ? 1 : 0;
  for (int q = 0; q < 24; q++) row[q] = 0;
  if (*inf) return;
  const F zi = F::norm(F::inv(Z)), zi2 = F::norm(F::sqr(zi));
  F::mul(F::from_ark(jac), zi2).to_ark(row);
  F::mul(F::from_ark(jac + 12), F::norm(F::mul(zi2, zi))).to_ark(row + 12);
}
// k P for k of three little-endian u64 (a sum of at most 2^24 exponents of 128 bits), P affine arkworks limbs: MSB-first over XYZZ
static void mul_row(const uint64_t* xy, const uint64_t k[3], uint64_t* row, uint8_t* inf) {
  const Affine<F> p = {F::norm(F::from_ark(xy)), F::norm(F::from_ark(xy + 12))};
  Xyzz<F> acc = Xyzz<F>::identity();
  for (int i = 191; i >= 0; i--) {
    acc = xyzz_dbl(acc);
    if ((k[i >> 6] >> (i & 63)) & 1) xyzz_madd(acc, p);
  }
  Affine<F> r = {F::zero(), F::zero()};
  for (int q = 0; q < 24; q++) row[q] = 0;
  *inf = fb_to_affine(acc, r) ? 0 : 1;
  if (!*inf) { r.x.to_ark(row); r.y.to_ark(row + 12); }
}

struct StageGuard {      // an engine that was staged and not run goes back to its pool
  PairingStage ps;
  ~StageGuard() { if (ps.lease) (void)pairing_run_staged_761(&ps, nullptr, 0, nullptr); }
};
struct DevProofs { uint64_t *a, *b, *c, *inputs, *acc; uint8_t *ainf, *binf, *cinf, *accinf, *status; };

// m products of four pairs; is_one: m host bytes.  The producer stream s is chained in front of the engine's by an event.
static int run_each(const VerifyingKey* vk, const DevProofs& d, size_t m, CallScope& cs, uint8_t* is_one, float* ms_pair) {
  StageGuard g;
  if (int rc = pairing_stage_761((uint32_t)(4 * m), m, &g.ps)) return rc;
  hipEvent_t ready;
  HIP_TRY(cs.event(&ready), 10);
  HIP_TRY(hipEventRecord(ready, cs.stream()), 10);
  HIP_TRY(hipStreamWaitEvent(g.ps.stream, ready, 0), 10);
  hipLaunchKernelGGL(k_g16_pack_each, dim3((unsigned)((m * 24 + 255) / 256)), dim3(256), 0, g.ps.stream, d.a, d.ainf, d.b, d.binf, d.c, d.cinf, d.acc, d.accinf, d.status,
                     vk->d_key, vk->kinf, (uint32_t)m, g.ps.d_g1, g.ps.d_g2, g.ps.d_i1, g.ps.d_i2);
  HIP_TRY(hipGetLastError(), 10);
  std::vector<uint32_t> off(m + 1);
  for (size_t p = 0; p <= m; p++) off[p] = (uint32_t)(4 * p);
  if (int rc = pairing_run_staged_761(&g.ps, off.data(), m, is_one)) return rc;      // synchronises the engine's stream, and s through the event
  float pm[4];
  pairing_timings_761(pm);
  *ms_pair += pm[3];
  return 0;
}

// Everything after the proofs' rows, identity flags, statuses and inputs are on the device (stream cs.stream()).
static int verify_core(const VerifyingKey* vk, DevProofs& d, size_t m, int mode, const uint32_t* key, uint8_t* out_ok, CallScope& cs, EvLog& log, float* ms, int* path) {
  const hipStream_t s = cs.stream();
  const uint32_t m32 = (uint32_t)m, wblocks = (m32 + 63) / 64;
  constexpr int K = 4;                                   // rows per lane of the normalisation (unit_setup.hip's choice for the 28-limb field)
  const unsigned nblocks = ((m32 + K - 1) / K + 63) / 64;
  uint32_t* d_xyzz;
  std::vector<uint8_t> h_status(m), is_one(m);
  HIP_TRY(cs.alloc(&d_xyzz, m * 4 * FW * 4), 10);
  HIP_TRY(cs.alloc(&d.acc, m * 24 * 8), 10);
  HIP_TRY(cs.alloc(&d.accinf, m), 10);
  hipEvent_t e0 = log.open();
  hipLaunchKernelGGL(k_g16_inputs, dim3(wblocks), dim3(64), 0, s, d.inputs, m32, vk->n_in, vk->d_abc0, vk->abc0_inf ? 1 : 0, vk->d_table, vk->d_tinf, vk->c, vk->W, d_xyzz,
                     d.status);
  hipLaunchKernelGGL((k_normalize<F, K, false, 0, true>), dim3(nblocks), dim3(64), 0, s, (const void*)d_xyzz, d.acc, d.accinf, m32, 0);
  log.close(1, e0);
  HIP_TRY(hipGetLastError(), 10);
  HIP_TRY(hipMemcpyAsync(h_status.data(), d.status, m, hipMemcpyDeviceToHost, s), 10);
  *path = 0;
  if (mode == 1) {
    uint32_t k8[8];
    if (key) memcpy(k8, key, sizeof k8);
    else {                                               // 32 bytes from the operating system per call, as batch_verify_strict's exponent stream
      size_t got = 0;
      while (got < sizeof k8) {
        const ssize_t r = getrandom((uint8_t*)k8 + got, sizeof k8 - got, 0);
        if (r <= 0) return 1;
        got += (size_t)r;
      }
    }
    uint64_t *d_r4, *d_sc, *d_ra;
    uint32_t* d_off;
    uint8_t* d_rainf;
    const uint32_t off2[2] = {0, m32};
    std::vector<uint64_t> h_r4(m * 4);
    HIP_TRY(cs.alloc(&d_r4, m * 32), 10);
    HIP_TRY(cs.alloc(&d_sc, m * 48), 10);
    HIP_TRY(cs.alloc(&d_ra, m * 24 * 8), 10);
    HIP_TRY(cs.alloc(&d_rainf, m), 10);
    HIP_TRY(cs.alloc(&d_off, 8), 10);
    HIP_TRY(hipMemcpyAsync(d_off, off2, 8, hipMemcpyHostToDevice, s), 10);
    e0 = log.open();
    // block i of the stream, its first 16 bytes: one "batch" of m signers makes the block kernel keep (128 + log2 m + 7) / 8 >= 16 bytes
    if (int rc = bv_draw_exponents(k8, d_off, 1, m, d_r4, s)) return rc;
    hipLaunchKernelGGL(k_g16_exponents, dim3((m32 + 255) / 256), dim3(256), 0, s, d_r4, d.status, m32, d_sc);
    hipLaunchKernelGGL(k_g16_scale, dim3(wblocks), dim3(64), 0, s, d.a, d.ainf, d.status, d_sc, m32, d_xyzz);
    hipLaunchKernelGGL((k_normalize<F, K, false, 0, true>), dim3(nblocks), dim3(64), 0, s, (const void*)d_xyzz, d_ra, d_rainf, m32, 0);
    log.close(2, e0);
    HIP_TRY(hipGetLastError(), 10);
    HIP_TRY(hipMemcpyAsync(h_r4.data(), d_r4, m * 32, hipMemcpyDeviceToHost, s), 10);
    // sum r_i acc_i, sum r_i C_i: the variable-base MSM over the rows where they lie, the same scalars (zero for a proof whose status is set)
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t jac[2][36], tail[3 * 24];
    uint8_t tinf[3];
    if (int rc = MsmApi<G_761>::dev(d.acc, d.accinf, d_sc, m, 0, jac[0], s)) return rc;
    if (int rc = MsmApi<G_761>::dev(d.c, d.cinf, d_sc, m, 0, jac[1], s)) return rc;
    HIP_TRY(hipStreamSynchronize(s), 10);                 // (the MSM calls return their sums to the host: s has drained already)
    jac_to_row(jac[0], tail, &tinf[0]);
    jac_to_row(jac[1], tail + 24, &tinf[1]);
    uint64_t sum[3] = {0, 0, 0};
    for (size_t i = 0; i < m; i++) {
      if (h_status[i]) continue;
      uint64_t lo, hi;
      g16_exponent(h_r4[i * 4], h_r4[i * 4 + 1], lo, hi);
      const unsigned __int128 t = (unsigned __int128)sum[0] + lo;
      const unsigned __int128 u = (unsigned __int128)sum[1] + hi + (uint64_t)(t >> 64);
      sum[0] = (uint64_t)t; sum[1] = (uint64_t)u; sum[2] += (uint64_t)(u >> 64);
    }
    if (vk->kinf & 1u) { memset(tail + 48, 0, 192); tinf[2] = 1; }
    else mul_row(vk->neg_alpha, sum, tail + 48, &tinf[2]);
    ms[3] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    int one = 0;
    {
      StageGuard g;
      if (int rc = pairing_stage_761(m32 + 3, 1, &g.ps)) return rc;
      hipLaunchKernelGGL(k_g16_pack_combined, dim3((unsigned)(((m + 3) * 24 + 255) / 256)), dim3(256), 0, g.ps.stream, d_ra, d_rainf, d.b, d.binf, d.status, vk->d_key,
                         vk->kinf, m32, g.ps.d_g1, g.ps.d_g2, g.ps.d_i1, g.ps.d_i2);
      HIP_TRY(hipGetLastError(), 10);
      HIP_TRY(hipMemcpyAsync(g.ps.d_g1 + m * 24, tail, sizeof tail, hipMemcpyHostToDevice, g.ps.stream), 10);
      HIP_TRY(hipMemcpyAsync(g.ps.d_i1 + m, tinf, 3, hipMemcpyHostToDevice, g.ps.stream), 10);
      const uint32_t off[2] = {0, m32 + 3};
      uint8_t v = 0;
      if (int rc = pairing_run_staged_761(&g.ps, off, 1, &v)) return rc;
      float pm[4];
      pairing_timings_761(pm);
      ms[4] += pm[3];
      one = v;
    }
    if (one) {
      for (size_t i = 0; i < m; i++) out_ok[i] = h_status[i] ? 0 : 1;
      *path = 1;
      return 0;
    }
    *path = 2;
  }
  if (int rc = run_each(vk, d, m, cs, is_one.data(), &ms[4])) return rc;
  for (size_t i = 0; i < m; i++) out_ok[i] = (is_one[i] && !h_status[i]) ? 1 : 0;
  return 0;
}

// proofs != NULL: the serialized entry (m x 288 B, a_xy .. c_inf unused); else the limb entry
int groth16_verify_761(const VerifyingKey* vk, const uint64_t* a_xy, const uint8_t* a_inf, const uint64_t* b_xy, const uint8_t* b_inf, const uint64_t* c_xy,
                       const uint8_t* c_inf, const uint8_t* proofs, const uint64_t* inputs, size_t m, int mode, const uint32_t* key, uint8_t* out_ok) {
  if (m == 0) return 0;
  if (!vk || !out_ok || (mode != 0 && mode != 1) || m > (size_t(1) << 24)) return 2;
  if (!proofs && (!a_xy || !b_xy || !c_xy)) return 2;
  if (!vk_is_live(vk)) return 2;
  if (vk->n_in && !inputs) return 2;
  if (int rc0 = api_enter()) return rc0;
  if (vk->device != api_device()) return 101;
  const auto t0 = std::chrono::steady_clock::now();
  float ms[8] = {};
  int path = 0;
  const int rc = [&]() -> int {
    CallScope cs(nullptr);
    HIP_TRY(cs.create_stream(), 10);
    const hipStream_t s = cs.stream();
    EvLog log(s);
    DevProofs d = {};
    uint64_t* d_rows;
    uint8_t* d_flags;
    const size_t in_bytes = m * vk->n_in * 48;
    HIP_TRY(cs.alloc(&d_rows, m * 3 * 24 * 8), 10);
    HIP_TRY(cs.alloc(&d_flags, 4 * m), 10);
    HIP_TRY(cs.alloc(&d.inputs, in_bytes ? in_bytes : 8), 10);
    d.a = d_rows; d.c = d_rows + m * 24; d.b = d_rows + 2 * m * 24;          // (A and C adjacent: one decoder call serves both)
    d.ainf = d_flags; d.cinf = d_flags + m; d.binf = d_flags + 2 * m; d.status = d_flags + 3 * m;
    hipEvent_t e0 = log.open();
    HIP_TRY(hipMemsetAsync(d_flags, 0, 4 * m, s), 10);
    if (in_bytes) HIP_TRY(hipMemcpyAsync(d.inputs, inputs, in_bytes, hipMemcpyHostToDevice, s), 10);
    if (proofs) {
      uint64_t *d_bytes, *d_g1b, *d_g2b;
      uint8_t* d_st;
      HIP_TRY(cs.alloc(&d_bytes, m * 288), 10);
      HIP_TRY(cs.alloc(&d_g1b, 2 * m * 96), 10);
      HIP_TRY(cs.alloc(&d_g2b, m * 96), 10);
      HIP_TRY(cs.alloc(&d_st, 3 * m), 10);
      HIP_TRY(hipMemcpyAsync(d_bytes, proofs, m * 288, hipMemcpyHostToDevice, s), 10);
      log.close(6, e0);
      e0 = log.open();
      hipLaunchKernelGGL(k_g16_split, dim3((unsigned)((m * 36 + 255) / 256)), dim3(256), 0, s, d_bytes, (uint32_t)m, d_g1b, d_g2b);
      HIP_TRY(hipGetLastError(), 10);
      if (int rcd = wire761_decode(0, 1, (const uint8_t*)d_g1b, 2 * m, 1, d.a, d_st, 1, s)) return rcd;
      if (int rcd = wire761_decode(1, 1, (const uint8_t*)d_g2b, m, 1, d.b, d_st + 2 * m, 1, s)) return rcd;
      hipLaunchKernelGGL(k_g16_fold, dim3(((uint32_t)m + 255) / 256), dim3(256), 0, s, d_st, d_st + 2 * m, (uint32_t)m, d.ainf, d.binf, d.cinf, d.status);
      HIP_TRY(hipGetLastError(), 10);
      log.close(0, e0);
    } else {
      HIP_TRY(hipMemcpyAsync(d.a, a_xy, m * 192, hipMemcpyHostToDevice, s), 10);
      HIP_TRY(hipMemcpyAsync(d.b, b_xy, m * 192, hipMemcpyHostToDevice, s), 10);
      HIP_TRY(hipMemcpyAsync(d.c, c_xy, m * 192, hipMemcpyHostToDevice, s), 10);
      if (a_inf) HIP_TRY(hipMemcpyAsync(d.ainf, a_inf, m, hipMemcpyHostToDevice, s), 10);
      if (b_inf) HIP_TRY(hipMemcpyAsync(d.binf, b_inf, m, hipMemcpyHostToDevice, s), 10);
      if (c_inf) HIP_TRY(hipMemcpyAsync(d.cinf, c_inf, m, hipMemcpyHostToDevice, s), 10);
      log.close(6, e0);
    }
    const int rcv = verify_core(vk, d, m, mode, key, out_ok, cs, log, ms, &path);
    HIP_TRY(hipStreamSynchronize(s), 10);
    log.sum(ms);
    return rcv;
  }();
  ms[5] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (!rc) {
    std::lock_guard<std::mutex> lk(g_last_mu);
    g_last.path = path; g_last.c = vk->c;
    for (int i = 0; i < 8; i++) g_last.ms[i] = ms[i];
  }
  return rc;
}

// tests / tooling: the exponents a combined call under `key` gives its m proofs, 2 x u64 each, on the host
int groth16_draw_exponents_run(const uint32_t key[8], size_t m, uint64_t* out) {
  if (!key || (m && !out) || m > (size_t(1) << 24)) return 2;
  if (int rc = api_enter()) return rc;
  if (m == 0) return 0;
  CallScope cs(nullptr);
  HIP_TRY(cs.create_stream(), 10);
  uint32_t* d_off;
  uint64_t *d_r4, *d_sc;
  const uint32_t off2[2] = {0, (uint32_t)m};
  std::vector<uint64_t> h(m * 6);
  HIP_TRY(cs.alloc(&d_off, 8), 10);
  HIP_TRY(cs.alloc(&d_r4, m * 32), 10);
  HIP_TRY(cs.alloc(&d_sc, m * 48), 10);
  HIP_TRY(hipMemcpyAsync(d_off, off2, 8, hipMemcpyHostToDevice, cs.stream()), 10);
  if (int rc = bv_draw_exponents(key, d_off, 1, m, d_r4, cs.stream())) return rc;
  hipLaunchKernelGGL(k_g16_exponents, dim3(((uint32_t)m + 255) / 256), dim3(256), 0, cs.stream(), d_r4, (const uint8_t*)nullptr, (uint32_t)m, d_sc);
  HIP_TRY(hipGetLastError(), 10);
  HIP_TRY(hipMemcpyAsync(h.data(), d_sc, m * 48, hipMemcpyDeviceToHost, cs.stream()), 10);
  HIP_TRY(hipStreamSynchronize(cs.stream()), 10);
  for (size_t i = 0; i < m; i++) { out[2 * i] = h[6 * i]; out[2 * i + 1] = h[6 * i + 1]; }
  return 0;
}

int groth16_verify_last(int* path, int* window_bits, float ms[8]) {
  std::lock_guard<std::mutex> lk(g_last_mu);
  if (path) *path = g_last.path;
  if (window_bits) *window_bits = g_last.c;
  if (ms) for (int i = 0; i < 8; i++) ms[i] = g_last.ms[i];
  return 0;
}

}  // namespace celo
