// Translation unit: batched fixed-base scalar multiplication (fixed_base.h) for the four groups, and Groth16 parameter generation after
// the QAP evaluation at tau (ark-groth16 0.1 generate_parameters, reached through crates/epoch-snark/src/api/setup.rs:22-46,63-105) - from
// the caller's vectors, or from constraint matrices through unit_r1cs.hip (groth16_setup_r1cs).
// DESIGN.md section 6f.
#include "fixed_base.h"
#include "normalize.h"
#include <hip/hip_runtime.h>
#include <cstring>
#include <mutex>
#include <vector>
#include "runtime.h"
#include "units.h"

namespace celo {
typedef Fp<P377> FrBw6;          // the scalar field of BW6-761 (the base field of BLS12-377)
typedef Fp<P253> FrBls;          // the scalar field of BLS12-377

// calls from several host threads are serialised per process (bulk calls: one fills the GPU).  Guards the setting g_fb_c
static std::mutex setup_mu;
// window bits of the generator tables: 0 = the default (FB_DEFAULT_C), else 2 .. 14 (celo_amd_fixed_base_set_window, for the A/B of DESIGN 6f)
static int g_fb_c = 0;
static constexpr int FB_DEFAULT_C = 10;   // same-box A/B on 2^20 BW6-761 G1 rows: c = 6 36.7 ms, 8 28.7, 10 22.6
// the last call's timings in ms: [0] table build, [1] Fr preparation, [2] G1 rows, [3] G2 rows, [4] normalisation, [5] key tables, [6] wall
static Last<CallTimes> g_setup_last;

template <class FR> struct FrParams;
template <class P> struct FrParams<Fp<P>> { typedef P type; };

// ---- table build (fixed_base.h).  k_fbm_bases: lane w -> 2^(c w) G, affine (bases: W x 2 FW words; binf: W flags).
template <class F>
__global__ void __launch_bounds__(64) k_fbm_bases(ArkWords<2 * F::ARK64> gen, uint32_t* __restrict__ bases, uint8_t* __restrict__ binf, int W, int c) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= W) return;
  const Affine<F> g = {F::norm(F::from_ark(gen.v)), F::norm(F::from_ark(gen.v + F::ARK64))};
  Affine<F> b = {F::zero(), F::zero()};
  const bool ok = fb_to_affine(fb_window_base(g, w, c), b);
  fb_store_entry(bases + (size_t)w * 2 * F::WORDS, b);
  binf[w] = ok ? 0 : 1;
}
// lane e = w H + d - 1 -> d 2^(c w) G, affine, canonical coordinates
template <class F>
__global__ void __launch_bounds__(64) k_fbm_table(const uint32_t* __restrict__ bases, const uint8_t* __restrict__ binf, uint32_t* __restrict__ table,
                                                  uint8_t* __restrict__ tinf, uint32_t H, uint32_t E) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const uint32_t w = e / H, d = e - w * H + 1;
  Affine<F> r = {F::zero(), F::zero()};
  bool ok = false;
  if (!binf[w]) ok = fb_to_affine(fb_table_entry(fb_load_entry<F>(bases + (size_t)w * 2 * F::WORDS), d), r);
  fb_store_entry(table + (size_t)e * 2 * F::WORDS, r);
  tinf[e] = ok ? 0 : 1;
}
// one lane per scalar: k_i G in XYZZ (device form, 4 FW words per row)
template <class F, int N64>
__global__ void __launch_bounds__(256) k_fbm_rows(const uint64_t* __restrict__ sc, uint32_t n, const uint32_t* __restrict__ table, const uint8_t* __restrict__ tinf,
                                                  int c, int W, uint32_t* __restrict__ xyzz) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t s[N64];
#pragma unroll
  for (int k = 0; k < N64; k++) s[k] = sc[(size_t)i * N64 + k];
  const Xyzz<F> a = fb_scalar_mul<F, N64>(s, table, tinf, c, W);
  uint32_t* o = xyzz + (size_t)i * 4 * F::WORDS;
  a.X.store(o); a.Y.store(o + F::WORDS); a.ZZ.store(o + 2 * F::WORDS); a.ZZZ.store(o + 3 * F::WORDS);
}

// ---- the Groth16 setup's scalars (fixed_base.h setup_*), written where the fixed-base kernels read them: the G1 scalar list is
// [alpha, beta, delta, gamma_abc (n_inputs), a (n_vars), b (n_vars), h (n_h), l (n_vars - n_inputs)], the G2 list [beta, gamma, delta, b (n_vars)]
// (the first three of each come from the host); one lane per variable.
template <class FR>
__global__ void __launch_bounds__(256) k_setup_fr(const uint64_t* __restrict__ qa, const uint64_t* __restrict__ qb, const uint64_t* __restrict__ qc, uint32_t n_vars,
                                                  uint32_t n_inputs, FR alpha, FR beta, FR ginv, FR dinv, uint64_t* __restrict__ g1s, uint64_t* __restrict__ g2s,
                                                  uint32_t n_h) {
  constexpr int A = FR::ARK64;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_vars) return;
  const size_t off_abc = 3, off_a = off_abc + n_inputs, off_b = off_a + n_vars, off_l = off_b + n_vars + n_h;
  const bool inst = i < n_inputs;
  setup_lc<FR>(qa + (size_t)i * A, qb + (size_t)i * A, qc + (size_t)i * A, alpha, beta, inst ? ginv : dinv,
               g1s + (inst ? off_abc + i : off_l + (i - n_inputs)) * A);
  setup_canon<FR>(qa + (size_t)i * A, g1s + (off_a + i) * A);
  setup_canon<FR>(qb + (size_t)i * A, g1s + (off_b + i) * A);
  setup_canon<FR>(qb + (size_t)i * A, g2s + (3 + (size_t)i) * A);
}
// h_i = zt delta^-1 tau^i, blocks of SETUP_H_BLOCK rows per lane (each lane starts at tau^(block start))
template <class FR>
__global__ void __launch_bounds__(256) k_setup_h(FR zt_dinv, FR tau, uint32_t n_h, uint64_t* __restrict__ out) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t i0 = (uint64_t)b * SETUP_H_BLOCK;
  if (i0 >= n_h) return;
  const uint32_t cnt = n_h - i0 < SETUP_H_BLOCK ? (uint32_t)(n_h - i0) : SETUP_H_BLOCK;
  setup_h_block<FR>(zt_dinv, tau, i0, cnt, out + i0 * FR::ARK64);
}

// ---- one group: G = the group's coordinate field F, N64 u64 per scalar, BITS scalar bits, R the group order's limbs
template <class F, int N64, int BITS> struct Fbm {
  typedef F Fc;
  static constexpr int A = F::ARK64;
  uint32_t* table = nullptr;
  uint8_t* tinf = nullptr;
  int c = FB_DEFAULT_C, W = 0;
  uint32_t H = 0;
  ~Fbm() { if (table) (void)hipFree(table); if (tinf) (void)hipFree(tinf); }
  // the generator's table (gen: affine arkworks limbs, not the identity)
  int build(const uint64_t* gen, hipStream_t s, EvLog* log) {
    CallScope cs(s);
    uint32_t* bases;
    uint8_t* binf;
    ArkWords<2 * A> g;
    c = g_fb_c ? g_fb_c : FB_DEFAULT_C;
    W = fb_windows(BITS, c);
    H = 1u << (c - 1);
    const uint32_t E = (uint32_t)W * H;
    memcpy(g.v, gen, sizeof g.v);
    HIP_TRY(cs.alloc(&bases, (size_t)W * 2 * F::WORDS * 4), 10);
    HIP_TRY(cs.alloc(&binf, W), 10);
    HIP_TRY(hipMalloc(&table, (size_t)E * 2 * F::WORDS * 4), 10);
    HIP_TRY(hipMalloc(&tinf, E), 10);
    hipEvent_t e0 = log->open();
    hipLaunchKernelGGL((k_fbm_bases<F>), dim3((W + 63) / 64), dim3(64), 0, s, g, bases, binf, W, c);
    hipLaunchKernelGGL((k_fbm_table<F>), dim3((E + 63) / 64), dim3(64), 0, s, bases, binf, table, tinf, H, E);
    log->close(0, e0);
    HIP_TRY(hipGetLastError(), 10);
    HIP_TRY(hipStreamSynchronize(s), 10);
    return 0;
  }
  // n rows from n canonical device scalars into device rows (2 A u64 each) and flags, in chunks that bound the XYZZ scratch buffer.
  // cat: the timing slot of the scalar kernel (2 = G1, 3 = G2); the normalisation goes to slot 4.
  int rows(const uint64_t* d_sc, size_t n, uint64_t* d_out, uint8_t* d_inf, int ark_zero_y, hipStream_t s, EvLog* log, int cat) {
    constexpr size_t CHUNK = size_t(1) << 20;
    if (n == 0) return 0;
    CallScope cs(s);
    uint32_t* tmp;
    const size_t m = n < CHUNK ? n : CHUNK;
    HIP_TRY(cs.alloc(&tmp, m * 4 * F::WORDS * 4), 10);
    for (size_t lo = 0; lo < n; lo += CHUNK) {
      const uint32_t k = (uint32_t)(n - lo < CHUNK ? n - lo : CHUNK);
      hipEvent_t e0 = log->open();
      hipLaunchKernelGGL((k_fbm_rows<F, N64>), dim3((k + 255) / 256), dim3(256), 0, s, d_sc + lo * N64, k, table, tinf, c, W, tmp);
      log->close(cat, e0);
      e0 = log->open();
      normalize_xyzz<F, true>(tmp, d_out + lo * 2 * A, d_inf + lo, k, ark_zero_y, s);
      log->close(4, e0);
      HIP_TRY(hipGetLastError(), 10);
    }
    HIP_TRY(hipStreamSynchronize(s), 10);
    return 0;
  }
};
typedef Fbm<Fp<P377>, 4, 253> FbmG1_377;
typedef Fbm<Fp2<P377>, 4, 253> FbmG2_377;
typedef Fbm<Fp<P761>, 6, 377> Fbm761;

// arkworks' identity as coordinates (x = 0 and y = 0 or 1): not a generator
template <class F> static bool gen_is_identity(const uint64_t* xy) {
  constexpr int A = F::ARK64;
  uint64_t one[A];
  F::one().to_ark(one);
  bool x0 = true, y0 = true, y1 = true;
  for (int k = 0; k < A; k++) { x0 = x0 && xy[k] == 0; y0 = y0 && xy[A + k] == 0; y1 = y1 && xy[A + k] == one[k]; }
  return x0 && (y0 || y1);
}

// out[i] = k_i G.  scalars / out / inf: host or device pointers (runtime.h, the call frame).  A scalar >= r: 2, nothing written.
template <class FB, class FR>
static int fbm_mul(const uint64_t* gen, const void* scalars, size_t n, void* out_xy, void* inf, int dev, void* stream_) {
  typedef typename FB::Fc F;
  constexpr int N64 = FR::ARK64, RW = 2 * FB::A;
  if (int rc0 = api_enter()) return rc0;
  if (!gen || (n && (!scalars || !out_xy || !inf)) || n > 0x7fffffffu) return 2;
  if (gen_is_identity<F>(gen)) return 2;
  std::lock_guard<std::mutex> lk(setup_mu);
  if (n == 0) return 0;
  if (!dev) {
    const uint64_t* sc = (const uint64_t*)scalars;
    for (size_t i = 0; i < n; i++) if (!fb_below<N64>(sc + i * N64, FrParams<FR>::type::P64)) return 2;
  }
  TimedCall call(g_setup_last, 6);
  CallScope cs;
  HIP_TRY(cs.open(dev, stream_), 10);
  EvLog log(cs.stream());
  FB fb;
  uint64_t *d_sc, *d_out;
  uint8_t* d_inf;
  if (dev) if (int rcs = scalars_below_order<N64>((const uint64_t*)scalars, n, FrParams<FR>::type::P64, cs)) return rcs;
  HIP_TRY(cs.in(&d_sc, scalars, n * N64 * 8, dev), 10);
  HIP_TRY(cs.out(&d_out, out_xy, n * RW * 8, dev), 10);
  HIP_TRY(cs.out(&d_inf, inf, n, dev), 10);
  if (int rcb = fb.build(gen, cs.stream(), &log)) return rcb;
  if (int rcr = fb.rows(d_sc, n, d_out, d_inf, 0, cs.stream(), &log, 2)) return rcr;
  HIP_TRY(cs.copy_back(), 10);
  HIP_TRY(hipStreamSynchronize(cs.stream()), 10);
  log.sum(call.t.ms);
  return 0;
}

int fixed_base_mul(int group, const uint64_t* gen, const void* scalars, size_t n, void* out_xy, void* inf, int dev, void* stream) {
  switch (group) {
    case 0: return fbm_mul<FbmG1_377, FrBls>(gen, scalars, n, out_xy, inf, dev, stream);
    case 1: return fbm_mul<FbmG2_377, FrBls>(gen, scalars, n, out_xy, inf, dev, stream);
    case 2: return fbm_mul<Fbm761, FrBw6>(gen, scalars, n, out_xy, inf, dev, stream);
    default: return 2;
  }
}
int fixed_base_set_window(int c) {
  if (c != 0 && (c < 2 || c > 14)) return 2;
  std::lock_guard<std::mutex> lk(setup_mu);
  g_fb_c = c;
  return 0;
}
void setup_last_timings(float ms[8]) { const CallTimes t = g_setup_last.read(); for (int i = 0; i < 8; i++) ms[i] = t.ms[i]; }

// The table of k_fbm_bases / k_fbm_table for each of n bases over the field F instead of one generator (the Groth16 verifier's gamma_abc rows,
// groth16_verify_unit.h): gens n x 2 F::ARK64 u64 affine arkworks limbs and inf their identity flags, both on the HOST; d_table n x W 2^(c-1)
// entries and d_tinf their flags on the device, base-major, W = fb_windows(scalar_bits, c).  An identity base's entries are all flagged.
// Enqueued on s; returns after the stream has drained (the window bases are the call's own scratch).
template <class F>
int fixed_base_tables(const uint64_t* gens, const uint8_t* inf, size_t n, int scalar_bits, int c, uint32_t* d_table, uint8_t* d_tinf, hipStream_t s) {
  constexpr int A = F::ARK64;
  if (n == 0) return 0;
  if (!gens || !d_table || !d_tinf || c < 2 || c > 14) return 2;
  const int W = fb_windows(scalar_bits, c);
  const uint32_t H = 1u << (c - 1), E = (uint32_t)W * H;
  CallScope cs(s);
  uint32_t* bases;
  uint8_t* binf;
  HIP_TRY(cs.alloc(&bases, (size_t)W * 2 * F::WORDS * 4), 10);
  HIP_TRY(cs.alloc(&binf, W), 10);
  for (size_t b = 0; b < n; b++) {
    uint32_t* t = d_table + b * (size_t)E * 2 * F::WORDS;
    uint8_t* ti = d_tinf + b * (size_t)E;
    if ((inf && inf[b]) || gen_is_identity<F>(gens + b * 2 * A)) {
      HIP_TRY(hipMemsetAsync(t, 0, (size_t)E * 2 * F::WORDS * 4, s), 10);
      HIP_TRY(hipMemsetAsync(ti, 1, E, s), 10);
      continue;
    }
    ArkWords<2 * A> g;
    memcpy(g.v, gens + b * 2 * A, sizeof g.v);
    hipLaunchKernelGGL((k_fbm_bases<F>), dim3((W + 63) / 64), dim3(64), 0, s, g, bases, binf, W, c);
    hipLaunchKernelGGL((k_fbm_table<F>), dim3((E + 63) / 64), dim3(64), 0, s, bases, binf, t, ti, H, E);
    HIP_TRY(hipGetLastError(), 10);
  }
  HIP_TRY(hipStreamSynchronize(s), 10);
  return 0;
}

template int fixed_base_tables<Fp<P761>>(const uint64_t*, const uint8_t*, size_t, int, int, uint32_t*, uint8_t*, hipStream_t);
template int fixed_base_tables<Fp<P377>>(const uint64_t*, const uint8_t*, size_t, int, int, uint32_t*, uint8_t*, hipStream_t);

// ---- Groth16 parameter generation (include/celo_bls_amd.h groth16_setup_*).  curve 0 = BW6-761 (FB1 = FB2 = Fbm761), 1 = BLS12-377.
// dev_in = 0: qa / qb / qc are host pointers; 1: device pointers, complete before the call (groth16_setup_r1cs).
template <class FB1, class FB2, class FR>
static int setup_run(int curve, int dev_in, const uint64_t* qa, const uint64_t* qb, const uint64_t* qc, size_t n_vars, size_t n_inputs, const uint64_t* zt,
                     const uint64_t* tau, size_t n_h, const uint64_t* toxic, const uint64_t* g1_xy, const uint64_t* g2_xy, int window_bits, uint64_t* out_vk,
                     uint64_t* out_rows, ProvingKey** out_key) {
  constexpr int N = FR::ARK64, R1 = 2 * FB1::A, R2 = 2 * FB2::A;
  if (out_key) *out_key = nullptr;
  if (int rc0 = api_enter()) return rc0;
  if (!out_vk && !out_rows && !out_key) return 2;
  if (n_inputs == 0 || n_inputs > n_vars || !qa || !qb || !qc || !zt || !toxic || !g1_xy || !g2_xy || (n_h && !tau)) return 2;
  const size_t n1 = 3 + n_inputs + 2 * n_vars + n_h + (n_vars - n_inputs), n2 = 3 + n_vars;
  if (n1 > 0x7fffffffu) return 2;
  if (gen_is_identity<typename FB1::Fc>(g1_xy) || gen_is_identity<typename FB2::Fc>(g2_xy)) return 2;
  const FR alpha = FR::norm(FR::from_ark(toxic)), beta = FR::norm(FR::from_ark(toxic + N)), gamma = FR::norm(FR::from_ark(toxic + 2 * N)),
           delta = FR::norm(FR::from_ark(toxic + 3 * N));
  if (gamma.is_zero_mod_p() || delta.is_zero_mod_p()) return 2;
  const FR ginv = FR::norm(FR::inv(gamma)), dinv = FR::norm(FR::inv(delta));
  const FR zt_dinv = FR::norm(FR::mul(FR::from_ark(zt), dinv)), tau_d = n_h ? FR::norm(FR::from_ark(tau)) : FR::zero();
  uint64_t head1[3 * N], head2[3 * N];
  setup_canon<FR>(toxic, head1); setup_canon<FR>(toxic + N, head1 + N); setup_canon<FR>(toxic + 3 * N, head1 + 2 * N);
  setup_canon<FR>(toxic + N, head2); setup_canon<FR>(toxic + 2 * N, head2 + N); setup_canon<FR>(toxic + 3 * N, head2 + 2 * N);
  std::lock_guard<std::mutex> lk(setup_mu);
  TimedCall call(g_setup_last, 6);       // (declared in front of the call's resources: their release is inside the wall time)
  CallScope cs;
  HIP_TRY(cs.open(0, nullptr), 10);
  const hipStream_t s = cs.stream();
  EvLog log(s);
  const size_t qb_bytes = n_vars * N * 8;
  uint64_t *d_s1, *d_s2, *d_r1, *d_r2;
  const uint64_t *d_qa = qa, *d_qb = qb, *d_qc = qc;
  uint8_t *d_i1, *d_i2;
  HIP_TRY(cs.alloc(&d_s1, n1 * N * 8), 10);
  HIP_TRY(cs.alloc(&d_s2, n2 * N * 8), 10);
  HIP_TRY(cs.alloc(&d_r1, n1 * R1 * 8), 10);
  HIP_TRY(cs.alloc(&d_r2, n2 * R2 * 8), 10);
  HIP_TRY(cs.alloc(&d_i1, n1), 10);
  HIP_TRY(cs.alloc(&d_i2, n2), 10);
  if (!dev_in) {
    uint64_t* d_q;
    HIP_TRY(cs.alloc(&d_q, 3 * qb_bytes), 10);
    HIP_TRY(hipMemcpyAsync(d_q, qa, qb_bytes, hipMemcpyHostToDevice, s), 10);
    HIP_TRY(hipMemcpyAsync(d_q + n_vars * N, qb, qb_bytes, hipMemcpyHostToDevice, s), 10);
    HIP_TRY(hipMemcpyAsync(d_q + 2 * n_vars * N, qc, qb_bytes, hipMemcpyHostToDevice, s), 10);
    d_qa = d_q; d_qb = d_q + n_vars * N; d_qc = d_q + 2 * n_vars * N;
  }
  HIP_TRY(hipMemcpyAsync(d_s1, head1, sizeof head1, hipMemcpyHostToDevice, s), 10);
  HIP_TRY(hipMemcpyAsync(d_s2, head2, sizeof head2, hipMemcpyHostToDevice, s), 10);
  hipEvent_t e0 = log.open();
  hipLaunchKernelGGL((k_setup_fr<FR>), dim3((unsigned)((n_vars + 255) / 256)), dim3(256), 0, s, d_qa, d_qb, d_qc, (uint32_t)n_vars, (uint32_t)n_inputs, alpha, beta, ginv, dinv, d_s1, d_s2, (uint32_t)n_h);
  if (n_h) {
    const size_t blocks = (n_h + SETUP_H_BLOCK - 1) / SETUP_H_BLOCK;
    hipLaunchKernelGGL((k_setup_h<FR>), dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, s, zt_dinv, tau_d, (uint32_t)n_h,
                       d_s1 + (3 + n_inputs + 2 * n_vars) * N);
  }
  log.close(1, e0);
  HIP_TRY(hipGetLastError(), 10);
  {
    FB1 t1;
    if (int rcb = t1.build(g1_xy, s, &log)) return rcb;
    if (int rcr = t1.rows(d_s1, n1, d_r1, d_i1, 1, s, &log, 2)) return rcr;
  }
  {
    FB2 t2;
    if (int rcb = t2.build(g2_xy, s, &log)) return rcb;
    if (int rcr = t2.rows(d_s2, n2, d_r2, d_i2, 1, s, &log, 3)) return rcr;
  }
  const size_t r_abc = 3, r_a = r_abc + n_inputs, r_h = r_a + 2 * n_vars, r_l = r_h + n_h;
  if (out_vk) {
    uint64_t* o = out_vk;
    HIP_TRY(hipMemcpyAsync(o, d_r1, R1 * 8, hipMemcpyDeviceToHost, s), 10); o += R1;
    HIP_TRY(hipMemcpyAsync(o, d_r2, 3 * R2 * 8, hipMemcpyDeviceToHost, s), 10); o += 3 * R2;
    HIP_TRY(hipMemcpyAsync(o, d_r1 + r_abc * R1, n_inputs * R1 * 8, hipMemcpyDeviceToHost, s), 10);
  }
  if (out_rows) {
    uint64_t* o = out_rows;
    HIP_TRY(hipMemcpyAsync(o, d_r1 + R1, 2 * R1 * 8, hipMemcpyDeviceToHost, s), 10); o += 2 * R1;
    HIP_TRY(hipMemcpyAsync(o, d_r1 + r_a * R1, 2 * n_vars * R1 * 8, hipMemcpyDeviceToHost, s), 10); o += 2 * n_vars * R1;
    HIP_TRY(hipMemcpyAsync(o, d_r2 + 3 * R2, n_vars * R2 * 8, hipMemcpyDeviceToHost, s), 10); o += n_vars * R2;
    HIP_TRY(hipMemcpyAsync(o, d_r1 + r_h * R1, (n_h + n_vars - n_inputs) * R1 * 8, hipMemcpyDeviceToHost, s), 10);
  }
  HIP_TRY(hipStreamSynchronize(s), 10);
  log.sum(call.t.ms);
  if (!out_key) return 0;
  // the four key elements the composition keeps on the host (query[0] of a and b_g2, alpha_g1, beta_g2): four rows, not a query
  uint64_t a0[R1], b0[R2], al[R1], be[R2];
  HIP_TRY(hipMemcpy(a0, d_r1 + r_a * R1, sizeof a0, hipMemcpyDeviceToHost), 10);
  HIP_TRY(hipMemcpy(b0, d_r2 + 3 * R2, sizeof b0, hipMemcpyDeviceToHost), 10);
  HIP_TRY(hipMemcpy(al, d_r1, sizeof al, hipMemcpyDeviceToHost), 10);
  HIP_TRY(hipMemcpy(be, d_r2, sizeof be, hipMemcpyDeviceToHost), 10);
  const WallMs wall_key;
  // (sets *out_key only on success; the key is the call's last step, so nothing after it can fail)
  const int rck = groth16_key_load_dev(curve, d_r1 + r_a * R1, d_i1 + r_a, n_vars, d_r2 + 3 * R2, d_i2 + 3, n_vars, d_r1 + r_h * R1, d_i1 + r_h, n_h,
                                       d_r1 + r_l * R1, d_i1 + r_l, n_vars - n_inputs, a0, b0, al, be, window_bits, out_key);
  call.t.ms[5] = wall_key.ms();
  return rck;
}

int groth16_setup(int curve, const uint64_t* qa, const uint64_t* qb, const uint64_t* qc, size_t n_vars, size_t n_inputs, const uint64_t* zt, const uint64_t* tau,
                  size_t n_h, const uint64_t* toxic, const uint64_t* g1_xy, const uint64_t* g2_xy, int window_bits, uint64_t* out_vk, uint64_t* out_rows,
                  ProvingKey** out_key) {
  if (curve == 0)
    return setup_run<Fbm761, Fbm761, FrBw6>(0, 0, qa, qb, qc, n_vars, n_inputs, zt, tau, n_h, toxic, g1_xy, g2_xy, window_bits, out_vk, out_rows, out_key);
  return setup_run<FbmG1_377, FbmG2_377, FrBls>(1, 0, qa, qb, qc, n_vars, n_inputs, zt, tau, n_h, toxic, g1_xy, g2_xy, window_bits, out_vk, out_rows, out_key);
}

// ---- matrices + toxic waste -> parameters (groth16_setup_r1cs_*): the QAP at tau on the device (unit_r1cs.hip), then setup_run on the three
// vectors where they lie; n_h = 2^log_n - 1
int groth16_setup_r1cs(int curve, const R1cs* r, unsigned log_n, const uint64_t* omega, const uint64_t* tau, const uint64_t* toxic, const uint64_t* g1_xy,
                       const uint64_t* g2_xy, int window_bits, uint64_t* out_vk, uint64_t* out_rows, ProvingKey** out_key) {
  if (out_key) *out_key = nullptr;
  if (int rc0 = api_enter()) return rc0;
  if (!r || !omega || !tau || log_n > 28) return 2;
  int r_curve, device;
  size_t m, n_vars, n_inputs;
  r1cs_shape(r, &r_curve, &device, &m, &n_vars, &n_inputs);
  if (r_curve != curve) return 2;
  if (device != api_device()) return 101;
  const WallMs wall;
  const int N = curve ? 4 : 6;
  const int rc = [&]() -> int {
    CallScope cs(nullptr);
    HIP_TRY(cs.create_stream(), 10);
    uint64_t *d_q, zt[6];
    HIP_TRY(cs.alloc(&d_q, 3 * n_vars * N * 8), 10);
    uint64_t *qa = d_q, *qb = d_q + n_vars * N, *qc = d_q + 2 * n_vars * N;
    if (int rcq = r1cs_qap_at_tau(r, log_n, omega, tau, qa, qb, qc, zt, 1, cs.stream())) return rcq;
    const size_t n_h = (size_t(1) << log_n) - 1;
    if (curve == 0)
      return setup_run<Fbm761, Fbm761, FrBw6>(0, 1, qa, qb, qc, n_vars, n_inputs, zt, tau, n_h, toxic, g1_xy, g2_xy, window_bits, out_vk, out_rows, out_key);
    return setup_run<FbmG1_377, FbmG2_377, FrBls>(1, 1, qa, qb, qc, n_vars, n_inputs, zt, tau, n_h, toxic, g1_xy, g2_xy, window_bits, out_vk, out_rows, out_key);
  }();
  r1cs_note_ms(5, wall.ms());
  return rc;
}

}  // namespace celo
