// Translation unit: batched variable-base scalar multiplication out[i] = [k_i] P_i (var_base.h) for the four groups, the subgroup (GLV)
// form for BLS12-377 G1, and batched signing on top of it: hash to G1 (unit_hash.hip, unchanged) -> [sk] H on the subgroup path ->
// compressed signatures (unit_wire_encode.hip).
// DESIGN.md section 6i.
#include "var_base.h"
#include "normalize.h"
#include <hip/hip_runtime.h>
#include <cstring>
#include <mutex>
#include <vector>
#include "runtime.h"
#include "units.h"

namespace celo {

// calls from several host threads are serialised per process (bulk calls: one fills the GPU).  Guards the settings g_vb_c and g_vb_chunk
static std::mutex vb_mu;
static int g_vb_c = 0;                       // 0 = the default of the group (vb_default_c), else VB_MIN_C .. VB_MAX_C (celo_amd_scalar_mul_set_window)
static uint32_t g_vb_chunk = 0;              // rows per chunk; 0 = the default (vb_default_chunk)
// The default window: same-run A/B over every accepted width on 2^16 rows (profiles/bench_scalar_mul.json), kernel time of the whole
// call: BLS12-377 G1 c = 3 3.70 ms, 4 3.64, 5 6.48 (subgroup entry 2.66 / 2.56 / 4.73); G2 c = 2 13.8, 3 12.5, 4 20.4; BW6-761 c = 2 24.0, 3 21.4, 4 36.6
template <class F> constexpr int vb_default_c() { return sizeof(F) <= 64 ? 4 : 3; }
static constexpr size_t VB_WORKSPACE = size_t(1) << 28;   // the default chunk keeps table + chain below this
static constexpr int VB_BLOCK = 64;          // one wave per workgroup: the kernels are register-heavy and the batches often small
// the last call's timings in ms: [0] table build, [1] ladder, [2] normalisation, [3] whole call (wall); published on every exit of a call that has entered
static Last<CallTimes> g_vb_last;

// lane i -> the table of P_i (var_base.h vb_build_table).  xy: rows of 2 A arkworks limbs; inf: flags or null.
template <class F>
__global__ void __launch_bounds__(VB_BLOCK) k_vb_table(const uint64_t* __restrict__ xy, const uint8_t* __restrict__ inf, uint32_t n, uint32_t H, uint4* __restrict__ chain,
                                                       uint4* __restrict__ table, uint8_t* __restrict__ tinf, uint32_t stride) {
  constexpr int A = F::ARK64;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Affine<F> p = {F::norm(F::from_ark(xy + (size_t)i * 2 * A)), F::norm(F::from_ark(xy + (size_t)i * 2 * A + A))};
  vb_build_table<F>(p, inf && inf[i], H, chain, table, tinf, stride, i);
}
// lane i -> [k_i] P_i in XYZZ (device form, 4 FW words per row).  sc_stride: N64, or 0 for one scalar shared by every row (every lane then
// reads scalars[0]: the recoding is uniform across the wave).  GLV: the subgroup ladder (BLS12-377 G1).
template <class F, int N64, int BITS, bool GLV>
__global__ void __launch_bounds__(VB_BLOCK) k_vb_ladder(const uint64_t* __restrict__ sc, uint32_t sc_stride, uint32_t n, const uint4* __restrict__ table,
                                                        const uint8_t* __restrict__ tinf, uint32_t stride, int c, uint32_t* __restrict__ xyzz) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t s[N64];
#pragma unroll
  for (int k = 0; k < N64; k++) s[k] = sc[(size_t)i * sc_stride + k];
  Xyzz<F> a;
  if constexpr (GLV) a = vb_ladder_glv<F>(s, c, table, tinf, stride, i);
  else a = vb_ladder<F, N64>(s, BITS, c, table, tinf, stride, i);
  uint32_t* o = xyzz + (size_t)i * 4 * F::WORDS;
  a.X.store(o); a.Y.store(o + F::WORDS); a.ZZ.store(o + 2 * F::WORDS); a.ZZZ.store(o + 3 * F::WORDS);
}

// ---- one group: F the coordinate field, N64 u64 per scalar, BITS scalar bits
template <class F, int N64, int BITS> struct Vbm {
  static constexpr int A = F::ARK64, FW = F::WORDS;
  static size_t lane_bytes(uint32_t H) { return (size_t)H * (6 * FW * 4 + 1); }
  static uint32_t default_chunk(uint32_t H) {
    size_t rows = VB_WORKSPACE / lane_bytes(H);
    if (rows > (size_t(1) << 16)) rows = size_t(1) << 16;
    rows &= ~size_t(VB_BLOCK - 1);
    return (uint32_t)(rows ? rows : VB_BLOCK);
  }
  // n rows, everything on the device, enqueued on s in chunks that bound the workspace; returns after the stream has drained
  template <bool GLV>
  static int run(const uint64_t* d_xy, const uint8_t* d_inf, const uint64_t* d_sc, size_t n_sc, size_t n, uint64_t* d_out, uint8_t* d_oinf, hipStream_t s, EvLog* log) {
    if (n == 0) return 0;
    const int c = g_vb_c ? g_vb_c : vb_default_c<F>();
    const uint32_t H = 1u << (c - 1);
    const size_t chunk = g_vb_chunk ? g_vb_chunk : default_chunk(H);
    const size_t m = n < chunk ? n : chunk;
    CallScope cs(s);
    uint4 *chain, *table;
    uint8_t* tinf;
    uint32_t* tmp;
    HIP_TRY(cs.alloc(&chain, m * H * FW * sizeof(uint4)), 10);
    HIP_TRY(cs.alloc(&table, m * H * (2 * FW / 4) * sizeof(uint4)), 10);
    HIP_TRY(cs.alloc(&tinf, m * H), 10);
    HIP_TRY(cs.alloc(&tmp, m * 4 * FW * 4), 10);
    for (size_t lo = 0; lo < n; lo += chunk) {
      const uint32_t k = (uint32_t)(n - lo < chunk ? n - lo : chunk);
      const dim3 grid((k + VB_BLOCK - 1) / VB_BLOCK), block(VB_BLOCK);
      hipEvent_t e0 = log->open();
      hipLaunchKernelGGL((k_vb_table<F>), grid, block, 0, s, d_xy + lo * 2 * A, d_inf ? d_inf + lo : nullptr, k, H, chain, table, tinf, (uint32_t)m);
      log->close(0, e0);
      e0 = log->open();
      hipLaunchKernelGGL((k_vb_ladder<F, N64, BITS, GLV>), grid, block, 0, s, d_sc + (n_sc == 1 ? 0 : lo * N64), n_sc == 1 ? 0u : (uint32_t)N64, k, table, tinf, (uint32_t)m, c,
                         tmp);
      log->close(1, e0);
      e0 = log->open();
      normalize_xyzz<F, false>(tmp, d_out + lo * 2 * A, d_oinf + lo, k, 0, s);
      log->close(2, e0);
      HIP_TRY(hipGetLastError(), 10);
    }
    HIP_TRY(hipStreamSynchronize(s), 10);
    return 0;
  }
};
typedef Vbm<Fp<P377>, 4, 253> VbmG1_377;
typedef Vbm<Fp2<P377>, 4, 253> VbmG2_377;
typedef Vbm<Fp<P761>, 6, 377> Vbm761;

template <int N64> static const uint64_t* vb_order() {
  if constexpr (N64 == 4) return P253::P64;
  else return P377::P64;
}

// Host or device pointers (runtime.h, the call frame).  Refused arguments: 2, nothing written.
template <class VB, int N64, bool GLV>
static int vb_mul(const void* xy, const void* inf, const void* scalars, size_t n_sc, size_t n, void* out_xy, void* out_inf, int dev, void* stream_) {
  constexpr int RW = 2 * VB::A;
  if (int rc0 = api_enter()) return rc0;
  if (n == 0) return 0;
  if (!xy || !scalars || !out_xy || !out_inf || (n_sc != 1 && n_sc != n) || n > 0x7fffffffu) return 2;
  if (!dev) {
    const uint64_t* sc = (const uint64_t*)scalars;
    for (size_t i = 0; i < n_sc; i++) if (!fb_below<N64>(sc + i * N64, vb_order<N64>())) return 2;
  }
  std::lock_guard<std::mutex> lk(vb_mu);
  TimedCall call(g_vb_last, 3);
  CallScope cs;
  HIP_TRY(cs.open(dev, stream_), 10);
  EvLog log(cs.stream());
  uint64_t *d_xy, *d_sc, *d_out;
  uint8_t *d_inf, *d_oinf;
  if (dev) if (int rcs = scalars_below_order<N64>((const uint64_t*)scalars, n_sc, vb_order<N64>(), cs)) return rcs;
  HIP_TRY(cs.in(&d_xy, xy, n * RW * 8, dev), 10);
  HIP_TRY(cs.in(&d_sc, scalars, n_sc * N64 * 8, dev), 10);
  HIP_TRY(cs.in(&d_inf, inf, n, dev), 10);
  HIP_TRY(cs.out(&d_out, out_xy, n * RW * 8, dev), 10);
  HIP_TRY(cs.out(&d_oinf, out_inf, n, dev), 10);
  if (int rcr = VB::template run<GLV>(d_xy, d_inf, d_sc, n_sc, n, d_out, d_oinf, cs.stream(), &log)) return rcr;
  HIP_TRY(cs.copy_back(), 10);
  HIP_TRY(hipStreamSynchronize(cs.stream()), 10);
  log.sum(call.t.ms);
  return 0;
}

// group 0 / 1: BLS12-377 G1 / G2, 2: BW6-761 (both groups); subgroup: the GLV ladder (group 0 only)
int scalar_mul_batch(int group, int subgroup, const void* xy, const void* inf, const void* scalars, size_t n_scalars, size_t n, void* out_xy, void* out_inf, int dev,
                     void* stream) {
  switch (group) {
    case 0:
      if (subgroup) return vb_mul<VbmG1_377, 4, true>(xy, inf, scalars, n_scalars, n, out_xy, out_inf, dev, stream);
      return vb_mul<VbmG1_377, 4, false>(xy, inf, scalars, n_scalars, n, out_xy, out_inf, dev, stream);
    case 1: return subgroup ? 2 : vb_mul<VbmG2_377, 4, false>(xy, inf, scalars, n_scalars, n, out_xy, out_inf, dev, stream);
    case 2: return subgroup ? 2 : vb_mul<Vbm761, 6, false>(xy, inf, scalars, n_scalars, n, out_xy, out_inf, dev, stream);
    default: return 2;
  }
}
int scalar_mul_set_window(int c) {
  if (c != 0 && (c < VB_MIN_C || c > VB_MAX_C)) return 2;
  std::lock_guard<std::mutex> lk(vb_mu);
  g_vb_c = c;
  return 0;
}
int scalar_mul_set_chunk_rows(uint32_t rows) {
  if (rows > (1u << 24)) return 2;
  std::lock_guard<std::mutex> lk(vb_mu);
  g_vb_chunk = rows;
  return 0;
}
void scalar_mul_last_ms(float ms[4]) {
  const CallTimes t = g_vb_last.read();
  for (int i = 0; i < 4; i++) ms[i] = t.ms[i];
}

// ---- sign_batch_bls12_377: sig_i = [sk_i] H(msg_i), compressed.  The hash unit's run function hands its rows back on the host (96 B per
// message); they return to the device with the keys, the product and the encoding stay there.  A message without a counter (attempts 255)
// enters as the identity and leaves as 48 zero bytes.
int sign_batch_377(const uint64_t* sk, size_t n_sk, const uint8_t* domain, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* extras, const uint64_t* extra_off,
                   size_t n, int mode, uint8_t* out_sig48, uint8_t* attempts) {
  if (int rc0 = api_enter()) return rc0;
  if (n == 0) return 0;
  if (!sk || !domain || !msgs || !msg_off || !out_sig48 || !attempts || (n_sk != 1 && n_sk != n) || n > 0x7fffffffu) return 2;
  if (mode != 0 && mode != 2 && mode != 3) return 2;
  for (size_t i = 0; i < n_sk; i++) if (!fb_below<4>(sk + i * 4, P253::P64)) return 2;
  TimedCall call(g_vb_last, 3);
  std::vector<uint64_t> hxy(n * 12);
  std::vector<uint8_t> att(n), hinf(n);
  if (int rc = hash_to_g1_direct_run(domain, msgs, msg_off, extras, extra_off, n, hxy.data(), att.data(), mode)) return rc;
  for (size_t i = 0; i < n; i++) hinf[i] = att[i] == 255 ? 1 : 0;
  std::vector<uint8_t> sig(n * 48);
  std::lock_guard<std::mutex> lk(vb_mu);
  CallScope cs;
  HIP_TRY(cs.open(0, nullptr), 10);
  const hipStream_t s = cs.stream();
  EvLog log(s);
  uint64_t *d_xy, *d_sc, *d_out;
  uint8_t *d_inf, *d_oinf, *d_sig, *d_status;
  HIP_TRY(cs.in(&d_xy, hxy.data(), n * 96, 0), 10);
  HIP_TRY(cs.in(&d_sc, sk, n_sk * 32, 0), 10);
  HIP_TRY(cs.in(&d_inf, hinf.data(), n, 0), 10);
  HIP_TRY(cs.alloc(&d_out, n * 96), 10);
  HIP_TRY(cs.alloc(&d_oinf, n), 10);
  HIP_TRY(cs.out(&d_sig, sig.data(), n * 48, 0), 10);
  HIP_TRY(cs.alloc(&d_status, n), 10);
  if (int rcr = VbmG1_377::run<true>(d_xy, d_inf, d_sc, n_sk, n, d_out, d_oinf, s, &log)) return rcr;
  if (int rce = wire_encode(0, 1, d_out, d_oinf, n, d_sig, d_status, 1, s)) return rce;
  HIP_TRY(cs.copy_back(), 10);
  HIP_TRY(hipStreamSynchronize(s), 10);
  log.sum(call.t.ms);
  for (size_t i = 0; i < n; i++) {
    if (hinf[i]) memset(out_sig48 + i * 48, 0, 48);
    else memcpy(out_sig48 + i * 48, sig.data() + i * 48, 48);
  }
  memcpy(attempts, att.data(), n);
  return 0;
}

}  // namespace celo
