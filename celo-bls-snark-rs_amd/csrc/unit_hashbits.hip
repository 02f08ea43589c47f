// Translation unit: the HashToBits circuit of the hash-helper proof on the device (hashbits.h) - from the CRH rows of a chain of epochs to the
// full assignment, the public inputs and, with a loaded key and circuit, the proof of generate_hash_helper
// (crates/epoch-snark/src/api/prover.rs:85-118).  DESIGN.md section 6m.
//   k_hashbits_trace    one lane per (epoch, compression): Blake2s on words, every intermediate the rows name stored as u32
//   k_hashbits_expand   one lane per 16 bytes of the assignment: descriptor -> trace word -> bit -> the Montgomery 0 or 1
//   k_hashbits_pack     one lane per instance variable: its 252 bits gathered from the trace
#include "hashbits.h"
#include <hip/hip_runtime.h>
#include <mutex>
#include <vector>
#include "runtime.h"
#include "units.h"

namespace celo {

constexpr uint32_t HB_TRACE_BLOCK = 64, HB_EXPAND_BLOCK = 256, HB_PACK_BLOCK = 64;

// the last groth16_hash_helper_prove or hash_to_bits_assignment call in ms: [0] trace, [1] expand, [2] pack (kernel times), and for the former
// [3] the proof (wall), [4] the call (wall)
static Last<CallTimes> g_hh_last;
void hash_helper_last(float ms[8]) { const CallTimes t = g_hh_last.read(); for (int i = 0; i < 8; i++) ms[i] = t.ms[i]; }

__global__ void __launch_bounds__(HB_TRACE_BLOCK) k_hashbits_trace(const uint8_t* __restrict__ rows48, uint32_t n_epochs, int bit_order, uint32_t* __restrict__ trace) {
  const uint32_t lane = blockIdx.x * HB_TRACE_BLOCK + threadIdx.x, e = lane >> 1;
  if (e >= n_epochs) return;
  hb_trace_lane(rows48 + (size_t)e * HB_ROW_BYTES, bit_order, lane & 1u, trace + (size_t)e * HB_TRACE_WORDS);
}
// Lane t writes bytes [16 t, 16 t + 16) of z: limbs 2 (t & 1), 2 (t & 1) + 1 of variable t / 2, so a wave's store is one KiB in a row.  The
// instance rows [1, n_inputs) are k_hashbits_pack's.  Neighbouring lanes read the same descriptor and, 32 variables long, the same trace word.
__global__ void __launch_bounds__(HB_EXPAND_BLOCK) k_hashbits_expand(const uint32_t* __restrict__ desc, const uint32_t* __restrict__ trace, uint32_t stride, uint32_t n_inputs,
                                                                     uint64_t n_halves, ulonglong2* __restrict__ z) {
  const uint64_t t = (uint64_t)blockIdx.x * HB_EXPAND_BLOCK + threadIdx.x;
  if (t >= n_halves) return;
  const uint32_t i = (uint32_t)(t >> 1), half = (uint32_t)(t & 1);
  if (i != 0 && i < n_inputs) return;
  const bool bit = i == 0 || hb_var_bit(desc, trace, stride, n_inputs, i);
  ulonglong2 v;
  v.x = bit ? (half ? HbFr::R[2] : HbFr::R[0]) : 0;
  v.y = bit ? (half ? HbFr::R[3] : HbFr::R[1]) : 0;
  z[t] = v;
}
// instance variable 1 + c of proof p (the trace of proof p starts n_epochs epochs after that of p - 1): Montgomery limbs into z_rows (row c of
// the proof's n_chunks rows) and / or canonical limbs into canonical, either may be NULL
__global__ void __launch_bounds__(HB_PACK_BLOCK) k_hashbits_pack(const uint32_t* __restrict__ trace, uint32_t n_epochs, uint32_t n_chunks, uint32_t n_proofs,
                                                                 uint64_t* __restrict__ z_rows, uint64_t* __restrict__ canonical) {
  const uint64_t t = (uint64_t)blockIdx.x * HB_PACK_BLOCK + threadIdx.x;
  if (t >= (uint64_t)n_chunks * n_proofs) return;
  const uint32_t p = (uint32_t)(t / n_chunks), c = (uint32_t)(t - (uint64_t)p * n_chunks);
  uint64_t v[4], w[4];
  hb_pack_chunk(trace + (size_t)p * n_epochs * HB_TRACE_WORDS, n_epochs, c, v);
  if (canonical) for (int j = 0; j < 4; j++) canonical[t * 4 + j] = v[j];
  if (z_rows) {
    hb_to_mont(v, w);
    for (int j = 0; j < 4; j++) z_rows[t * 4 + j] = w[j];
  }
}

// ---- host-only entries
int hashbits_sizes(size_t m, uint64_t out[8]) {
  HbSizes s;
  if (!out) return 2;
  if (int rc = hb_sizes(m, &s)) return rc;
  const uint64_t v[8] = {s.n_constraints, s.n_vars, s.n_inputs, s.nnz[0], s.nnz[1], s.nnz[2], s.log_n, s.stride};
  memcpy(out, v, sizeof v);
  return 0;
}
int hashbits_write_csr(size_t m, uint64_t* const row_ptr[3], uint32_t* const col[3], uint64_t* const val[3]) { return hb_write_csr(m, row_ptr, col, val); }
int hashbits_assignment_host(const uint8_t* rows48, size_t m, int bit_order, uint64_t* z) { return hb_assignment_host(rows48, m, bit_order, z); }

int hashbits_r1cs_load(size_t m, R1cs** out) {
  HbSizes s;
  if (!out) return 2;
  *out = nullptr;
  if (int rc = hb_sizes(m, &s)) return rc;
  std::vector<uint64_t> rp[3], val[3];
  std::vector<uint32_t> col[3];
  uint64_t *rpp[3], *valp[3];
  uint32_t* colp[3];
  for (int k = 0; k < 3; k++) {
    rp[k].resize(s.n_constraints + 1); col[k].resize(s.nnz[k] + 1); val[k].resize(4 * s.nnz[k] + 4);
    rpp[k] = rp[k].data(); colp[k] = col[k].data(); valp[k] = val[k].data();
  }
  if (int rc = hb_write_csr(m, rpp, colp, valp)) return rc;
  return r1cs_load(1, s.n_constraints, s.n_vars, s.n_inputs, rpp, colp, valp, s.nnz, out, nullptr);
}

// ---- the per-device copy of the descriptors, made at the first call and kept for the process
static int device_desc(const uint32_t** out) {
  static std::mutex mu;
  static uint32_t* d_desc[MAX_DEVICES] = {};
  const int dev = api_device();
  std::lock_guard<std::mutex> lk(mu);
  if (!d_desc[dev]) {
    const HbTemplate& T = hb_template();
    uint32_t* p = nullptr;
    HIP_TRY(hipMalloc((void**)&p, T.desc.size() * 4), 10);
    if (hipMemcpy(p, T.desc.data(), T.desc.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(p); return 10; }
    d_desc[dev] = p;
  }
  *out = d_desc[dev];
  return 0;
}

// the three kernels on cs.stream(): rows (device) -> trace -> z (device, may be NULL: no expansion) and the canonical inputs (device, may be
// NULL).  n_proofs > 1 only without z.
static int enqueue(CallScope& cs, EvLog& log, const uint8_t* d_rows, size_t n_proofs, size_t m, int bit_order, const HbSizes& s, uint64_t* d_z, uint64_t* d_canonical) {
  const hipStream_t st = cs.stream();
  const size_t epochs = n_proofs * m;
  uint32_t* d_trace;
  HIP_TRY(cs.alloc(&d_trace, epochs * HB_TRACE_WORDS * 4), 10);
  hipEvent_t e0 = log.open();
  hipLaunchKernelGGL(k_hashbits_trace, dim3((unsigned)((2 * epochs + HB_TRACE_BLOCK - 1) / HB_TRACE_BLOCK)), dim3(HB_TRACE_BLOCK), 0, st, d_rows, (uint32_t)epochs, bit_order,
                     d_trace);
  log.close(0, e0);
  if (d_z) {
    const uint32_t* d_desc;
    if (int rc = device_desc(&d_desc)) return rc;
    const uint64_t n_halves = 2 * s.n_vars;
    e0 = log.open();
    hipLaunchKernelGGL(k_hashbits_expand, dim3((unsigned)((n_halves + HB_EXPAND_BLOCK - 1) / HB_EXPAND_BLOCK)), dim3(HB_EXPAND_BLOCK), 0, st, d_desc, d_trace,
                       (uint32_t)s.stride, (uint32_t)s.n_inputs, n_halves, (ulonglong2*)d_z);
    log.close(1, e0);
  }
  const uint64_t n_chunks = s.n_inputs - 1, lanes = n_chunks * n_proofs;
  e0 = log.open();
  hipLaunchKernelGGL(k_hashbits_pack, dim3((unsigned)((lanes + HB_PACK_BLOCK - 1) / HB_PACK_BLOCK)), dim3(HB_PACK_BLOCK), 0, st, d_trace, (uint32_t)m, (uint32_t)n_chunks,
                     (uint32_t)n_proofs, d_z ? d_z + 4 : nullptr, d_canonical);
  log.close(2, e0);
  HIP_TRY(hipGetLastError(), 10);
  return 0;
}

// rows48 and z: host (dev = 0) or device pointers (dev = 1, the work on the caller's stream); complete on return in both forms
int hashbits_assignment(const uint8_t* rows48, size_t m, int bit_order, uint64_t* z, int dev, void* stream) {
  HbSizes s;
  if (!rows48 || !z || bit_order < 0 || bit_order > 1) return 2;
  if (int rc = hb_sizes(m, &s)) return rc;
  if (int rc0 = api_enter()) return rc0;
  CallScope cs;
  HIP_TRY(cs.open(dev, stream), 10);
  uint8_t* d_rows;
  uint64_t* d_z;
  HIP_TRY(cs.in(&d_rows, rows48, m * HB_ROW_BYTES, dev), 10);
  HIP_TRY(cs.out(&d_z, z, s.n_vars * 32, dev), 10);
  EvLog log(cs.stream());
  if (int rc = enqueue(cs, log, d_rows, 1, m, bit_order, s, d_z, nullptr)) return rc;
  HIP_TRY(cs.copy_back(), 10);
  HIP_TRY(hipStreamSynchronize(cs.stream()), 10);
  CallTimes t;
  log.sum(t.ms);
  g_hh_last.note(t);
  return 0;
}
// out: n_proofs x (n_inputs - 1) x 4 canonical limbs, the layout groth16_verify_batch_bls12_377 takes; proof p reads rows [p m, (p + 1) m)
int hashbits_public_inputs(const uint8_t* rows48, size_t n_proofs, size_t m, int bit_order, uint64_t* out, int dev, void* stream) {
  HbSizes s;
  if (!rows48 || !out || bit_order < 0 || bit_order > 1 || n_proofs == 0 || n_proofs > (size_t(1) << 24)) return 2;
  if (int rc = hb_sizes(m, &s)) return rc;
  if (n_proofs * m > (size_t(1) << 24)) return 2;
  if (int rc0 = api_enter()) return rc0;
  CallScope cs;
  HIP_TRY(cs.open(dev, stream), 10);
  uint8_t* d_rows;
  uint64_t* d_out;
  HIP_TRY(cs.in(&d_rows, rows48, n_proofs * m * HB_ROW_BYTES, dev), 10);
  HIP_TRY(cs.out(&d_out, out, n_proofs * (s.n_inputs - 1) * 32, dev), 10);
  EvLog log(cs.stream());
  if (int rc = enqueue(cs, log, d_rows, n_proofs, m, bit_order, s, nullptr, d_out)) return rc;
  HIP_TRY(cs.copy_back(), 10);
  HIP_TRY(hipStreamSynchronize(cs.stream()), 10);
  return 0;
}

// generate_hash_helper in one call: the rows go up (48 bytes an epoch), the assignment is made on the device and proved from there, the
// canonical instance rows (n_inputs - 1 of them) come back beside A, B, C (Jacobian, as groth16_prove_r1cs_with_key returns them)
int hash_helper_prove(const ProvingKey* k, const R1cs* r, const uint8_t* rows48, size_t m, int bit_order, unsigned log_n, const uint64_t* omega, const uint64_t* omega_inv,
                      const uint64_t* coset, const uint64_t* coset_inv, const uint64_t* n_inv, const uint64_t* z_inv, uint64_t* out_a, uint64_t* out_b, uint64_t* out_c,
                      uint64_t* out_inputs) {
  HbSizes s;
  if (!k || !r || !rows48 || bit_order < 0 || bit_order > 1 || !omega || !omega_inv || !coset || !coset_inv || !n_inv || !z_inv || !out_a || !out_b || !out_c || !out_inputs)
    return 2;
  if (int rc = hb_sizes(m, &s)) return rc;
  if (int rc0 = api_enter()) return rc0;
  int curve, device, kcurve;
  size_t rm, n_vars, n_inputs, krows[4];
  r1cs_shape(r, &curve, &device, &rm, &n_vars, &n_inputs);
  groth16_key_shape(k, &kcurve, krows);
  if (curve != 1 || kcurve != 1 || rm != s.n_constraints || n_vars != s.n_vars || n_inputs != s.n_inputs) return 2;
  if (log_n > 28 || log_n < s.log_n) return 2;
  if (krows[0] != n_vars || krows[1] != n_vars || krows[2] != n_vars - n_inputs || krows[3] != (size_t(1) << log_n) - 1) return 2;
  if (device != api_device()) return 101;
  CallTimes t;
  const WallMs wall;
  {
    CallScope cs;
    HIP_TRY(cs.open(0, nullptr), 10);
    uint8_t* d_rows;
    uint64_t *d_z, *d_in;
    HIP_TRY(cs.in(&d_rows, rows48, m * HB_ROW_BYTES, 0), 10);
    HIP_TRY(cs.alloc(&d_z, s.n_vars * 32), 10);
    HIP_TRY(cs.out(&d_in, out_inputs, (s.n_inputs - 1) * 32, 0), 10);
    EvLog log(cs.stream());
    if (int rc = enqueue(cs, log, d_rows, 1, m, bit_order, s, d_z, d_in)) return rc;
    HIP_TRY(cs.copy_back(), 10);
    HIP_TRY(hipStreamSynchronize(cs.stream()), 10);
    log.sum(t.ms);
    const WallMs prove;
    if (int rc = groth16_prove_r1cs(k, r, d_z, 2, log_n, omega, omega_inv, coset, coset_inv, n_inv, z_inv, out_a, out_b, out_c)) return rc;
    t.ms[3] = prove.ms();
  }
  t.ms[4] = wall.ms();
  g_hh_last.note(t);
  return 0;
}

// The verifier's side of generate_hash_helper in one call: n_proofs proofs (192 bytes each) of chains of m epochs, proof p over rows
// [p m, (p + 1) m).  The rows go up, the canonical inputs are made on the device (hashbits_public_inputs' kernels) and the Groth16 verifier
// reads them where they lie.  2: a NULL pointer, a size the size query refuses, or a key whose input count is not n_inputs(m) - 1 (a handle
// that is not a live BLS12-377 one among them) - all before any device use; else the verifier's codes.
int hash_helper_verify(const VerifyingKey* vk, const uint8_t* rows48, size_t n_proofs, size_t m, int bit_order, const uint8_t* proofs, int mode, const uint32_t* key,
                       uint8_t* out_ok) {
  HbSizes s;
  if (!vk || !rows48 || !proofs || !out_ok || bit_order < 0 || bit_order > 1 || (mode != 0 && mode != 1)) return 2;
  if (n_proofs == 0 || n_proofs > (size_t(1) << 24)) return 2;
  if (int rc = hb_sizes(m, &s)) return rc;
  if (n_proofs * m > (size_t(1) << 24)) return 2;
  if (groth16_vk_inputs(vk, 1) != (int)(s.n_inputs - 1)) return 2;
  if (int rc0 = api_enter()) return rc0;
  CallScope cs;
  HIP_TRY(cs.open(0, nullptr), 10);
  uint8_t* d_rows;
  uint64_t* d_in;
  HIP_TRY(cs.in(&d_rows, rows48, n_proofs * m * HB_ROW_BYTES, 0), 10);
  HIP_TRY(cs.alloc(&d_in, n_proofs * (s.n_inputs - 1) * 32), 10);
  EvLog log(cs.stream());
  if (int rc = enqueue(cs, log, d_rows, n_proofs, m, bit_order, s, nullptr, d_in)) return rc;
  HIP_TRY(hipStreamSynchronize(cs.stream()), 10);          // the verifier works on a stream of its own
  return G16Api<G16Bls>::verify_staged(vk, proofs, d_in, nullptr, n_proofs, mode, key, out_ok, nullptr);
}

}  // namespace celo
