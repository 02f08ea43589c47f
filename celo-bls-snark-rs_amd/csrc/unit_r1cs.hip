// Translation unit: R1CS matrices on the device (r1cs.h) - the step of ark-groth16 0.1 between cs.to_matrices() and the entry points of
// unit_prover.hip / unit_setup.hip: R1CStoQAP::witness_map's constraint evaluation (the matrices with the assignment) and
// R1CStoQAP::instance_map_with_evaluation (their transposes with the Lagrange basis at tau).  DESIGN.md section 6g.
#include "r1cs.h"
#include <hip/hip_runtime.h>
#include <cstring>
#include <vector>
#include "runtime.h"
#include "units.h"

namespace celo {

typedef Fp<P377> FrBw6;          // the scalar field of BW6-761 (the base field of BLS12-377)
typedef Fp<P253> FrBls;          // the scalar field of BLS12-377

// the last call's timings in ms: [0] load (validation, transposition, binning, copies: host wall), [1] the rows kernels, [2] the Lagrange kernel,
// [3] the columns kernels, [4] groth16_prove_r1cs_with_key wall, [5] groth16_setup_r1cs_* wall
static Last<CallTimes> g_r1cs_last;
// every writer owns its slots: the calls of this unit [0] .. [3], the prover [4], the setup [5]
void r1cs_note_ms(int slot, float v) { g_r1cs_last.update([&](CallTimes& t) { t.ms[slot] = v; }); }
void r1cs_last_timings(float ms[8]) { const CallTimes t = g_r1cs_last.read(); for (int i = 0; i < 8; i++) ms[i] = t.ms[i]; }

// one CSR structure on the device with its binning
struct DevCsr {
  uint64_t* row_ptr = nullptr;
  uint32_t* col = nullptr;
  uint64_t* val = nullptr;
  uint32_t *long_rows = nullptr, *long_first = nullptr, *chunk_li = nullptr;
  uint32_t rows = 0, n_long = 0, n_chunks = 0;
  uint64_t nnz = 0;
};
struct R1cs {
  int curve = 0, device = 0;
  size_t m = 0, n_vars = 0, n_inputs = 0;
  DevCsr mat[3], tr[3];          // the matrices (rows = constraints) and their transposes (rows = variables)
  size_t bytes = 0;
};

// ---- the product kernels (r1cs.h).  Lists of at most R1CS_LONG entries: one lane each.
template <class FR>
__global__ void __launch_bounds__(256) k_r1cs_short(const uint64_t* __restrict__ row_ptr, const uint32_t* __restrict__ col, const uint64_t* __restrict__ val,
                                                    uint32_t rows, const uint64_t* __restrict__ vec, uint64_t* __restrict__ out) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const uint64_t lo = row_ptr[r], hi = row_ptr[r + 1];
  if (hi - lo > R1CS_LONG) return;
  r1cs_finish(r1cs_sum<FR>(col, val, vec, lo, hi, 1), out + (size_t)r * FR::ARK64);
}
// one wave per chunk of a long list: lane sums, then lane 0 adds the 64 in lane order
template <class FR>
__global__ void __launch_bounds__(R1CS_WAVE) k_r1cs_chunk(const uint64_t* __restrict__ row_ptr, const uint32_t* __restrict__ col, const uint64_t* __restrict__ val,
                                                          const uint32_t* __restrict__ long_rows, const uint32_t* __restrict__ long_first,
                                                          const uint32_t* __restrict__ chunk_li, const uint64_t* __restrict__ vec, uint32_t* __restrict__ parts) {
  __shared__ __attribute__((aligned(16))) uint32_t lanes[R1CS_WAVE * FR::WORDS];
  const uint32_t c = blockIdx.x, t = threadIdx.x, li = chunk_li[c], r = long_rows[li];
  uint64_t c_lo, c_hi;
  r1cs_chunk_range(row_ptr[r], row_ptr[r + 1], c - long_first[li], c_lo, c_hi);
  r1cs_sum<FR>(col, val, vec, c_lo + t, c_hi, R1CS_WAVE).store(lanes + (size_t)t * FR::WORDS);
  __syncthreads();
  if (t == 0) r1cs_combine<FR>(lanes, 0, R1CS_WAVE, 1).store(parts + (size_t)c * FR::WORDS);
}
// one wave per long list: lane t adds its chunks' sums t, t + 64, ..., then lane 0 the 64 lane sums in lane order
template <class FR>
__global__ void __launch_bounds__(R1CS_WAVE) k_r1cs_long(const uint32_t* __restrict__ long_rows, const uint32_t* __restrict__ long_first,
                                                         const uint32_t* __restrict__ parts, uint64_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint32_t lanes[R1CS_WAVE * FR::WORDS];
  const uint32_t li = blockIdx.x, t = threadIdx.x, f = long_first[li];
  r1cs_combine<FR>(parts + (size_t)f * FR::WORDS, t, long_first[li + 1] - f, R1CS_WAVE).store(lanes + (size_t)t * FR::WORDS);
  __syncthreads();
  if (t == 0) r1cs_finish(r1cs_combine<FR>(lanes, 0, R1CS_WAVE, 1), out + (size_t)long_rows[li] * FR::ARK64);
}
template <class FR>
__global__ void __launch_bounds__(64) k_r1cs_lagrange(FR c, FR tau, FR omega, FR omega_inv, uint32_t n, uint64_t* __restrict__ out) {
  const uint64_t j0 = (uint64_t)(blockIdx.x * blockDim.x + threadIdx.x) * R1CS_LAG_BLOCK;
  if (j0 >= n) return;
  r1cs_lagrange_block(c, tau, omega, omega_inv, j0, n - j0 < R1CS_LAG_BLOCK ? (uint32_t)(n - j0) : R1CS_LAG_BLOCK, out);
}
template <class FR>
__global__ void __launch_bounds__(64) k_r1cs_add_inputs(uint64_t* __restrict__ a, const uint64_t* __restrict__ l, uint32_t n_inputs) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_inputs) r1cs_add_input<FR>(a + (size_t)i * FR::ARK64, l + (size_t)i * FR::ARK64);
}
template <class FR>
__global__ void __launch_bounds__(256) k_r1cs_check(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b, const uint64_t* __restrict__ c, uint32_t m,
                                                    uint32_t* __restrict__ first) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  constexpr int A = FR::ARK64;
  if (!r1cs_row_holds<FR>(a + (size_t)j * A, b + (size_t)j * A, c + (size_t)j * A)) atomicMin(first, j);
}

// out (M.rows x N64) = M vec on stream s.  parts: room for M.n_chunks partial sums.
template <class FR>
static void matvec(const DevCsr& M, const uint64_t* vec, uint64_t* out, uint32_t* parts, hipStream_t s) {
  if (M.rows == 0) return;
  hipLaunchKernelGGL((k_r1cs_short<FR>), dim3((M.rows + 255) / 256), dim3(256), 0, s, M.row_ptr, M.col, M.val, M.rows, vec, out);
  if (M.n_long == 0) return;
  hipLaunchKernelGGL((k_r1cs_chunk<FR>), dim3(M.n_chunks), dim3(R1CS_WAVE), 0, s, M.row_ptr, M.col, M.val, M.long_rows, M.long_first, M.chunk_li, vec, parts);
  hipLaunchKernelGGL((k_r1cs_long<FR>), dim3(M.n_long), dim3(R1CS_WAVE), 0, s, M.long_rows, M.long_first, parts, out);
}
static uint32_t max_chunks(const DevCsr* M) {
  uint32_t c = 1;
  for (int k = 0; k < 3; k++) if (M[k].n_chunks > c) c = M[k].n_chunks;
  return c;
}

// ---- load / free
static void csr_free(DevCsr& d) {
  for (void* p : {(void*)d.row_ptr, (void*)d.col, (void*)d.val, (void*)d.long_rows, (void*)d.long_first, (void*)d.chunk_li}) if (p) (void)hipFree(p);
  d = DevCsr();
}
void r1cs_free(R1cs* r) {
  if (!r) return;
  for (int k = 0; k < 3; k++) { csr_free(r->mat[k]); csr_free(r->tr[k]); }
  delete r;
}
template <class T> static int up(T** d, const T* h, size_t count, size_t& bytes) {
  const size_t b = (count ? count : 1) * sizeof(T);
  HIP_TRY(hipMalloc((void**)d, b), 10);
  if (count) HIP_TRY(hipMemcpy(*d, h, count * sizeof(T), hipMemcpyHostToDevice), 10);
  bytes += b;
  return 0;
}
template <int N64>
static int csr_up(DevCsr& d, const uint64_t* row_ptr, const uint32_t* col, const uint64_t* val, size_t rows, uint64_t nnz, size_t& bytes) {
  const R1csBins b = r1cs_bin(row_ptr, rows);
  d.rows = (uint32_t)rows; d.nnz = nnz; d.n_long = (uint32_t)b.long_rows.size(); d.n_chunks = (uint32_t)b.chunk_li.size();
  if (int rc = up(&d.row_ptr, row_ptr, rows + 1, bytes)) return rc;
  if (int rc = up(&d.col, col, nnz, bytes)) return rc;
  if (int rc = up(&d.val, val, nnz * N64, bytes)) return rc;
  if (int rc = up(&d.long_rows, b.long_rows.data(), b.long_rows.size(), bytes)) return rc;
  if (int rc = up(&d.long_first, b.long_first.data(), b.long_first.size(), bytes)) return rc;
  return up(&d.chunk_li, b.chunk_li.data(), b.chunk_li.size(), bytes);
}
template <class P>
static int load_t(int curve, size_t m, size_t n_vars, size_t n_inputs, const R1csCsr* mats, R1cs** out, uint64_t* first_bad) {
  constexpr int N64 = P::N64;
  if (out) *out = nullptr;
  if (int rc0 = api_enter()) return rc0;
  if (!out) return 2;
  const WallMs wall;
  if (int rc = r1cs_validate<N64>(m, n_vars, n_inputs, mats, P::P64, first_bad)) return rc;
  R1cs* r = new R1cs();
  r->curve = curve; r->device = api_device(); r->m = m; r->n_vars = n_vars; r->n_inputs = n_inputs;
  int rc = 0;
  for (int k = 0; k < 3 && !rc; k++) {
    rc = csr_up<N64>(r->mat[k], mats[k].row_ptr, mats[k].col, mats[k].val, m, mats[k].nnz, r->bytes);
    if (rc) break;
    std::vector<uint64_t> t_ptr, t_val;
    std::vector<uint32_t> t_idx;
    r1cs_transpose<N64>(m, n_vars, mats[k], t_ptr, t_idx, t_val);
    rc = csr_up<N64>(r->tr[k], t_ptr.data(), t_idx.data(), t_val.data(), n_vars, mats[k].nnz, r->bytes);
  }
  if (rc) { r1cs_free(r); return rc; }
  *out = r;
  r1cs_note_ms(0, wall.ms());
  return 0;
}
int r1cs_load(int curve, size_t m, size_t n_vars, size_t n_inputs, const uint64_t* const row_ptr[3], const uint32_t* const col[3], const uint64_t* const val[3],
              const uint64_t nnz[3], R1cs** out, uint64_t* first_bad) {
  const R1csCsr mats[3] = {{row_ptr[0], col[0], val[0], nnz[0]}, {row_ptr[1], col[1], val[1], nnz[1]}, {row_ptr[2], col[2], val[2], nnz[2]}};
  return curve == 0 ? load_t<P377>(0, m, n_vars, n_inputs, mats, out, first_bad) : load_t<P253>(1, m, n_vars, n_inputs, mats, out, first_bad);
}
int r1cs_info(const R1cs* r, uint64_t out[8]) {
  if (!r || !out) return 2;
  const uint64_t v[8] = {(uint64_t)r->curve, r->m, r->n_vars, r->n_inputs, r->mat[0].nnz, r->mat[1].nnz, r->mat[2].nnz, r->bytes};
  memcpy(out, v, sizeof v);
  return 0;
}
// what the chained entry points of unit_prover.hip / unit_setup.hip need to know of a handle
void r1cs_shape(const R1cs* r, int* curve, int* device, size_t* m, size_t* n_vars, size_t* n_inputs) {
  *curve = r->curve; *device = r->device; *m = r->m; *n_vars = r->n_vars; *n_inputs = r->n_inputs;
}

// ---- prover side: (A z, B z, C z) over 2^log_n rows.  z and the outputs: host or device pointers (runtime.h, the call frame).
template <class FR>
static int rows_t(const R1cs* r, const uint64_t* z, unsigned log_n, uint64_t* oa, uint64_t* ob, uint64_t* oc, int dev, void* stream_) {
  constexpr int A = FR::ARK64;
  if (log_n > 28 || (size_t(1) << log_n) < r->m + r->n_inputs) return 2;
  const size_t n = size_t(1) << log_n, bytes = n * A * 8;
  CallScope cs;
  HIP_TRY(cs.open(dev, stream_), 10);
  const hipStream_t s = cs.stream();
  uint64_t *d_z, *d_o[3], *h_o[3] = {oa, ob, oc};
  uint32_t* parts;
  HIP_TRY(cs.alloc(&parts, (size_t)max_chunks(r->mat) * FR::WORDS * 4), 10);
  HIP_TRY(cs.in(&d_z, z, r->n_vars * A * 8, dev), 10);
  for (int k = 0; k < 3; k++) HIP_TRY(cs.out(&d_o[k], h_o[k], bytes, dev), 10);
  EvLog log(s);
  float ms[8] = {};
  if (n > r->m) for (int k = 0; k < 3; k++) HIP_TRY(hipMemsetAsync(d_o[k] + r->m * A, 0, (n - r->m) * A * 8, s), 10);
  hipEvent_t e0 = log.open();
  for (int k = 0; k < 3; k++) matvec<FR>(r->mat[k], d_z, d_o[k], parts, s);
  log.close(1, e0);
  HIP_TRY(hipGetLastError(), 10);
  // the input-consistency rows a[m + i] = z_i
  HIP_TRY(hipMemcpyAsync(d_o[0] + r->m * A, d_z, r->n_inputs * A * 8, hipMemcpyDeviceToDevice, s), 10);
  HIP_TRY(cs.copy_back(), 10);
  HIP_TRY(hipStreamSynchronize(s), 10);
  log.sum(ms);
  r1cs_note_ms(1, ms[1]);
  return 0;
}
int r1cs_rows(const R1cs* r, const uint64_t* z, unsigned log_n, uint64_t* oa, uint64_t* ob, uint64_t* oc, int dev, void* stream) {
  if (int rc0 = api_enter()) return rc0;
  if (!r || !z || !oa || !ob || !oc) return 2;
  if (r->device != api_device()) return 101;
  return r->curve == 0 ? rows_t<FrBw6>(r, z, log_n, oa, ob, oc, dev, stream) : rows_t<FrBls>(r, z, log_n, oa, ob, oc, dev, stream);
}

template <class FR>
static int check_t(const R1cs* r, const uint64_t* z, int64_t* first_unsatisfied) {
  constexpr int A = FR::ARK64;
  *first_unsatisfied = -1;
  if (r->m == 0) return 0;
  CallScope cs;
  HIP_TRY(cs.open(0, nullptr), 10);
  const hipStream_t s = cs.stream();
  uint64_t *d_z, *d_o[3];
  uint32_t *parts, *d_first, first = 0xffffffffu;
  HIP_TRY(cs.in(&d_z, z, r->n_vars * A * 8, 0), 10);
  for (int k = 0; k < 3; k++) HIP_TRY(cs.alloc(&d_o[k], r->m * A * 8), 10);
  HIP_TRY(cs.alloc(&parts, (size_t)max_chunks(r->mat) * FR::WORDS * 4), 10);
  HIP_TRY(cs.alloc(&d_first, 4), 10);
  HIP_TRY(hipMemsetAsync(d_first, 0xff, 4, s), 10);
  for (int k = 0; k < 3; k++) matvec<FR>(r->mat[k], d_z, d_o[k], parts, s);
  hipLaunchKernelGGL((k_r1cs_check<FR>), dim3((unsigned)((r->m + 255) / 256)), dim3(256), 0, s, d_o[0], d_o[1], d_o[2], (uint32_t)r->m, d_first);
  HIP_TRY(hipGetLastError(), 10);
  HIP_TRY(hipMemcpyAsync(&first, d_first, 4, hipMemcpyDeviceToHost, s), 10);
  HIP_TRY(hipStreamSynchronize(s), 10);
  if (first != 0xffffffffu) *first_unsatisfied = (int64_t)first;
  return 0;
}
int r1cs_check(const R1cs* r, const uint64_t* z, int64_t* first_unsatisfied) {
  if (int rc0 = api_enter()) return rc0;
  if (!r || !z || !first_unsatisfied) return 2;
  if (r->device != api_device()) return 101;
  return r->curve == 0 ? check_t<FrBw6>(r, z, first_unsatisfied) : check_t<FrBls>(r, z, first_unsatisfied);
}

// ---- setup side: a_i(tau), b_i(tau), c_i(tau) for the n_vars variables and zt = Z(tau) (a host pointer in both forms).
// oa / ob / oc: host or device pointers (runtime.h, the call frame).
template <class FR>
static int qap_t(const R1cs* r, unsigned log_n, const uint64_t* omega, const uint64_t* tau, uint64_t* oa, uint64_t* ob, uint64_t* oc, uint64_t* ozt, int dev,
                 void* stream_) {
  constexpr int A = FR::ARK64;
  if (log_n > 28 || (size_t(1) << log_n) < r->m + r->n_inputs) return 2;
  const size_t n = size_t(1) << log_n, bytes = r->n_vars * A * 8;
  const R1csLagConsts<FR> k = r1cs_lagrange_consts<FR>(log_n, omega, tau, ozt);
  CallScope cs;
  HIP_TRY(cs.open(dev, stream_), 10);
  const hipStream_t s = cs.stream();
  uint64_t *d_l, *d_o[3], *h_o[3] = {oa, ob, oc};
  uint32_t* parts;
  HIP_TRY(cs.alloc(&d_l, n * A * 8), 10);
  HIP_TRY(cs.alloc(&parts, (size_t)max_chunks(r->tr) * FR::WORDS * 4), 10);
  for (int q = 0; q < 3; q++) HIP_TRY(cs.out(&d_o[q], h_o[q], bytes, dev), 10);
  EvLog log(s);
  float ms[8] = {};
  hipEvent_t e0 = log.open();
  const size_t lanes = (n + R1CS_LAG_BLOCK - 1) / R1CS_LAG_BLOCK;
  hipLaunchKernelGGL((k_r1cs_lagrange<FR>), dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, s, k.c, k.tau, k.omega, k.omega_inv, (uint32_t)n, d_l);
  log.close(2, e0);
  e0 = log.open();
  for (int q = 0; q < 3; q++) matvec<FR>(r->tr[q], d_l, d_o[q], parts, s);
  hipLaunchKernelGGL((k_r1cs_add_inputs<FR>), dim3((unsigned)((r->n_inputs + 63) / 64)), dim3(64), 0, s, d_o[0], d_l + r->m * A, (uint32_t)r->n_inputs);
  log.close(3, e0);
  HIP_TRY(hipGetLastError(), 10);
  HIP_TRY(cs.copy_back(), 10);
  HIP_TRY(hipStreamSynchronize(s), 10);
  log.sum(ms);
  r1cs_note_ms(2, ms[2]);
  r1cs_note_ms(3, ms[3]);
  return 0;
}
int r1cs_qap_at_tau(const R1cs* r, unsigned log_n, const uint64_t* omega, const uint64_t* tau, uint64_t* oa, uint64_t* ob, uint64_t* oc, uint64_t* ozt, int dev,
                    void* stream) {
  if (int rc0 = api_enter()) return rc0;
  if (!r || !omega || !tau || !oa || !ob || !oc || !ozt) return 2;
  if (r->device != api_device()) return 101;
  return r->curve == 0 ? qap_t<FrBw6>(r, log_n, omega, tau, oa, ob, oc, ozt, dev, stream) : qap_t<FrBls>(r, log_n, omega, tau, oa, ob, oc, ozt, dev, stream);
}

}  // namespace celo
