// Translation unit: bulk decoding of BLS12-377 points, compressed and uncompressed (see wire.h), one point per lane, and the batch
// normalisation of Jacobian points of both curves (normalize.h).
#include "wire.h"
#include "normalize.h"
#include <hip/hip_runtime.h>
#include <mutex>
#include "runtime.h"
#include "units.h"

// two waves per SIMD (scratch instead of AGPRs for what does not fit 256 VGPRs) unless overridden: -DFROW_OCC= for the A/B
#ifndef FROW_OCC
#define FROW_OCC __attribute__((amdgpu_waves_per_eu(2, 2)))
#endif
namespace celo {
// decode / normalise calls stage through the call frame of runtime.h and run on the caller's stream in both forms (the null stream when
// none is given); calls from several host threads are serialised per process by this lock (bulk calls: one fills the GPU) - serialisation only
static std::mutex wire_mu;

// in: n x 48 (G1) / n x 96 (G2) wire bytes.  out: n x 12 / n x 24 u64, affine (x, y) in arkworks Montgomery limbs (the layout
// the MSM and pairing entry points take), zeros unless status == WIRE_OK.  Control flow is uniform apart from the table scans of the square
// root; the subgroup test (64-bit ladders by the curve parameter x, wire.h) uses the same scalar in every lane.
template <bool G2> __global__ void __launch_bounds__(64) FROW_OCC k_decompress(const uint8_t* __restrict__ in, uint64_t* __restrict__ out,
                                                                      uint8_t* __restrict__ status, uint32_t n, int check, WireConsts k) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if constexpr (G2) {
    Affine<Fq2> p = {Fq2::zero(), Fq2::zero()};
    const WireStatus st = wire_decode_g2(in + (size_t)i * 96, k, check != 0, p);
    uint64_t* o = out + (size_t)i * 24;
    if (st == WIRE_OK) { p.x.c0.to_ark(o); p.x.c1.to_ark(o + 6); p.y.c0.to_ark(o + 12); p.y.c1.to_ark(o + 18); }
    else for (int j = 0; j < 24; j++) o[j] = 0;
    status[i] = st;
  } else {
    Affine<Fq> p = {Fq::zero(), Fq::zero()};
    const WireStatus st = wire_decode_g1(in + (size_t)i * 48, k, check != 0, p);
    uint64_t* o = out + (size_t)i * 12;
    if (st == WIRE_OK) { p.x.to_ark(o); p.y.to_ark(o + 6); }
    else for (int j = 0; j < 12; j++) o[j] = 0;
    status[i] = st;
  }
}

// The uncompressed forms (wire.h wire_decode_row_*<false>): in n x 96 (G1) / n x 192 (G2) bytes, x then y; out and status as above.  check:
// the curve equation and the same subgroup test; 0: the canonical range alone.  No square root, so no table and no run-time-indexed array;
// one kernel per group (a split into parse and subgroup passes, as unit_wire761.hip has it, would buy nothing here: DESIGN.md section 6c''').
template <bool G2> __global__ void __launch_bounds__(64) FROW_OCC k_decode377u(const uint8_t* __restrict__ in, uint64_t* __restrict__ out,
                                                                      uint8_t* __restrict__ status, uint32_t n, int check, WireConsts k) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if constexpr (G2) status[i] = wire_decode_row_g2<false>(in + (size_t)i * 192, k, check != 0, out + (size_t)i * 24);
  else status[i] = wire_decode_row_g1<false>(in + (size_t)i * 96, k, check != 0, out + (size_t)i * 12);
}

// the constants with the discrete-log tables in device memory: one copy per device, uploaded on first use there
int wire_consts_device(WireConsts& out) {
  static std::mutex mu;
  static WireTables* d_tabs[MAX_DEVICES] = {};
  std::lock_guard<std::mutex> lk(mu);
  WireTables*& d_tab = d_tabs[api_device()];
  out = wire_consts();
  if (!d_tab) {
    if (hipMalloc(&d_tab, sizeof(WireTables)) != hipSuccess) { d_tab = nullptr; return 10; }
    if (hipMemcpy(d_tab, out.tab, sizeof(WireTables), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d_tab); d_tab = nullptr; return 10; }
  }
  out.tab = d_tab;
  return 0;
}
int wire_consts_warm() { WireConsts k; return wire_consts_device(k); }
static Last<float> g_wire_last;               // kernel ms of the last decode or normalise call that succeeded

// one decode launch on device buffers (the entry points below; the serialized-key loader of unit_wire761.hip, one per section)
int wire377_launch_decode(int g2, int compressed, const uint8_t* d_in, size_t n, int check, uint64_t* d_out, uint8_t* d_st, hipStream_t stream) {
  WireConsts k = wire_consts();
  if (compressed) { if (int rck = wire_consts_device(k)) return rck; }
  else k.tab = nullptr;                                               // the uncompressed forms take no root
  const dim3 grid(((uint32_t)n + 63) / 64), block(64);
  if (compressed) {
    if (g2) hipLaunchKernelGGL((k_decompress<true>), grid, block, 0, stream, d_in, d_out, d_st, (uint32_t)n, check, k);
    else hipLaunchKernelGGL((k_decompress<false>), grid, block, 0, stream, d_in, d_out, d_st, (uint32_t)n, check, k);
  } else {
    if (g2) hipLaunchKernelGGL((k_decode377u<true>), grid, block, 0, stream, d_in, d_out, d_st, (uint32_t)n, check, k);
    else hipLaunchKernelGGL((k_decode377u<false>), grid, block, 0, stream, d_in, d_out, d_st, (uint32_t)n, check, k);
  }
  return hipGetLastError() == hipSuccess ? 0 : 10;
}

int wire_decompress(int g2, const uint8_t* in, size_t n, int check, uint64_t* out, uint8_t* status, int dev, void* stream_, float* kernel_ms) {
  return wire377_decode(g2, 1, in, n, check, out, status, dev, stream_, kernel_ms);
}
// compressed: 1 = 48 / 96 B points (k_decompress), 0 = 96 / 192 B (k_decode377u)
int wire377_decode(int g2, int compressed, const uint8_t* in, size_t n, int check, uint64_t* out, uint8_t* status, int dev, void* stream_, float* kernel_ms) {
  if (int rc0 = api_enter()) return rc0;
  std::lock_guard<std::mutex> lk(wire_mu);
  if (n == 0) return 0;
  if (!in || !out || !status || n > 0x7fffffffu) return 2;
  if (!compressed && dev && ((uintptr_t)out & 7)) return 2;           // the rows are stored as 64-bit words
  if (compressed) {                                                   // first use on this device: the tables' upload stays outside the events
    WireConsts k;
    if (int rck = wire_consts_device(k)) return rck;
  }
  const size_t ib = (g2 ? 96 : 48) * (compressed ? 1 : 2), ow = g2 ? 24 : 12;
  CallScope cs((hipStream_t)stream_);
  const hipStream_t stream = cs.stream();
  uint8_t *d_in, *d_st;
  uint64_t* d_out;
  HIP_TRY(cs.in(&d_in, in, n * ib, dev), 10);
  HIP_TRY(cs.out(&d_out, out, n * ow * 8, dev), 10);
  HIP_TRY(cs.out(&d_st, status, n, dev), 10);
  EvLog log(stream);
  const hipEvent_t e0 = log.open();
  if (int rcl = wire377_launch_decode(g2, compressed, d_in, n, check, d_out, d_st, stream)) return rcl;
  log.close(0, e0);
  HIP_TRY(cs.copy_back(), 10);
  HIP_TRY(hipStreamSynchronize(stream), 10);
  float ms = 0.f;
  log.sum(&ms);
  g_wire_last.note(ms);
  if (kernel_ms) *kernel_ms = ms;
  return 0;
}
// Jacobian -> affine for n points (normalize.h): jac n x 3 coordinates, out_xy n x (x, y), zero rows + inf[i] = 1 for the identity.
// group 0: BLS12-377 G1, 1: BLS12-377 G2 (both at two waves per SIMD), 2: BW6-761 (G1 and G2: one coordinate field)
int wire_normalize(int group, const uint64_t* jac, size_t n, uint64_t* out_xy, uint8_t* inf) {
  if (int rc0 = api_enter()) return rc0;
  std::lock_guard<std::mutex> lk(wire_mu);
  if (n == 0) return 0;
  if (!jac || !out_xy || !inf || n > 0x7fffffffu) return 2;
  const size_t cw = group ? 12 : 6;
  CallScope cs(nullptr);
  uint64_t *d_in, *d_out;
  uint8_t* d_inf;
  HIP_TRY(cs.in(&d_in, jac, n * 3 * cw * 8, 0), 10);
  HIP_TRY(cs.out(&d_out, out_xy, n * 2 * cw * 8, 0), 10);
  HIP_TRY(cs.out(&d_inf, inf, n, 0), 10);
  EvLog log(nullptr);
  const hipEvent_t e0 = log.open();
  const dim3 grid4(((uint32_t)((n + 3) / 4) + 63) / 64), grid8(((uint32_t)((n + 7) / 8) + 63) / 64);
  if (group == 2) hipLaunchKernelGGL((k_normalize<Fp<P761>, 4, true, 0, true>), grid4, dim3(64), 0, 0, d_in, d_out, d_inf, (uint32_t)n, 0);
  else if (group == 1) hipLaunchKernelGGL((k_normalize<Fq2, 4, true, 2, false>), grid4, dim3(64), 0, 0, d_in, d_out, d_inf, (uint32_t)n, 0);
  else hipLaunchKernelGGL((k_normalize<Fq, 8, true, 2, false>), grid8, dim3(64), 0, 0, d_in, d_out, d_inf, (uint32_t)n, 0);
  HIP_TRY(hipGetLastError(), 10);
  log.close(0, e0);
  HIP_TRY(cs.copy_back(), 10);
  HIP_TRY(hipStreamSynchronize(0), 10);
  float ms = 0.f;
  log.sum(&ms);
  g_wire_last.note(ms);
  return 0;
}
float wire_last_ms() { return g_wire_last.read(); }
}  // namespace celo
