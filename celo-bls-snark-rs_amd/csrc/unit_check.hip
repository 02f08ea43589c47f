// Translation unit: bulk validation of affine rows (check.h) - check_points_* of include/celo_bls_amd.h, one row per lane - and the
// BW6-761 subgroup test by endomorphism (wire761.h w761_in_subgroup_endo) as the second pass of the BW6-761 decoders (unit_wire761.hip
// launch_decode761) and of the validator.
#include "check.h"
#include <hip/hip_runtime.h>
#include <mutex>
#include "runtime.h"
#include "units.h"

// BW6-761: one wave per SIMD, as unit_wire761.hip and for its reason: the accumulator (4 x 28 registers), the point (2 x 28), beta x (28) and
// the addition's temporaries do not fit 256 VGPRs; with the AGPR half of the file the ladder spills little (build/unit_check.remarks.txt;
// DESIGN.md section 6c').  BLS12-377: two waves per SIMD, as unit_wire.hip's decoders, which run the same subgroup tests.
#ifndef CHECK761_OCC
#define CHECK761_OCC __attribute__((amdgpu_waves_per_eu(1, 1)))
#endif
#ifndef CHECK377_OCC
#define CHECK377_OCC __attribute__((amdgpu_waves_per_eu(2, 2)))
#endif
namespace celo {
// bulk calls, serialised per process (one fills the GPU); each runs on a stream of its own (host pointers) or the caller's (_dev)
static std::mutex check_mu;
static Last<float> g_check_last;              // kernel ms of the last check_points_* call that succeeded

// BLS12-377: the whole check of a row in one kernel (range, curve equation, and at level 2 the endomorphism tests of wire.h), as k_decode377u
template <bool G2> __global__ void __launch_bounds__(64) CHECK377_OCC k_check_rows(const uint64_t* __restrict__ xy, const uint8_t* __restrict__ inf,
                                                                                  uint8_t* __restrict__ status, uint32_t n, int level, WireConsts k) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool flagged = inf != nullptr && inf[i] != 0;
  status[i] = check_row<G2 ? 1 : 0>(xy + (size_t)i * (G2 ? 24 : 12), flagged, level, k);
}
// BW6-761 in two passes, as the decoders: k_check_rows761 is everything up to the curve equation (status 0, 1 or 2), k_endo761 the subgroup
// test of the rows still at status 0 - the ladder's state and the curve check's are never live together.  (The first pass is four
// products on a row of 192 B: it fits 256 VGPRs and is left to the occupancy the compiler finds.)
template <int B> __global__ void __launch_bounds__(64) k_check_rows761(const uint64_t* __restrict__ xy, const uint8_t* __restrict__ inf,
                                                                                   uint8_t* __restrict__ status, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (inf != nullptr && inf[i] != 0) { status[i] = WIRE_INFINITY; return; }
  Affine<Fw761> p = {Fw761::zero(), Fw761::zero()};
  status[i] = check_curve_761<B>(xy + (size_t)i * 24, p);
}
// [a]P + [b]phi(P) == O for the rows at status 0: status 3 otherwise, and the row at zero_rows (the decoders' output rows, which are `rows`
// themselves; NULL for the validator, whose rows are the caller's) set to zeros.  Control flow is uniform across the wave up to the
// per-lane exits and the "accumulator equals the addend" doubling: the digit program is a compile-time constant.
template <int B> __global__ void __launch_bounds__(64) CHECK761_OCC k_endo761(const uint64_t* rows, uint64_t* zero_rows, uint8_t* __restrict__ status, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || status[i] != WIRE_OK) return;
  const uint64_t* r = rows + (size_t)i * 24;
  const Affine<Fw761> p = {Fw761::norm(Fw761::from_ark(r)), Fw761::norm(Fw761::from_ark(r + 12))};
  if (w761_in_subgroup_endo<B>(p)) return;
  if (zero_rows != nullptr) {
    uint64_t* o = zero_rows + (size_t)i * 24;
    for (int j = 0; j < 24; j++) o[j] = 0;
  }
  status[i] = WIRE_NOT_IN_SUBGROUP;
}
// the smallest index of a rejected row (status 2 or 3)
__global__ void __launch_bounds__(256) k_first_bad_row(const uint8_t* __restrict__ status, uint32_t n, unsigned long long* first) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && status[i] >= WIRE_INVALID) atomicMin(first, (unsigned long long)i);
}

void check761_launch_endo(int g2, const uint64_t* d_rows, uint64_t* d_zero_rows, uint8_t* d_st, size_t n, hipStream_t s) {
  const dim3 grid(((uint32_t)n + 63) / 64), block(64);
  if (g2) hipLaunchKernelGGL((k_endo761<4>), grid, block, 0, s, d_rows, d_zero_rows, d_st, (uint32_t)n);
  else hipLaunchKernelGGL((k_endo761<-1>), grid, block, 0, s, d_rows, d_zero_rows, d_st, (uint32_t)n);
}

// cg 0 / 1: BLS12-377 G1 / G2, 2 / 3: BW6-761 G1 / G2; dev: xy, inf and status are device pointers and the work runs on stream_ (first_bad
// is a host pointer in both forms: the call returns after the work has drained)
int check_points(int cg, const uint64_t* xy, const uint8_t* inf, size_t n, int level, uint8_t* status, uint64_t* first_bad, int dev, void* stream_) {
  if (cg < 0 || cg > 3 || level < 1 || level > 2 || n > 0x7fffffffu) return 2;
  if (n == 0) { if (first_bad) *first_bad = 0; return 0; }
  if (!xy || !status) return 2;
  if (int rc0 = api_enter()) return rc0;
  std::lock_guard<std::mutex> lk(check_mu);
  const size_t words = check_row_words(cg);
  CallScope cs;
  HIP_TRY(cs.open(dev, stream_), 10);
  const hipStream_t stream = cs.stream();
  uint64_t* d_xy;                                                       // (the caller's rows with dev set: only read)
  uint8_t *d_inf, *d_st;
  unsigned long long* d_first;
  unsigned long long first = n;
  HIP_TRY(cs.in(&d_xy, xy, n * words * 8, dev), 10);
  HIP_TRY(cs.in(&d_inf, inf, n, dev), 10);
  HIP_TRY(cs.out(&d_st, status, n, dev), 10);
  HIP_TRY(cs.alloc(&d_first, sizeof first), 10);
  HIP_TRY(hipMemcpyAsync(d_first, &first, sizeof first, hipMemcpyHostToDevice, stream), 10);
  uint64_t* d_copy = nullptr;                                           // the ladder kernel zeroes the rows it rejects: it gets a copy
  const bool ladder = cg >= 2 && level == 2 && wire761_subgroup_test() == 1;
  if (ladder) HIP_TRY(cs.alloc(&d_copy, n * words * 8), 10);
  EvLog log(stream);
  const hipEvent_t e0 = log.open();
  const dim3 grid(((uint32_t)n + 63) / 64), block(64);
  if (cg < 2) {
    WireConsts k = wire_consts();
    k.tab = nullptr;                                                    // no square root here: the tables are not touched
    if (cg == 1) hipLaunchKernelGGL((k_check_rows<true>), grid, block, 0, stream, d_xy, d_inf, d_st, (uint32_t)n, level, k);
    else hipLaunchKernelGGL((k_check_rows<false>), grid, block, 0, stream, d_xy, d_inf, d_st, (uint32_t)n, level, k);
  } else {
    if (cg == 3) hipLaunchKernelGGL((k_check_rows761<4>), grid, block, 0, stream, d_xy, d_inf, d_st, (uint32_t)n);
    else hipLaunchKernelGGL((k_check_rows761<-1>), grid, block, 0, stream, d_xy, d_inf, d_st, (uint32_t)n);
    HIP_TRY(hipGetLastError(), 10);
    if (ladder) {
      HIP_TRY(hipMemcpyAsync(d_copy, d_xy, n * words * 8, hipMemcpyDeviceToDevice, stream), 10);
      wire761_launch_ladder(d_copy, d_st, n, stream);
    } else if (level == 2) check761_launch_endo(cg == 3, d_xy, nullptr, d_st, n, stream);
  }
  HIP_TRY(hipGetLastError(), 10);
  hipLaunchKernelGGL(k_first_bad_row, dim3(((uint32_t)n + 255) / 256), dim3(256), 0, stream, d_st, (uint32_t)n, d_first);
  HIP_TRY(hipGetLastError(), 10);
  log.close(0, e0);
  HIP_TRY(hipMemcpyAsync(&first, d_first, sizeof first, hipMemcpyDeviceToHost, stream), 10);
  HIP_TRY(cs.copy_back(), 10);
  HIP_TRY(hipStreamSynchronize(stream), 10);
  if (first_bad) *first_bad = first;
  float ms = 0.f;
  log.sum(&ms);
  g_check_last.note(ms);
  return 0;
}
float check_points_last_ms() { return g_check_last.read(); }
}  // namespace celo
