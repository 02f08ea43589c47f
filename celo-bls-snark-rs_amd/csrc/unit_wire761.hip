// Translation unit: bulk decoding of serialized BW6-761 points (see wire761.h), one point per lane, and the loader of a serialized
// ark-groth16 0.1 ProvingKey<BW6_761> or ProvingKey<Bls12_377> (the latter's points through unit_wire.hip's kernels) that decodes its point
// sections on the device straight into the buffers the fixed-base table build reads.
#include "wire761.h"
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdio>
#include <mutex>
#include "runtime.h"
#include "units.h"

// one wave per SIMD: the square root (four odd powers and the running power, 5 x 28 registers) and the ladder (XYZZ accumulator 4 x 28, the
// point 2 x 28, the addition's temporaries) do not fit 256 VGPRs.  With the AGPR half of the file k_decode761 needs no scratch and
// k_subgroup761 36 B/lane (build/unit_wire761.remarks.txt; DESIGN.md section 6c')
#ifndef W761_OCC
#define W761_OCC __attribute__((amdgpu_waves_per_eu(1, 1)))
#endif
namespace celo {
// calls from several host threads are serialised per process (they are bulk calls: one fills the GPU); each runs on a stream of its own
// (host-pointer calls) or on the caller's (the _dev forms).  The lock guards nothing else: serialisation only
static std::mutex w761_mu;
// [0] kernel ms of the last decode call; [1] .. [3] the last key load's transfer / decode / table build (each call owns its slots)
static Last<CallTimes> g_w761_last;

// Two passes, one point per lane (the second is unit_check.hip's k_endo761 by default; k_subgroup761 is its twin, hook 1).  k_decode761: in n x 96 B (compressed) / n x 192 B (uncompressed) -> out n x 24 u64, (x, y) in arkworks
// Montgomery limbs (the layout of msm_bw6_761_*), zeros unless status == WIRE_OK; everything but the subgroup test.  k_subgroup761: r P == O
// for the rows still at status 0 (status 3 and a zero row otherwise); one kernel for both groups (the ladder does not depend on b).  Split
// because the square root's four odd powers and the ladder's XYZZ state are never live together then: the first pass needs no scratch.
// Control flow is uniform across the wave up to the per-lane status exits: the root's exponent and the ladder's r are compile-time constants.
template <int B, bool COMPRESSED> __global__ void __launch_bounds__(64) W761_OCC
k_decode761(const uint8_t* __restrict__ in, uint64_t* __restrict__ out, uint8_t* __restrict__ status, uint32_t n, int check) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Affine<Fw761> p = {Fw761::zero(), Fw761::zero()};
  const WireStatus st = w761_parse<B, COMPRESSED>(in + (size_t)i * (COMPRESSED ? 96 : 192), check != 0, p);
  uint64_t* o = out + (size_t)i * 24;
  if (st == WIRE_OK) { p.x.to_ark(o); p.y.to_ark(o + 12); }
  else for (int j = 0; j < 24; j++) o[j] = 0;
  status[i] = st;
}
__global__ void __launch_bounds__(64) W761_OCC k_subgroup761(uint64_t* __restrict__ out, uint8_t* __restrict__ status, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || status[i] != WIRE_OK) return;
  uint64_t* o = out + (size_t)i * 24;
  const Affine<Fw761> p = {Fw761::norm(Fw761::from_ark(o)), Fw761::norm(Fw761::from_ark(o + 12))};
  if (w761_in_subgroup(p)) return;
  for (int j = 0; j < 24; j++) o[j] = 0;
  status[i] = WIRE_NOT_IN_SUBGROUP;
}
// the smallest index of a rejected point (status 2 or 3)
__global__ void __launch_bounds__(256) k_first_bad761(const uint8_t* __restrict__ status, uint32_t n, unsigned long long* first) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && status[i] >= WIRE_INVALID) atomicMin(first, (unsigned long long)i);
}

// which subgroup pass the decoders (and check_points_bw6_761_*) launch: 0 = k_endo761 (unit_check.hip), 1 = k_subgroup761 above
static std::atomic<int> g_w761_subgroup_test{0};
static void launch_decode761(int g2, int compressed, const uint8_t* d_in, size_t n, int check, uint64_t* d_out, uint8_t* d_st, hipStream_t s) {
  const dim3 grid(((uint32_t)n + 63) / 64), block(64);
  if (g2) {
    if (compressed) hipLaunchKernelGGL((k_decode761<4, true>), grid, block, 0, s, d_in, d_out, d_st, (uint32_t)n, check);
    else hipLaunchKernelGGL((k_decode761<4, false>), grid, block, 0, s, d_in, d_out, d_st, (uint32_t)n, check);
  } else {
    if (compressed) hipLaunchKernelGGL((k_decode761<-1, true>), grid, block, 0, s, d_in, d_out, d_st, (uint32_t)n, check);
    else hipLaunchKernelGGL((k_decode761<-1, false>), grid, block, 0, s, d_in, d_out, d_st, (uint32_t)n, check);
  }
  if (!check) return;
  // the subgroup pass: the endomorphism form (unit_check.hip k_endo761) unless the hook asks for the ladder; the verdicts and rows are the same
  if (g_w761_subgroup_test.load() == 0) check761_launch_endo(g2, d_out, d_out, d_st, n, s);
  else hipLaunchKernelGGL(k_subgroup761, grid, block, 0, s, d_out, d_st, (uint32_t)n);
}
// celo_amd_wire761_set_subgroup_test: 0 = [a]P + [b]phi(P) == O (the default), 1 = the r P ladder; 2 for anything else
int wire761_set_subgroup_test(int form) {
  if (form != 0 && form != 1) return 2;
  g_w761_subgroup_test.store(form);
  return 0;
}
int wire761_subgroup_test() { return g_w761_subgroup_test.load(); }
// the ladder pass on rows the caller owns (unit_check.hip, under hook 1)
void wire761_launch_ladder(uint64_t* d_rows, uint8_t* d_st, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_subgroup761, dim3(((uint32_t)n + 63) / 64), dim3(64), 0, s, d_rows, d_st, (uint32_t)n);
}

// g2: 0 = G1 (b = -1), 1 = G2 (b = 4); compressed: 1 = 96 B points, 0 = 192 B; dev: all four pointers are device pointers, run on stream_
int wire761_decode(int g2, int compressed, const uint8_t* in, size_t n, int check, uint64_t* out, uint8_t* status, int dev, void* stream_) {
  if (int rc0 = api_enter()) return rc0;
  std::lock_guard<std::mutex> lk(w761_mu);
  if (n == 0) return 0;
  if (!in || !out || !status || n > 0x7fffffffu) return 2;
  const size_t ib = compressed ? 96 : 192;
  CallScope cs;
  HIP_TRY(cs.open(dev, stream_), 10);
  const hipStream_t stream = cs.stream();
  uint8_t *d_in, *d_st;
  uint64_t* d_out;
  HIP_TRY(cs.in(&d_in, in, n * ib, dev), 10);
  HIP_TRY(cs.out(&d_out, out, n * 24 * 8, dev), 10);
  HIP_TRY(cs.out(&d_st, status, n, dev), 10);
  EvLog log(stream);
  const hipEvent_t e0 = log.open();
  launch_decode761(g2, compressed, d_in, n, check, d_out, d_st, stream);
  HIP_TRY(hipGetLastError(), 10);
  log.close(0, e0);
  HIP_TRY(cs.copy_back(), 10);
  HIP_TRY(hipStreamSynchronize(stream), 10);
  float ms = 0.f;
  log.sum(&ms);
  g_w761_last.update([&](CallTimes& t) { t.ms[0] = ms; });
  return 0;
}

int wire_key_layout(int curve, const uint8_t* bytes, size_t len, int form, uint64_t out[16]) { return wkey_layout(curve, bytes, len, form, out); }

// one point of a key, decoded again on the host (unchecked: the device has checked it) into the row the key keeps there
static WireStatus key_host_row(int curve, int g2, int compressed, const uint8_t* src, uint64_t* row) {
  if (curve == 0) {
    if (g2) return compressed ? w761_decode_row<4, true>(src, false, row) : w761_decode_row<4, false>(src, false, row);
    return compressed ? w761_decode_row<-1, true>(src, false, row) : w761_decode_row<-1, false>(src, false, row);
  }
  const WireConsts& k = wire_consts();
  if (g2) return compressed ? wire_decode_row_g2<true>(src, k, false, row) : wire_decode_row_g2<false>(src, k, false, row);
  return compressed ? wire_decode_row_g1<true>(src, k, false, row) : wire_decode_row_g1<false>(src, k, false, row);
}

// ProvingKey::<E>::deserialize (form 0) / deserialize_uncompressed (1) / deserialize_unchecked (2), then groth16_load_key_<curve>; curve 0 =
// BW6-761, 1 = BLS12-377.  The whole byte string crosses to the device once; every point of every section is decoded there (one launch per
// section: k_decode761 + the subgroup pass, or unit_wire.hip's k_decompress / k_decode377u) into a G1 row buffer and a G2 row buffer (24 u64 per
// row; BLS12-377 G1: 12), each in serialization order, with one status array indexed by the point's position in serialization order.  The first
// rejected index is found by an atomic minimum, and the four queries' rows and statuses are handed to the table build where they lie (a status-1
// row - the point at infinity - is that query's identity through the build's `inf` bytes: after the check every status is 0 or 1).
// a_query[0], b_g2_query[0], alpha_g1 and beta_g2, which the key keeps on the host, are decoded again on the host from their bytes.
int wire_key_load(int curve, const uint8_t* bytes, size_t len, int form, int window_bits, ProvingKey** out_key, uint64_t* first_bad) {
  if (!out_key) return 2;
  *out_key = nullptr;
  uint64_t L[16];
  if (int rcl = wkey_layout(curve, bytes, len, form, L)) return rcl;
  if (L[W761_A] == 0 || L[W761_BG2] == 0) return 2;                 // the proof needs a_query[0] and b_g2_query[0]
  if (L[W761_NPOINTS] > 0x7fffffffu) return 2;
  if (int rc0 = api_enter()) return rc0;
  std::lock_guard<std::mutex> lk(w761_mu);
  const int compressed = form == 0, check = form != 2;
  const uint64_t P = L[W761_PT], N = L[W761_NPOINTS], w1 = curve ? 12 : 24, w2 = 24;    // u64 per G1 / G2 row
  struct Sec { uint64_t off, n; int g2; };
  const Sec secs[9] = {{0, 1, 0},     {P, 3, 1},           {L[W761_ABC + 1], L[W761_ABC], 0}, {L[W761_BETA_G1], 2, 0}, {L[W761_A + 1], L[W761_A], 0},
                       {L[W761_BG1 + 1], L[W761_BG1], 0}, {L[W761_BG2 + 1], L[W761_BG2], 1}, {L[W761_H + 1], L[W761_H], 0}, {L[W761_L + 1], L[W761_L], 0}};
  uint64_t base[9], row[9], n_grp[2] = {0, 0};                       // a section's first point: in serialization order, among its group's rows
  for (uint64_t s = 0, acc = 0; s < 9; s++) {
    base[s] = acc;
    acc += secs[s].n;
    row[s] = n_grp[secs[s].g2];
    n_grp[secs[s].g2] += secs[s].n;
  }
  CallScope cs(nullptr);
  HIP_TRY(cs.create_stream(), 10);
  const hipStream_t stream = cs.stream();
  hipEvent_t ev[3];
  for (auto& e : ev) HIP_TRY(cs.event(&e), 10);
  uint8_t *d_bytes, *d_st;
  uint64_t* d_xy[2];
  unsigned long long* d_first;
  unsigned long long first = ~0ull;
  HIP_TRY(cs.alloc(&d_bytes, len), 10);
  HIP_TRY(cs.alloc(&d_xy[0], n_grp[0] * w1 * 8), 10);
  HIP_TRY(cs.alloc(&d_xy[1], n_grp[1] * w2 * 8), 10);
  HIP_TRY(cs.alloc(&d_st, N), 10);
  HIP_TRY(cs.alloc(&d_first, sizeof(unsigned long long)), 10);
  auto rows_of = [&](int s) { return d_xy[secs[s].g2] + row[s] * (secs[s].g2 ? w2 : w1); };
  HIP_TRY(hipEventRecord(ev[0], stream), 10);
  HIP_TRY(hipMemcpyAsync(d_bytes, bytes, len, hipMemcpyHostToDevice, stream), 10);
  HIP_TRY(hipMemcpyAsync(d_first, &first, sizeof first, hipMemcpyHostToDevice, stream), 10);
  HIP_TRY(hipEventRecord(ev[1], stream), 10);
  for (int s = 0; s < 9; s++) {
    if (!secs[s].n) continue;
    if (curve == 0) {
      launch_decode761(secs[s].g2, compressed, d_bytes + secs[s].off, secs[s].n, check, rows_of(s), d_st + base[s], stream);
      HIP_TRY(hipGetLastError(), 10);
    } else if (int rcd = wire377_launch_decode(secs[s].g2, compressed, d_bytes + secs[s].off, secs[s].n, check, rows_of(s), d_st + base[s], stream)) return rcd;
  }
  hipLaunchKernelGGL(k_first_bad761, dim3(((uint32_t)N + 255) / 256), dim3(256), 0, stream, d_st, (uint32_t)N, d_first);
  HIP_TRY(hipGetLastError(), 10);
  HIP_TRY(hipEventRecord(ev[2], stream), 10);
  HIP_TRY(hipMemcpyAsync(&first, d_first, sizeof first, hipMemcpyDeviceToHost, stream), 10);
  HIP_TRY(hipStreamSynchronize(stream), 10);
  float ms_xfer = 0.f, ms_decode = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms_xfer, ev[0], ev[1]), 10);
  HIP_TRY(hipEventElapsedTime(&ms_decode, ev[1], ev[2]), 10);
  g_w761_last.update([&](CallTimes& t) { t.ms[1] = ms_xfer; t.ms[2] = ms_decode; });
  if (first != ~0ull) {
    if (first_bad) *first_bad = first;
    return W761_ERR_POINT;
  }
  // the four key elements the composition keeps on the host (ark's identity encoding (0, 1) for the point at infinity)
  uint64_t host_rows[4][24];
  const uint64_t where[4] = {secs[4].off, secs[6].off, 0, P};      // a_query[0], b_g2_query[0], alpha_g1, beta_g2
  const int grp[4] = {0, 1, 0, 1};
  for (int q = 0; q < 4; q++) {
    const WireStatus st = key_host_row(curve, grp[q], compressed, bytes + where[q], host_rows[q]);
    const uint64_t y_at = (grp[q] ? w2 : w1) / 2;                     // y (an Fq2 y: its c0) in the row
    if (st == WIRE_INFINITY) { if (curve) Fq::one().to_ark(host_rows[q] + y_at); else Fw761::one().to_ark(host_rows[q] + y_at); }
    else if (st != WIRE_OK) return 10;                                // not reached: the same function accepted these bytes on the device
  }
  const WallMs wall;
  // (frees the key itself when it fails, and sets *out_key only on success: the call's last step)
  const int rc = groth16_key_load_dev(curve, rows_of(4), d_st + base[4], L[W761_A], rows_of(6), d_st + base[6], L[W761_BG2], rows_of(7), d_st + base[7], L[W761_H],
                                      rows_of(8), d_st + base[8], L[W761_L], host_rows[0], host_rows[1], host_rows[2], host_rows[3], window_bits, out_key);
  g_w761_last.update([&](CallTimes& t) { t.ms[3] = wall.ms(); });
  return rc;
}
void wire761_last_timings(float ms[4]) { const CallTimes t = g_w761_last.read(); for (int i = 0; i < 4; i++) ms[i] = t.ms[i]; }
}  // namespace celo
