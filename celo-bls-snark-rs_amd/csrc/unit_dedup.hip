// Translation unit: compressed BLS12-377 keys decoded once per distinct byte string (dedup.h) - decompress_bls12_377_g1/_g2_dedup(_dev) of
// include/celo_bls_amd.h, and the key decoding of the composed epoch entry points (unit_epoch.hip epoch_stage) when the switch says so:
//   k_dedup_insert (the table) -> k_dedup_rep (representatives, compacted) -> U to the host (8 bytes) -> k_dedup_gather (U keys made
//   contiguous) -> wire377_launch_decode on U keys (unit_wire.hip; k_decompress as it is) -> k_dedup_scatter (every key its representative's
//   row and status).  Same bytes in, same kernel, same row out: the outputs are those of the plain decoder bit for bit.  DESIGN.md section 6c.
#include "dedup.h"
#include <hip/hip_runtime.h>
#include <mutex>
#include "runtime.h"
#include "units.h"

namespace celo {
// bulk calls, serialised per process like the decoders'; the lock also guards the three settings
static std::mutex dedup_mu;
static int g_dedup_on = -1, g_dedup_slack = DEDUP_SLACK_DEFAULT, g_dedup_probes = DEDUP_PROBES_DEFAULT;
struct DedupRecord { uint64_t counts[2] = {}; float ms[4] = {}; };
static Last<DedupRecord> g_dedup_last;        // published at the successful end of a de-duplicating call
enum { DD_TABLE = 0, DD_GATHER = 1, DD_DECODE = 2, DD_SCATTER = 3 };

// device-scope atomics: a slot is read only through what they return
struct DedupDeviceOps {
  __device__ uint32_t cas(uint32_t* p, uint32_t expect, uint32_t v) const { return atomicCAS(p, expect, v); }
  __device__ uint32_t min(uint32_t* p, uint32_t v) const { return atomicMin(p, v); }
};

// one lane per key
template <int KB, bool ALIGNED>
__global__ void __launch_bounds__(256) k_dedup_insert(const uint8_t* __restrict__ keys, uint32_t n, uint32_t* owner, uint32_t* first, uint32_t mask, uint32_t max_probes,
                                                      uint32_t* __restrict__ slot_of) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  slot_of[i] = dedup_insert<KB, ALIGNED>(keys, i, owner, first, mask, max_probes, DedupDeviceOps{});
}
// one lane per key: rep[i], and the representatives (rep[i] == i) compacted into list in whatever order the waves arrive, rank its inverse
// (rank is written at representatives only, and read there only).  One atomic per wave: the lanes that hold a representative are counted
// by ballot.  count[0] ends as U
__global__ void __launch_bounds__(256) k_dedup_rep(const uint32_t* __restrict__ first, const uint32_t* __restrict__ slot_of, uint32_t n, uint32_t* __restrict__ rep,
                                                   uint32_t* __restrict__ list, uint32_t* __restrict__ rank, unsigned long long* count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool is_rep = false;
  if (i < n) {
    const uint32_t r = dedup_rep(first, slot_of[i], i);
    rep[i] = r;
    is_rep = r == i;
  }
  const unsigned long long mine = __ballot(is_rep);
  if (mine == 0) return;
  const uint32_t lane = threadIdx.x & 63u;
  const int leader = __ffsll((long long)mine) - 1;
  unsigned long long base = 0;
  if ((int)lane == leader) base = atomicAdd(count, (unsigned long long)__popcll(mine));
  base = __shfl(base, leader, 64);
  if (is_rep) {
    const uint32_t r = (uint32_t)base + (uint32_t)__popcll(mine & ((1ull << lane) - 1ull));
    list[r] = i;
    rank[i] = r;
  }
}
// KB / 16 lanes per representative, 16 bytes each, into the contiguous (16-aligned) buffer.  ALIGNED: the caller's keys lie at multiples of 16
template <int KB, bool ALIGNED>
__global__ void __launch_bounds__(256) k_dedup_gather(const uint8_t* __restrict__ keys, const uint32_t* __restrict__ list, uint32_t U, uint8_t* __restrict__ out) {
  constexpr uint32_t L = KB / 16;
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (uint64_t)U * L) return;
  const uint32_t r = (uint32_t)(t / L), c = (uint32_t)(t % L);
  const uint8_t* src = keys + (size_t)list[r] * KB + 16 * c;
  uint4 v;
  if constexpr (ALIGNED) v = *reinterpret_cast<const uint4*>(src);
  else {
    uint32_t w[4];
    for (int j = 0; j < 4; j++) w[j] = (uint32_t)src[4 * j] | (uint32_t)src[4 * j + 1] << 8 | (uint32_t)src[4 * j + 2] << 16 | (uint32_t)src[4 * j + 3] << 24;
    v = make_uint4(w[0], w[1], w[2], w[3]);
  }
  reinterpret_cast<uint4*>(out)[t] = v;
}
// ROW / 16 lanes per key, 16 bytes each (12 for a G2 row of 192 B, 6 for a G1 row of 96 B): a wave writes contiguous lines.  rows / st: the
// U decoded representatives.  ALIGNED: out_xy lies at a multiple of 16 (it is a multiple of 8 in any case: rows of uint64_t)
template <int ROW, bool ALIGNED>
__global__ void __launch_bounds__(256) k_dedup_scatter(const uint64_t* __restrict__ rows, const uint8_t* __restrict__ st, const uint32_t* __restrict__ rep,
                                                       const uint32_t* __restrict__ rank, uint32_t n, uint64_t* __restrict__ out_xy, uint8_t* __restrict__ status) {
  constexpr uint32_t L = ROW / 16;
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (uint64_t)n * L) return;
  const uint32_t i = (uint32_t)(t / L), c = (uint32_t)(t % L);
  const uint32_t r = rank[rep[i]];
  const uint4 v = reinterpret_cast<const uint4*>(rows)[(size_t)r * L + c];
  if constexpr (ALIGNED) reinterpret_cast<uint4*>(out_xy)[t] = v;
  else {
    out_xy[2 * t] = (uint64_t)v.x | (uint64_t)v.y << 32;
    out_xy[2 * t + 1] = (uint64_t)v.z | (uint64_t)v.w << 32;
  }
  if (c == 0) status[i] = st[r];
}

template <int KB> static void launch_insert(bool aligned, dim3 grid, hipStream_t s, const uint8_t* keys, uint32_t n, uint32_t* owner, uint32_t* first, uint32_t mask,
                                            uint32_t probes, uint32_t* slot_of) {
  if (aligned) hipLaunchKernelGGL((k_dedup_insert<KB, true>), grid, dim3(256), 0, s, keys, n, owner, first, mask, probes, slot_of);
  else hipLaunchKernelGGL((k_dedup_insert<KB, false>), grid, dim3(256), 0, s, keys, n, owner, first, mask, probes, slot_of);
}
template <int KB> static void launch_gather(bool aligned, hipStream_t s, const uint8_t* keys, const uint32_t* list, uint32_t U, uint8_t* out) {
  const dim3 grid((unsigned)(((uint64_t)U * (KB / 16) + 255) / 256));
  if (aligned) hipLaunchKernelGGL((k_dedup_gather<KB, true>), grid, dim3(256), 0, s, keys, list, U, out);
  else hipLaunchKernelGGL((k_dedup_gather<KB, false>), grid, dim3(256), 0, s, keys, list, U, out);
}
template <int ROW> static void launch_scatter(bool aligned, hipStream_t s, const uint64_t* rows, const uint8_t* st, const uint32_t* rep, const uint32_t* rank, uint32_t n,
                                              uint64_t* out_xy, uint8_t* status) {
  const dim3 grid((unsigned)(((uint64_t)n * (ROW / 16) + 255) / 256));
  if (aligned) hipLaunchKernelGGL((k_dedup_scatter<ROW, true>), grid, dim3(256), 0, s, rows, st, rep, rank, n, out_xy, status);
  else hipLaunchKernelGGL((k_dedup_scatter<ROW, false>), grid, dim3(256), 0, s, rows, st, rep, rank, n, out_xy, status);
}

int key_dedup_set(int on, int slack_log, int max_probes) {
  if (on < -1 || on > 1 || slack_log < -1 || slack_log > DEDUP_SLACK_MAX || max_probes < 0 || max_probes > DEDUP_PROBES_MAX) return 2;
  std::lock_guard<std::mutex> lk(dedup_mu);
  g_dedup_on = on;
  g_dedup_slack = slack_log < 0 ? DEDUP_SLACK_DEFAULT : slack_log;
  g_dedup_probes = max_probes == 0 ? DEDUP_PROBES_DEFAULT : max_probes;
  return 0;
}
int key_dedup_get(int out[3]) {
  if (!out) return 2;
  std::lock_guard<std::mutex> lk(dedup_mu);
  out[0] = g_dedup_on; out[1] = g_dedup_slack; out[2] = g_dedup_probes;
  return 0;
}
bool key_dedup_use(size_t n) {
  std::lock_guard<std::mutex> lk(dedup_mu);
  return g_dedup_on == 1 || (g_dedup_on == -1 && key_dedup_pick(n));
}
int key_dedup_last(uint64_t counts[2], float ms[4]) {
  if (!counts || !ms) return 2;
  const DedupRecord r = g_dedup_last.read();
  for (int i = 0; i < 2; i++) counts[i] = r.counts[i];
  for (int i = 0; i < 4; i++) ms[i] = r.ms[i];
  return 0;
}

// in, out, status, out_rep: host pointers, or device pointers with dev set (the work then runs on the caller's stream); out_decoded: a host
// pointer in both forms.  The refusals come first and need no device
int wire_decompress_dedup(int g2, const uint8_t* in, size_t n, int check, uint64_t* out, uint8_t* status, uint32_t* out_rep, uint64_t* out_decoded, int dev, void* stream_) {
  if (n == 0) { if (out_decoded) *out_decoded = 0; return 0; }
  if (!in || !out || !status || n > 0x7fffffffu) return 2;
  if (int rc0 = api_enter()) return rc0;
  std::lock_guard<std::mutex> lk(dedup_mu);
  if (int rck = wire_consts_warm()) return rck;                       // first use on this device: the tables' upload stays outside the events
  const size_t kb = g2 ? 96 : 48, ow = g2 ? 24 : 12;
  const uint32_t n32 = (uint32_t)n, probes = (uint32_t)g_dedup_probes;
  const uint64_t S = dedup_slots(n, g_dedup_slack);
  CallScope cs((hipStream_t)stream_);
  const hipStream_t stream = cs.stream();
  uint8_t *d_in, *d_st, *d_keys, *d_ust;
  uint64_t *d_out, *d_rows;
  uint32_t *d_rep, *d_table, *d_slot_of, *d_list, *d_rank;
  unsigned long long* d_count;
  HIP_TRY(cs.in(&d_in, in, n * kb, dev), 10);
  HIP_TRY(cs.out(&d_out, out, n * ow * 8, dev), 10);
  HIP_TRY(cs.out(&d_st, status, n, dev), 10);
  HIP_TRY(cs.out(&d_rep, out_rep, n * 4, dev), 10);
  if (!d_rep) HIP_TRY(cs.alloc(&d_rep, n * 4), 10);
  HIP_TRY(cs.alloc(&d_table, S * 8), 10);                              // owner, then first
  HIP_TRY(cs.alloc(&d_slot_of, n * 4), 10);
  HIP_TRY(cs.alloc(&d_list, n * 4), 10);
  HIP_TRY(cs.alloc(&d_rank, n * 4), 10);
  HIP_TRY(cs.alloc(&d_count, 8), 10);
  EvLog log(stream);
  hipEvent_t e0 = log.open();
  HIP_TRY(hipMemsetAsync(d_table, 0xFF, S * 8, stream), 10);
  HIP_TRY(hipMemsetAsync(d_count, 0, 8, stream), 10);
  const dim3 grid((n32 + 255) / 256);
  const bool in8 = ((uintptr_t)d_in & 7) == 0, in16 = ((uintptr_t)d_in & 15) == 0, out16 = ((uintptr_t)d_out & 15) == 0;
  if (g2) launch_insert<96>(in8, grid, stream, d_in, n32, d_table, d_table + S, (uint32_t)(S - 1), probes, d_slot_of);
  else launch_insert<48>(in8, grid, stream, d_in, n32, d_table, d_table + S, (uint32_t)(S - 1), probes, d_slot_of);
  HIP_TRY(hipGetLastError(), 10);
  hipLaunchKernelGGL(k_dedup_rep, grid, dim3(256), 0, stream, d_table + S, d_slot_of, n32, d_rep, d_list, d_rank, d_count);
  HIP_TRY(hipGetLastError(), 10);
  log.close(DD_TABLE, e0);
  unsigned long long U = 0;
  HIP_TRY(hipMemcpyAsync(&U, d_count, 8, hipMemcpyDeviceToHost, stream), 10);
  HIP_TRY(hipStreamSynchronize(stream), 10);                          // the one round trip: U sizes the three launches below
  if (U == 0 || U > n) return 10;
  HIP_TRY(cs.alloc(&d_keys, (size_t)U * kb), 10);
  HIP_TRY(cs.alloc(&d_rows, (size_t)U * ow * 8), 10);
  HIP_TRY(cs.alloc(&d_ust, (size_t)U), 10);
  e0 = log.open();
  if (g2) launch_gather<96>(in16, stream, d_in, d_list, (uint32_t)U, d_keys);
  else launch_gather<48>(in16, stream, d_in, d_list, (uint32_t)U, d_keys);
  HIP_TRY(hipGetLastError(), 10);
  log.close(DD_GATHER, e0);
  e0 = log.open();
  if (int rcl = wire377_launch_decode(g2, 1, d_keys, (size_t)U, check, d_rows, d_ust, stream)) return rcl;
  log.close(DD_DECODE, e0);
  e0 = log.open();
  if (g2) launch_scatter<192>(out16, stream, d_rows, d_ust, d_rep, d_rank, n32, d_out, d_st);
  else launch_scatter<96>(out16, stream, d_rows, d_ust, d_rep, d_rank, n32, d_out, d_st);
  HIP_TRY(hipGetLastError(), 10);
  log.close(DD_SCATTER, e0);
  HIP_TRY(cs.copy_back(), 10);
  HIP_TRY(hipStreamSynchronize(stream), 10);
  DedupRecord rec;
  rec.counts[0] = n; rec.counts[1] = U;
  log.sum(rec.ms);
  g_dedup_last.note(rec);
  if (out_decoded) *out_decoded = U;
  return 0;
}
}  // namespace celo
