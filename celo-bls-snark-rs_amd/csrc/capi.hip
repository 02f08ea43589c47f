// extern "C" boundary of the gfx950 hot path (include/celo_bls_amd.h).
#include <hip/hip_runtime.h>
#include <atomic>
#include <mutex>
#include <condition_variable>
#include <vector>
#include <cstring>
#include <cstdio>
#include "../../include/celo_bls_amd.h"
#include "runtime.h"
#include "units.h"

namespace celo {
// Device binding.  HIP's current device is a per-thread setting, and this library is entered from many host threads (and
// starts its own): every entry point passes through api_enter(), which applies the calling thread's device - the one bound
// with celo_amd_use_device(), else the process default chosen by celo_amd_init() (device 0 if init was never called).
static std::atomic<int> g_device_count{-1};
static std::atomic<int> g_default_device{0};
static thread_local int t_bound_device = -1;
static int device_count() {
  int n = g_device_count.load();
  if (n >= 0) return n;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  if (n > MAX_DEVICES) n = MAX_DEVICES;
  g_device_count.store(n);
  return n;
}
int api_device() { return t_bound_device >= 0 ? t_bound_device : g_default_device.load(); }
int api_enter() {
  if (device_count() == 0) {
    fprintf(stderr, "[celo-amd] no HIP device: the MSM/pairing path has no CPU fallback\n");
    return 100;
  }
  // applied on every entry, not cached: HIP's current device is shared with whatever else runs on this thread (torch in the
  // bench and the tests), which may have switched it between two calls into the library; hipSetDevice is a TLS store when
  // nothing changes
  if (hipSetDevice(api_device()) != hipSuccess) return 102;
  return 0;
}
int api_bind_thread(int device) {
  if (device < 0 || device >= device_count()) return 101;
  t_bound_device = device;
  return 0;
}
// the `group` argument of the celo_amd_msm_* / celo_amd_selftest_* controls: 0 / 1 = BLS12-377 G1 / G2, 2 = BW6-761; anything else returns `bad`
template <class G> struct GroupTag { typedef G type; };
template <class F> static int by_group(int group, int bad, F f) {
  switch (group) {
    case 0: return f(GroupTag<G1_377>());
    case 1: return f(GroupTag<G2_377>());
    case 2: return f(GroupTag<G_761>());
    default: return bad;
  }
}
}  // namespace celo
using namespace celo;

extern "C" {
int celo_amd_init(int device) {
  const int n = device_count();
  if (n == 0) return 100;
  if (device < 0 || device >= n) return 101;
  g_default_device.store(device);      // every thread that has not bound itself to a device uses this one from now on
  t_bound_device = -1;
  return api_enter();
}
int celo_amd_use_device(int device) {
  if (device_count() == 0) return 100;
  if (int rc = api_bind_thread(device)) return rc;
  return api_enter();
}
int celo_amd_host_alloc(size_t bytes, void** out) {
  if (!out || !bytes) return 2;
  *out = nullptr;
  if (int rc = api_enter()) return rc;
  // portable: page-locked for every device of the process, not only the calling thread's
  return hipHostMalloc(out, bytes, hipHostMallocPortable) == hipSuccess ? 0 : 1;
}
int celo_amd_host_free(void* p) {
  if (!p) return 0;
  if (int rc = api_enter()) return rc;
  return hipHostFree(p) == hipSuccess ? 0 : 1;
}
int celo_amd_device_count(int* count) {
  if (!count) return 2;
  *count = device_count();
  return *count ? 0 : 100;
}
int celo_amd_device_name(char* buf, size_t buflen) {
  if (int rc = api_enter()) return rc;
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, api_device()) != hipSuccess) return 100;
  snprintf(buf, buflen, "%s", p.gcnArchName);
  return 0;
}
#define MULTI(NAME, G)                                                                                                                \
  int NAME##_multi(const int* devices, int ndev, const uint64_t* b, const uint8_t* inf, const uint64_t* s, size_t n, uint64_t* out) { \
    MsmAuxApi<G>::note_big_call();                                                                                                    \
    return MsmApi<G>::multi_host(devices, ndev, b, inf, s, n, out);                                                                   \
  }                                                                                                                                   \
  int NAME##_multi_dev(const int* devices, int ndev, const void* const* b, const void* const* inf, const void* const* s,              \
                       const size_t* n_per, uint64_t* out) {                                                                          \
    MsmAuxApi<G>::note_big_call();                                                                                                    \
    return MsmApi<G>::multi_dev(devices, ndev, b, inf, s, n_per, out);                                                                \
  }
MULTI(msm_bls12_377_g1, G1_377) MULTI(msm_bls12_377_g2, G2_377) MULTI(msm_bw6_761_g1, G_761) MULTI(msm_bw6_761_g2, G_761)
#undef MULTI
// the window partition (include/celo_bls_amd.h): host form = every shard stages the same host arrays; device form = one replica per device
#define MULTIW(NAME, G, SUB)                                                                                                          \
  int NAME##_multi_windows(const int* devices, int ndev, const uint64_t* b, const uint8_t* inf, const uint64_t* s, size_t n, uint64_t* out) { \
    if (ndev <= 0 || ndev > 64) return 2;                                                                                             \
    MsmAuxApi<G>::note_big_call();                                                                                                    \
    std::vector<const void*> pb((size_t)ndev, b), pi((size_t)ndev, inf), ps((size_t)ndev, s);                                         \
    return MsmApi<G>::multi_windows(devices, ndev, 0, pb.data(), inf ? pi.data() : nullptr, ps.data(), n, SUB, out);                  \
  }                                                                                                                                   \
  int NAME##_multi_windows_dev(const int* devices, int ndev, const void* const* b, const void* const* inf, const void* const* s,      \
                               size_t n, uint64_t* out) {                                                                             \
    MsmAuxApi<G>::note_big_call();                                                                                                    \
    return MsmApi<G>::multi_windows(devices, ndev, 1, b, inf, s, n, SUB, out);                                                        \
  }
MULTIW(msm_bls12_377_g1, G1_377, 0) MULTIW(msm_bls12_377_g1_subgroup, G1_377, 1) MULTIW(msm_bls12_377_g2, G2_377, 0) MULTIW(msm_bls12_377_g2_subgroup, G2_377, 1)
MULTIW(msm_bw6_761_g1, G_761, 0) MULTIW(msm_bw6_761_g2, G_761, 0)
#undef MULTIW
int msm_bls12_377_g1_window_shard_dev(const void* b, const void* inf, const void* s, size_t n, int subgroup, int shard, int nshards, uint64_t* o, int* bit_lo, void* st) {
  MsmAuxApi<G1_377>::note_big_call(); return MsmApi<G1_377>::window_shard(b, inf, s, n, subgroup, shard, nshards, o, bit_lo, st);
}
int msm_bls12_377_g2_window_shard_dev(const void* b, const void* inf, const void* s, size_t n, int subgroup, int shard, int nshards, uint64_t* o, int* bit_lo, void* st) {
  MsmAuxApi<G2_377>::note_big_call(); return MsmApi<G2_377>::window_shard(b, inf, s, n, subgroup, shard, nshards, o, bit_lo, st);
}
int msm_bw6_761_window_shard_dev(const void* b, const void* inf, const void* s, size_t n, int shard, int nshards, uint64_t* o, int* bit_lo, void* st) {
  MsmAuxApi<G_761>::note_big_call(); return MsmApi<G_761>::window_shard(b, inf, s, n, 0, shard, nshards, o, bit_lo, st);
}
// ---- fixed-base MSM: per-key tables (include/celo_bls_amd.h)
#define FIXED(NAME, G)                                                                                                                \
  int NAME##_precompute(const uint64_t* b, const uint8_t* inf, size_t n, int window_bits, void** handle) {                            \
    if (!handle) return 2;                                                                                                            \
    *handle = nullptr;                                                                                                                \
    return MsmApi<G>::fixed_build(b, inf, n, 0, window_bits, (FixedTable**)handle);                                                   \
  }                                                                                                                                   \
  int NAME##_precompute_dev(const void* b, const void* inf, size_t n, int window_bits, void** handle) {                               \
    if (!handle) return 2;                                                                                                            \
    *handle = nullptr;                                                                                                                \
    return MsmApi<G>::fixed_build(b, inf, n, 1, window_bits, (FixedTable**)handle);                                                   \
  }                                                                                                                                   \
  int NAME##_fixed(const void* handle, const uint64_t* s, size_t n, uint64_t* out) {                                                  \
    MsmAuxApi<G>::note_big_call(); return MsmApi<G>::fixed_run((const FixedTable*)handle, s, n, 0, out, nullptr);                     \
  }                                                                                                                                   \
  int NAME##_fixed_dev(const void* handle, const void* s, size_t n, uint64_t* out, void* st) {                                        \
    MsmAuxApi<G>::note_big_call(); return MsmApi<G>::fixed_run((const FixedTable*)handle, s, n, 1, out, st);                          \
  }
FIXED(msm_bls12_377_g1, G1_377) FIXED(msm_bls12_377_g2, G2_377) FIXED(msm_bw6_761_g1, G_761) FIXED(msm_bw6_761_g2, G_761)
#undef FIXED
// ---- Groth16 prover against a loaded key (include/celo_bls_amd.h)
int groth16_load_key_bw6_761(const uint64_t* a_query, size_t na, const uint64_t* b_g2_query, size_t nb, const uint64_t* h_query, size_t nh, const uint64_t* l_query, size_t nl,
                             const uint64_t alpha_g1[24], const uint64_t beta_g2[24], int window_bits, void** out_key) {
  if (!out_key) return 2;
  *out_key = nullptr;
  return groth16_key_load(0, a_query, na, b_g2_query, nb, h_query, nh, l_query, nl, alpha_g1, beta_g2, window_bits, (ProvingKey**)out_key);
}
int groth16_load_key_bls12_377(const uint64_t* a_query, size_t na, const uint64_t* b_g2_query, size_t nb, const uint64_t* h_query, size_t nh, const uint64_t* l_query, size_t nl,
                               const uint64_t alpha_g1[12], const uint64_t beta_g2[24], int window_bits, void** out_key) {
  if (!out_key) return 2;
  *out_key = nullptr;
  return groth16_key_load(1, a_query, na, b_g2_query, nb, h_query, nh, l_query, nl, alpha_g1, beta_g2, window_bits, (ProvingKey**)out_key);
}
int groth16_prove_with_key(const void* key, const uint64_t* assignment, size_t n_assignment, size_t n_aux, const uint64_t* h, size_t n_h, uint64_t* out_a, uint64_t* out_b,
                           uint64_t* out_c) {
  return groth16_prove_keyed((const ProvingKey*)key, assignment, n_assignment, n_aux, h, n_h, out_a, out_b, out_c);
}
int groth16_free_key(void* key) { if (!key) return 2; groth16_key_free((ProvingKey*)key); return 0; }
int celo_amd_msm_fixed_release(void* handle) { return fixed_table_release((FixedTable*)handle); }
int celo_amd_msm_fixed_info(const void* handle, size_t* n, int* window_bits, int* windows, size_t* table_bytes, float* build_ms) {
  return fixed_table_info((const FixedTable*)handle, n, window_bits, windows, table_bytes, build_ms);
}
int msm_bls12_377_g1_join_windows(const uint64_t* xyzz, const int* bit_lo, int nshards, uint64_t* out) { return MsmApi<G1_377>::join_windows(xyzz, bit_lo, nshards, out); }
int msm_bls12_377_g2_join_windows(const uint64_t* xyzz, const int* bit_lo, int nshards, uint64_t* out) { return MsmApi<G2_377>::join_windows(xyzz, bit_lo, nshards, out); }
int msm_bw6_761_join_windows(const uint64_t* xyzz, const int* bit_lo, int nshards, uint64_t* out) { return MsmApi<G_761>::join_windows(xyzz, bit_lo, nshards, out); }
int msm_bls12_377_g1(const uint64_t* b, const uint8_t* inf, const uint64_t* s, size_t n, uint64_t* out) { MsmAuxApi<G1_377>::note_big_call(); return MsmApi<G1_377>::host(b, inf, s, n, 0, out); }
int msm_bls12_377_g1_subgroup(const uint64_t* b, const uint8_t* inf, const uint64_t* s, size_t n, uint64_t* out) { MsmAuxApi<G1_377>::note_big_call(); return MsmApi<G1_377>::host(b, inf, s, n, 1, out); }
int msm_bls12_377_g1_subgroup_dev(const void* b, const void* inf, const void* s, size_t n, uint64_t* out, void* st) { MsmAuxApi<G1_377>::note_big_call(); return MsmApi<G1_377>::dev(b, inf, s, n, 1, out, st); }
int msm_bls12_377_g2(const uint64_t* b, const uint8_t* inf, const uint64_t* s, size_t n, uint64_t* out) { MsmAuxApi<G2_377>::note_big_call(); return MsmApi<G2_377>::host(b, inf, s, n, 0, out); }
int msm_bls12_377_g2_subgroup(const uint64_t* b, const uint8_t* inf, const uint64_t* s, size_t n, uint64_t* out) { MsmAuxApi<G2_377>::note_big_call(); return MsmApi<G2_377>::host(b, inf, s, n, 1, out); }
int msm_bls12_377_g2_subgroup_dev(const void* b, const void* inf, const void* s, size_t n, uint64_t* out, void* st) { MsmAuxApi<G2_377>::note_big_call(); return MsmApi<G2_377>::dev(b, inf, s, n, 1, out, st); }
int msm_bw6_761_g1(const uint64_t* b, const uint8_t* inf, const uint64_t* s, size_t n, uint64_t* out) { MsmAuxApi<G_761>::note_big_call(); return MsmApi<G_761>::host(b, inf, s, n, 0, out); }
int msm_bw6_761_g2(const uint64_t* b, const uint8_t* inf, const uint64_t* s, size_t n, uint64_t* out) { MsmAuxApi<G_761>::note_big_call(); return MsmApi<G_761>::host(b, inf, s, n, 0, out); }
int msm_bls12_377_g1_dev(const void* b, const void* inf, const void* s, size_t n, uint64_t* out, void* st) { MsmAuxApi<G1_377>::note_big_call(); return MsmApi<G1_377>::dev(b, inf, s, n, 0, out, st); }
int msm_bls12_377_g2_dev(const void* b, const void* inf, const void* s, size_t n, uint64_t* out, void* st) { MsmAuxApi<G2_377>::note_big_call(); return MsmApi<G2_377>::dev(b, inf, s, n, 0, out, st); }
int msm_bw6_761_g1_dev(const void* b, const void* inf, const void* s, size_t n, uint64_t* out, void* st) { MsmAuxApi<G_761>::note_big_call(); return MsmApi<G_761>::dev(b, inf, s, n, 0, out, st); }
int msm_bw6_761_g2_dev(const void* b, const void* inf, const void* s, size_t n, uint64_t* out, void* st) { MsmAuxApi<G_761>::note_big_call(); return MsmApi<G_761>::dev(b, inf, s, n, 0, out, st); }
int msm_batch_bls12_377_g1(const uint64_t* b, const uint8_t* inf, const uint64_t* s, const uint32_t* off, size_t m, uint64_t* out) { return MsmAuxApi<G1_377>::batch_host(b, inf, s, off, m, 0, out); }
int msm_batch_bls12_377_g2(const uint64_t* b, const uint8_t* inf, const uint64_t* s, const uint32_t* off, size_t m, uint64_t* out) { return MsmAuxApi<G2_377>::batch_host(b, inf, s, off, m, 0, out); }
int msm_batch_bls12_377_g2_subgroup(const uint64_t* b, const uint8_t* inf, const uint64_t* s, const uint32_t* off, size_t m, uint64_t* out) { return MsmAuxApi<G2_377>::batch_host(b, inf, s, off, m, 1, out); }
int msm_batch_bw6_761_g1(const uint64_t* b, const uint8_t* inf, const uint64_t* s, const uint32_t* off, size_t m, uint64_t* out) { return MsmAuxApi<G_761>::batch_host(b, inf, s, off, m, 0, out); }
int msm_batch_bw6_761_g2(const uint64_t* b, const uint8_t* inf, const uint64_t* s, const uint32_t* off, size_t m, uint64_t* out) { return MsmAuxApi<G_761>::batch_host(b, inf, s, off, m, 0, out); }
// Single-product checks from concurrent host threads are COMBINED: bls-snark-sys is synchronous and re-entrant and its callers
// verify from many threads ("Threading"); one product keeps one lane group of the GPU busy for ~11 ms, so
// serialising callers behind a mutex would cap the library at ~90 verifications/s.  The first caller to arrive becomes the
// leader of a round: it takes the queue of pending products, runs them as ONE batched launch and publishes the verdicts; the
// others sleep on a condition variable, and one of those still waiting leads the next round.
namespace {
struct ProductJob {
  const uint64_t* g1; const uint8_t* inf1; const uint64_t* g2; const uint8_t* inf2; size_t k;
  int rc = 0; int is_one = 0; bool done = false;
};
// (static: an unnamed namespace inside the extern "C" block does not keep these out of the dynamic symbol table - VERDICT r3)
static std::mutex q_mu;
static std::condition_variable q_cv;
static std::vector<ProductJob*> q_pending;
static bool q_leader = false;

static void run_products(std::vector<ProductJob*>& jobs) {
  if (jobs.size() == 1) {
    ProductJob* j = jobs[0];
    uint32_t offs[2] = {0, (uint32_t)j->k};
    uint8_t one = 0;
    j->rc = pairing_run_377(j->g1, j->inf1, j->g2, j->inf2, offs, 1, &one, nullptr, 0);
    j->is_one = one;
    return;
  }
  size_t tot = 0;
  for (ProductJob* j : jobs) tot += j->k;
  std::vector<uint64_t> g1(tot * 12), g2(tot * 24);
  std::vector<uint8_t> i1(tot, 0), i2(tot, 0), one(jobs.size(), 0);
  std::vector<uint32_t> offs(jobs.size() + 1, 0);
  size_t at = 0;
  for (size_t p = 0; p < jobs.size(); p++) {
    ProductJob* j = jobs[p];
    memcpy(&g1[at * 12], j->g1, j->k * 96);
    memcpy(&g2[at * 24], j->g2, j->k * 192);
    if (j->inf1) memcpy(&i1[at], j->inf1, j->k);
    if (j->inf2) memcpy(&i2[at], j->inf2, j->k);
    at += j->k;
    offs[p + 1] = (uint32_t)at;
  }
  const int rc = pairing_run_377(g1.data(), i1.data(), g2.data(), i2.data(), offs.data(), jobs.size(), one.data(), nullptr, 0);
  for (size_t p = 0; p < jobs.size(); p++) { jobs[p]->rc = rc; jobs[p]->is_one = one[p]; }
}
}  // namespace

int pairing_product_is_one_bls12_377(const uint64_t* g1, const uint8_t* inf1, const uint64_t* g2, const uint8_t* inf2, size_t k, int* is_one) {
  ProductJob job{g1, inf1, g2, inf2, k};
  std::unique_lock<std::mutex> lk(q_mu);
  q_pending.push_back(&job);
  while (!job.done) {
    if (q_leader) { q_cv.wait(lk); continue; }
    // lead ONE round: everything pending right now (this job included) becomes one launch; whoever is still waiting when
    // it is over leads the next round, so no caller serves the queue for longer than its own verdict takes
    q_leader = true;
    std::vector<ProductJob*> batch;
    batch.swap(q_pending);
    lk.unlock();
    try { run_products(batch); }
    catch (...) { for (ProductJob* j : batch) j->rc = 103; }     // e.g. std::bad_alloc while staging: every job of the round fails
    lk.lock();
    for (ProductJob* j : batch) j->done = true;
    q_leader = false;
    q_cv.notify_all();
  }
  lk.unlock();
  if (job.rc == 0 && is_one) *is_one = job.is_one;
  return job.rc;
}
int pairing_product_is_one_batch_bls12_377(const uint64_t* g1, const uint8_t* inf1, const uint64_t* g2, const uint8_t* inf2,
                                           const uint32_t* offsets, size_t m, uint8_t* is_one) {
  return pairing_run_377(g1, inf1, g2, inf2, offsets, m, is_one, nullptr, 0);
}
int celo_amd_pairing_gt_bls12_377(const uint64_t* g1, const uint8_t* inf1, const uint64_t* g2, const uint8_t* inf2, const uint32_t* offsets,
                                  size_t m, int miller_only, uint64_t* gt72) {
  return pairing_run_377(g1, inf1, g2, inf2, offsets, m, nullptr, gt72, miller_only ? 1 : 0);
}
int pairing_product_is_one_bw6_761(const uint64_t* g1, const uint8_t* inf1, const uint64_t* g2, const uint8_t* inf2, size_t k, int* is_one) {
  uint32_t offs[2] = {0, (uint32_t)k};
  uint8_t one = 0;
  int rc = pairing_run_761(g1, inf1, g2, inf2, offs, 1, &one, nullptr, 0);
  if (rc == 0 && is_one) *is_one = one;
  return rc;
}
int pairing_product_is_one_batch_bw6_761(const uint64_t* g1, const uint8_t* inf1, const uint64_t* g2, const uint8_t* inf2,
                                         const uint32_t* offsets, size_t m, uint8_t* is_one) {
  return pairing_run_761(g1, inf1, g2, inf2, offsets, m, is_one, nullptr, 0);
}
int celo_amd_pairing_gt_bw6_761(const uint64_t* g1, const uint8_t* inf1, const uint64_t* g2, const uint8_t* inf2, const uint32_t* offsets,
                                size_t m, int miller_only, uint64_t* gt72) {
  return pairing_run_761(g1, inf1, g2, inf2, offsets, m, nullptr, gt72, miller_only ? 1 : 0);
}
int batch_verify_bls12_377(const uint64_t* pk_xy, const uint8_t* pk_inf, const uint64_t* sig_xy, const uint8_t* sig_inf, const uint64_t* exponents,
                           const uint32_t* offsets, const uint64_t* hash_xy, const uint8_t* hash_inf, const uint64_t neg_g2_xy[24], size_t m, uint8_t* out_ok) {
  return batch_verify_377_run(pk_xy, pk_inf, sig_xy, sig_inf, exponents, 0, offsets, hash_xy, hash_inf, neg_g2_xy, m, out_ok);
}
int batch_verify_bls12_377_dev(const void* d_pk_xy, const void* d_pk_inf, const void* d_sig_xy, const void* d_sig_inf, const void* d_exponents,
                               const uint32_t* offsets, const void* d_hash_xy, const void* d_hash_inf, const uint64_t neg_g2_xy[24], size_t m, uint8_t* out_ok) {
  return batch_verify_377_run(d_pk_xy, d_pk_inf, d_sig_xy, d_sig_inf, d_exponents, 1, offsets, d_hash_xy, d_hash_inf, neg_g2_xy, m, out_ok);
}
int celo_amd_draw_batch_exponents(const uint32_t key[8], const uint32_t* offsets, size_t m, uint64_t* out) { return draw_exponents_run(key, offsets, m, out); }
int celo_amd_pairing_last_timings(float ms[4]) { return pairing_timings_377(ms); }
int ntt_bw6_761_fr(uint64_t* data, unsigned log_n, const uint64_t omega[6], const uint64_t* coset, int coset_after, const uint64_t* scale) {
  return ntt_run<Fr761>(data, log_n, omega, coset, coset_after, scale, 0, nullptr);
}
int ntt_bw6_761_fr_dev(uint64_t* d_data, unsigned log_n, const uint64_t omega[6], const uint64_t* coset, int coset_after, const uint64_t* scale,
                       void* hip_stream) {
  return ntt_run<Fr761>(d_data, log_n, omega, coset, coset_after, scale, 1, hip_stream);
}
int celo_amd_ntt_last_timings(float ms[4], int* passes) { return ntt_timings(ms, passes); }
int groth16_witness_map_bw6_761(uint64_t* a, uint64_t* b, uint64_t* c, unsigned log_n, const uint64_t omega[6], const uint64_t omega_inv[6], const uint64_t coset[6],
                                const uint64_t coset_inv[6], const uint64_t size_inv[6], const uint64_t vanishing_inv[6], int out_canonical) {
  return witness_map_run<Fr761>(a, b, c, log_n, omega, omega_inv, coset, coset_inv, size_inv, vanishing_inv, out_canonical, 0, nullptr);
}
int groth16_witness_map_bw6_761_dev(uint64_t* d_a, uint64_t* d_b, uint64_t* d_c, unsigned log_n, const uint64_t omega[6], const uint64_t omega_inv[6],
                                    const uint64_t coset[6], const uint64_t coset_inv[6], const uint64_t size_inv[6], const uint64_t vanishing_inv[6],
                                    int out_canonical, void* hip_stream) {
  return witness_map_run<Fr761>(d_a, d_b, d_c, log_n, omega, omega_inv, coset, coset_inv, size_inv, vanishing_inv, out_canonical, 1, hip_stream);
}
int groth16_prove_bw6_761(const uint64_t* a_query, size_t na, const uint64_t* b_g2_query, size_t nb, const uint64_t* h_query, size_t nh, const uint64_t* l_query,
                          size_t nl, const uint64_t alpha_g1[24], const uint64_t beta_g2[24], const uint64_t* assignment, size_t n_assignment, size_t n_aux,
                          const uint64_t* h, size_t n_h, uint64_t out_a[36], uint64_t out_b[36], uint64_t out_c[36]) {
  MsmAuxApi<G_761>::note_big_call();
  return groth16_prove_761_run(a_query, na, b_g2_query, nb, h_query, nh, l_query, nl, alpha_g1, beta_g2, assignment, n_assignment, n_aux, h, n_h, out_a, out_b, out_c);
}
int ntt_bls12_377_fr(uint64_t* data, unsigned log_n, const uint64_t omega[4], const uint64_t* coset, int coset_after, const uint64_t* scale) {
  return ntt_run<Fr377>(data, log_n, omega, coset, coset_after, scale, 0, nullptr);
}
int ntt_bls12_377_fr_dev(uint64_t* d_data, unsigned log_n, const uint64_t omega[4], const uint64_t* coset, int coset_after, const uint64_t* scale,
                         void* hip_stream) {
  return ntt_run<Fr377>(d_data, log_n, omega, coset, coset_after, scale, 1, hip_stream);
}
int groth16_witness_map_bls12_377(uint64_t* a, uint64_t* b, uint64_t* c, unsigned log_n, const uint64_t omega[4], const uint64_t omega_inv[4], const uint64_t coset[4],
                                  const uint64_t coset_inv[4], const uint64_t size_inv[4], const uint64_t vanishing_inv[4], int out_canonical) {
  return witness_map_run<Fr377>(a, b, c, log_n, omega, omega_inv, coset, coset_inv, size_inv, vanishing_inv, out_canonical, 0, nullptr);
}
int groth16_witness_map_bls12_377_dev(uint64_t* d_a, uint64_t* d_b, uint64_t* d_c, unsigned log_n, const uint64_t omega[4], const uint64_t omega_inv[4],
                                      const uint64_t coset[4], const uint64_t coset_inv[4], const uint64_t size_inv[4], const uint64_t vanishing_inv[4],
                                      int out_canonical, void* hip_stream) {
  return witness_map_run<Fr377>(d_a, d_b, d_c, log_n, omega, omega_inv, coset, coset_inv, size_inv, vanishing_inv, out_canonical, 1, hip_stream);
}
int groth16_prove_bls12_377(const uint64_t* a_query, size_t na, const uint64_t* b_g2_query, size_t nb, const uint64_t* h_query, size_t nh, const uint64_t* l_query,
                            size_t nl, const uint64_t alpha_g1[12], const uint64_t beta_g2[24], const uint64_t* assignment, size_t n_assignment, size_t n_aux,
                            const uint64_t* h, size_t n_h, uint64_t out_a[18], uint64_t out_b[36], uint64_t out_c[18]) {
  MsmAuxApi<G1_377>::note_big_call();
  MsmAuxApi<G2_377>::note_big_call();
  return groth16_prove_377_run(a_query, na, b_g2_query, nb, h_query, nh, l_query, nl, alpha_g1, beta_g2, assignment, n_assignment, n_aux, h, n_h, out_a, out_b, out_c);
}
int decompress_bls12_377_g1(const uint8_t* in, size_t n, int check_subgroup, uint64_t* out_xy, uint8_t* status) {
  return wire_decompress(0, in, n, check_subgroup, out_xy, status, 0, nullptr);
}
int decompress_bls12_377_g2(const uint8_t* in, size_t n, int check_subgroup, uint64_t* out_xy, uint8_t* status) {
  return wire_decompress(1, in, n, check_subgroup, out_xy, status, 0, nullptr);
}
int decompress_bls12_377_g1_dev(const uint8_t* d_in, size_t n, int check_subgroup, uint64_t* d_out_xy, uint8_t* d_status, void* hip_stream) {
  return wire_decompress(0, d_in, n, check_subgroup, d_out_xy, d_status, 1, hip_stream);
}
int decompress_bls12_377_g2_dev(const uint8_t* d_in, size_t n, int check_subgroup, uint64_t* d_out_xy, uint8_t* d_status, void* hip_stream) {
  return wire_decompress(1, d_in, n, check_subgroup, d_out_xy, d_status, 1, hip_stream);
}
// ---- the same keys decoded once per distinct byte string (unit_dedup.hip)
int decompress_bls12_377_g1_dedup(const uint8_t* in, size_t n, int check_subgroup, uint64_t* out_xy, uint8_t* status, uint32_t* out_rep, uint64_t* out_decoded) {
  return wire_decompress_dedup(0, in, n, check_subgroup, out_xy, status, out_rep, out_decoded, 0, nullptr);
}
int decompress_bls12_377_g2_dedup(const uint8_t* in, size_t n, int check_subgroup, uint64_t* out_xy, uint8_t* status, uint32_t* out_rep, uint64_t* out_decoded) {
  return wire_decompress_dedup(1, in, n, check_subgroup, out_xy, status, out_rep, out_decoded, 0, nullptr);
}
int decompress_bls12_377_g1_dedup_dev(const uint8_t* d_in, size_t n, int check_subgroup, uint64_t* d_out_xy, uint8_t* d_status, uint32_t* d_out_rep, uint64_t* out_decoded,
                                      void* hip_stream) {
  return wire_decompress_dedup(0, d_in, n, check_subgroup, d_out_xy, d_status, d_out_rep, out_decoded, 1, hip_stream);
}
int decompress_bls12_377_g2_dedup_dev(const uint8_t* d_in, size_t n, int check_subgroup, uint64_t* d_out_xy, uint8_t* d_status, uint32_t* d_out_rep, uint64_t* out_decoded,
                                      void* hip_stream) {
  return wire_decompress_dedup(1, d_in, n, check_subgroup, d_out_xy, d_status, d_out_rep, out_decoded, 1, hip_stream);
}
int celo_amd_key_dedup_set(int on, int slack_log, int max_probes) { return key_dedup_set(on, slack_log, max_probes); }
int celo_amd_key_dedup_get(int out[3]) { return key_dedup_get(out); }
int celo_amd_key_dedup_last(uint64_t counts[2], float ms[4]) { return key_dedup_last(counts, ms); }
int decompress_bw6_761_g1(const uint8_t* in, size_t n, int check_subgroup, uint64_t* out_xy, uint8_t* status) {
  return wire761_decode(0, 1, in, n, check_subgroup, out_xy, status, 0, nullptr);
}
int decompress_bw6_761_g2(const uint8_t* in, size_t n, int check_subgroup, uint64_t* out_xy, uint8_t* status) {
  return wire761_decode(1, 1, in, n, check_subgroup, out_xy, status, 0, nullptr);
}
int decompress_bw6_761_g1_dev(const uint8_t* d_in, size_t n, int check_subgroup, uint64_t* d_out_xy, uint8_t* d_status, void* hip_stream) {
  return wire761_decode(0, 1, d_in, n, check_subgroup, d_out_xy, d_status, 1, hip_stream);
}
int decompress_bw6_761_g2_dev(const uint8_t* d_in, size_t n, int check_subgroup, uint64_t* d_out_xy, uint8_t* d_status, void* hip_stream) {
  return wire761_decode(1, 1, d_in, n, check_subgroup, d_out_xy, d_status, 1, hip_stream);
}
int decode_uncompressed_bw6_761_g1(const uint8_t* in, size_t n, int check, uint64_t* out_xy, uint8_t* status) {
  return wire761_decode(0, 0, in, n, check, out_xy, status, 0, nullptr);
}
int decode_uncompressed_bw6_761_g2(const uint8_t* in, size_t n, int check, uint64_t* out_xy, uint8_t* status) {
  return wire761_decode(1, 0, in, n, check, out_xy, status, 0, nullptr);
}
int decode_uncompressed_bls12_377_g1(const uint8_t* in, size_t n, int check, uint64_t* out_xy, uint8_t* status) {
  return wire377_decode(0, 0, in, n, check, out_xy, status, 0, nullptr);
}
int decode_uncompressed_bls12_377_g2(const uint8_t* in, size_t n, int check, uint64_t* out_xy, uint8_t* status) {
  return wire377_decode(1, 0, in, n, check, out_xy, status, 0, nullptr);
}
int decode_uncompressed_bls12_377_g1_dev(const uint8_t* d_in, size_t n, int check, uint64_t* d_out_xy, uint8_t* d_status, void* hip_stream) {
  return wire377_decode(0, 0, d_in, n, check, d_out_xy, d_status, 1, hip_stream);
}
int decode_uncompressed_bls12_377_g2_dev(const uint8_t* d_in, size_t n, int check, uint64_t* d_out_xy, uint8_t* d_status, void* hip_stream) {
  return wire377_decode(1, 0, d_in, n, check, d_out_xy, d_status, 1, hip_stream);
}
// ---- bulk validation of affine rows (unit_check.hip)
int check_points_bls12_377_g1(const uint64_t* xy, const uint8_t* inf, size_t n, int level, uint8_t* out_status, uint64_t* out_first_bad) {
  return check_points(0, xy, inf, n, level, out_status, out_first_bad, 0, nullptr);
}
int check_points_bls12_377_g2(const uint64_t* xy, const uint8_t* inf, size_t n, int level, uint8_t* out_status, uint64_t* out_first_bad) {
  return check_points(1, xy, inf, n, level, out_status, out_first_bad, 0, nullptr);
}
int check_points_bw6_761_g1(const uint64_t* xy, const uint8_t* inf, size_t n, int level, uint8_t* out_status, uint64_t* out_first_bad) {
  return check_points(2, xy, inf, n, level, out_status, out_first_bad, 0, nullptr);
}
int check_points_bw6_761_g2(const uint64_t* xy, const uint8_t* inf, size_t n, int level, uint8_t* out_status, uint64_t* out_first_bad) {
  return check_points(3, xy, inf, n, level, out_status, out_first_bad, 0, nullptr);
}
int check_points_bls12_377_g1_dev(const uint64_t* d_xy, const uint8_t* d_inf, size_t n, int level, uint8_t* d_out_status, uint64_t* out_first_bad, void* hip_stream) {
  return check_points(0, d_xy, d_inf, n, level, d_out_status, out_first_bad, 1, hip_stream);
}
int check_points_bls12_377_g2_dev(const uint64_t* d_xy, const uint8_t* d_inf, size_t n, int level, uint8_t* d_out_status, uint64_t* out_first_bad, void* hip_stream) {
  return check_points(1, d_xy, d_inf, n, level, d_out_status, out_first_bad, 1, hip_stream);
}
int check_points_bw6_761_g1_dev(const uint64_t* d_xy, const uint8_t* d_inf, size_t n, int level, uint8_t* d_out_status, uint64_t* out_first_bad, void* hip_stream) {
  return check_points(2, d_xy, d_inf, n, level, d_out_status, out_first_bad, 1, hip_stream);
}
int check_points_bw6_761_g2_dev(const uint64_t* d_xy, const uint8_t* d_inf, size_t n, int level, uint8_t* d_out_status, uint64_t* out_first_bad, void* hip_stream) {
  return check_points(3, d_xy, d_inf, n, level, d_out_status, out_first_bad, 1, hip_stream);
}
int celo_amd_check_points_last_ms(float* ms) {
  if (!ms) return 2;
  *ms = check_points_last_ms();
  return 0;
}
int celo_amd_wire761_set_subgroup_test(int form) { return wire761_set_subgroup_test(form); }
int groth16_key_layout_bw6_761(const uint8_t* bytes, size_t len, int form, uint64_t out[16]) { return wire_key_layout(0, bytes, len, form, out); }
int groth16_key_layout_bls12_377(const uint8_t* bytes, size_t len, int form, uint64_t out[16]) { return wire_key_layout(1, bytes, len, form, out); }
int groth16_load_key_bw6_761_serialized(const uint8_t* bytes, size_t len, int form, int window_bits, void** out_key, uint64_t* first_bad_point) {
  if (!out_key) return 2;
  *out_key = nullptr;
  return wire_key_load(0, bytes, len, form, window_bits, (ProvingKey**)out_key, first_bad_point);
}
int groth16_load_key_bls12_377_serialized(const uint8_t* bytes, size_t len, int form, int window_bits, void** out_key, uint64_t* first_bad_point) {
  if (!out_key) return 2;
  *out_key = nullptr;
  return wire_key_load(1, bytes, len, form, window_bits, (ProvingKey**)out_key, first_bad_point);
}
// ---- Groth16 verification of many proofs under one key (unit_groth16_verify.hip, unit_groth16_verify377.hip)
int groth16_vk_load_bw6_761(const uint64_t alpha_g1[24], const uint64_t beta_g2[24], const uint64_t gamma_g2[24], const uint64_t delta_g2[24], const uint64_t* gamma_abc_g1,
                            size_t n_abc, void** out_vk) {
  return G16Api<G16Bw6>::vk_load(alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1, n_abc, (VerifyingKey**)out_vk);
}
int groth16_vk_load_bw6_761_serialized(const uint8_t* bytes, size_t len, void** out_vk) { return G16Api<G16Bw6>::vk_load_serialized(bytes, len, (VerifyingKey**)out_vk); }
int groth16_vk_free(void* vk) { return groth16_vk_release((VerifyingKey*)vk); }
int groth16_verify_batch_bw6_761(const void* vk, const uint64_t* a_xy, const uint8_t* a_inf, const uint64_t* b_xy, const uint8_t* b_inf, const uint64_t* c_xy,
                                 const uint8_t* c_inf, const uint64_t* inputs, size_t m, int mode, const uint32_t* key, uint8_t* out_ok) {
  if (m && (!a_xy || !b_xy || !c_xy)) return 2;
  return G16Api<G16Bw6>::verify((const VerifyingKey*)vk, a_xy, a_inf, b_xy, b_inf, c_xy, c_inf, nullptr, inputs, m, mode, key, out_ok);
}
int groth16_verify_batch_bw6_761_serialized(const void* vk, const uint8_t* proofs, const uint64_t* inputs, size_t m, int mode, const uint32_t* key, uint8_t* out_ok) {
  if (m && !proofs) return 2;
  return G16Api<G16Bw6>::verify((const VerifyingKey*)vk, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, proofs, inputs, m, mode, key, out_ok);
}
int groth16_vk_load_bls12_377(const uint64_t alpha_g1[12], const uint64_t beta_g2[24], const uint64_t gamma_g2[24], const uint64_t delta_g2[24], const uint64_t* gamma_abc_g1,
                              size_t n_abc, void** out_vk) {
  return G16Api<G16Bls>::vk_load(alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1, n_abc, (VerifyingKey**)out_vk);
}
int groth16_vk_load_bls12_377_serialized(const uint8_t* bytes, size_t len, void** out_vk) { return G16Api<G16Bls>::vk_load_serialized(bytes, len, (VerifyingKey**)out_vk); }
int groth16_verify_batch_bls12_377(const void* vk, const uint64_t* a_xy, const uint8_t* a_inf, const uint64_t* b_xy, const uint8_t* b_inf, const uint64_t* c_xy,
                                   const uint8_t* c_inf, const uint64_t* inputs, size_t m, int mode, const uint32_t* key, uint8_t* out_ok) {
  if (m && (!a_xy || !b_xy || !c_xy)) return 2;
  return G16Api<G16Bls>::verify((const VerifyingKey*)vk, a_xy, a_inf, b_xy, b_inf, c_xy, c_inf, nullptr, inputs, m, mode, key, out_ok);
}
int groth16_verify_batch_bls12_377_serialized(const void* vk, const uint8_t* proofs, const uint64_t* inputs, size_t m, int mode, const uint32_t* key, uint8_t* out_ok) {
  if (m && !proofs) return 2;
  return G16Api<G16Bls>::verify((const VerifyingKey*)vk, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, proofs, inputs, m, mode, key, out_ok);
}
// the wide loaders: up to VK_MAX_INPUTS_WIDE public inputs where the two above stop at VK_MAX_INPUTS (units.h); the same handle type
int groth16_vk_load_bls12_377_wide(const uint64_t alpha_g1[12], const uint64_t beta_g2[24], const uint64_t gamma_g2[24], const uint64_t delta_g2[24],
                                   const uint64_t* gamma_abc_g1, size_t n_abc, void** out_vk) {
  return G16Api<G16Bls>::vk_load(alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1, n_abc, (VerifyingKey**)out_vk, VK_MAX_INPUTS_WIDE);
}
int groth16_vk_load_bls12_377_wide_serialized(const uint8_t* bytes, size_t len, void** out_vk) {
  return G16Api<G16Bls>::vk_load_serialized(bytes, len, (VerifyingKey**)out_vk, VK_MAX_INPUTS_WIDE);
}
int celo_amd_groth16_set_input_lanes(int lanes) { return groth16_set_input_lanes(lanes); }
int celo_amd_groth16_inputs_last(int* lanes, int* n_inputs) { return groth16_inputs_last(lanes, n_inputs); }
int celo_amd_groth16_draw_exponents(const uint32_t key[8], size_t m, uint64_t* out) { return groth16_draw_exponents_run(key, m, out); }
int celo_amd_groth16_verify_last(int* path, int* window_bits, float ms[8]) { return groth16_verify_last(path, window_bits, ms); }
int celo_amd_wire761_last_timings(float ms[4]) { if (!ms) return 2; wire761_last_timings(ms); return 0; }
// ---- the encoders (unit_wire_encode.hip): group 0 / 1 = BLS12-377 G1 / G2, 2 = BW6-761
int compress_bls12_377_g1(const uint64_t* rows, const uint8_t* inf, size_t n, uint8_t* out, uint8_t* status) { return wire_encode(0, 1, rows, inf, n, out, status, 0, nullptr); }
int compress_bls12_377_g2(const uint64_t* rows, const uint8_t* inf, size_t n, uint8_t* out, uint8_t* status) { return wire_encode(1, 1, rows, inf, n, out, status, 0, nullptr); }
int compress_bw6_761(const uint64_t* rows, const uint8_t* inf, size_t n, uint8_t* out, uint8_t* status) { return wire_encode(2, 1, rows, inf, n, out, status, 0, nullptr); }
int encode_uncompressed_bls12_377_g1(const uint64_t* rows, const uint8_t* inf, size_t n, uint8_t* out, uint8_t* status) { return wire_encode(0, 0, rows, inf, n, out, status, 0, nullptr); }
int encode_uncompressed_bls12_377_g2(const uint64_t* rows, const uint8_t* inf, size_t n, uint8_t* out, uint8_t* status) { return wire_encode(1, 0, rows, inf, n, out, status, 0, nullptr); }
int encode_uncompressed_bw6_761(const uint64_t* rows, const uint8_t* inf, size_t n, uint8_t* out, uint8_t* status) { return wire_encode(2, 0, rows, inf, n, out, status, 0, nullptr); }
int compress_bls12_377_g1_dev(const uint64_t* d_rows, const uint8_t* d_inf, size_t n, uint8_t* d_out, uint8_t* d_status, void* hip_stream) {
  return wire_encode(0, 1, d_rows, d_inf, n, d_out, d_status, 1, hip_stream);
}
int compress_bls12_377_g2_dev(const uint64_t* d_rows, const uint8_t* d_inf, size_t n, uint8_t* d_out, uint8_t* d_status, void* hip_stream) {
  return wire_encode(1, 1, d_rows, d_inf, n, d_out, d_status, 1, hip_stream);
}
int compress_bw6_761_dev(const uint64_t* d_rows, const uint8_t* d_inf, size_t n, uint8_t* d_out, uint8_t* d_status, void* hip_stream) {
  return wire_encode(2, 1, d_rows, d_inf, n, d_out, d_status, 1, hip_stream);
}
int encode_uncompressed_bls12_377_g1_dev(const uint64_t* d_rows, const uint8_t* d_inf, size_t n, uint8_t* d_out, uint8_t* d_status, void* hip_stream) {
  return wire_encode(0, 0, d_rows, d_inf, n, d_out, d_status, 1, hip_stream);
}
int encode_uncompressed_bls12_377_g2_dev(const uint64_t* d_rows, const uint8_t* d_inf, size_t n, uint8_t* d_out, uint8_t* d_status, void* hip_stream) {
  return wire_encode(1, 0, d_rows, d_inf, n, d_out, d_status, 1, hip_stream);
}
int encode_uncompressed_bw6_761_dev(const uint64_t* d_rows, const uint8_t* d_inf, size_t n, uint8_t* d_out, uint8_t* d_status, void* hip_stream) {
  return wire_encode(2, 0, d_rows, d_inf, n, d_out, d_status, 1, hip_stream);
}
int groth16_serialized_key_size_bw6_761(size_t n_inputs, size_t n_vars, size_t n_h, int form, int vk_only, uint64_t* len) {
  return wire_key_size(0, n_inputs, n_vars, n_h, form, vk_only, len);
}
int groth16_serialized_key_size_bls12_377(size_t n_inputs, size_t n_vars, size_t n_h, int form, int vk_only, uint64_t* len) {
  return wire_key_size(1, n_inputs, n_vars, n_h, form, vk_only, len);
}
int groth16_serialize_key_bw6_761(const uint64_t* vk, size_t n_inputs, const uint64_t* rows, size_t n_vars, size_t n_h, int form, uint8_t* out, size_t cap, uint64_t* out_len,
                                  uint64_t* first_bad_point) {
  return wire_key_serialize(0, vk, n_inputs, rows, n_vars, n_h, form, out, cap, out_len, first_bad_point);
}
int groth16_serialize_key_bls12_377(const uint64_t* vk, size_t n_inputs, const uint64_t* rows, size_t n_vars, size_t n_h, int form, uint8_t* out, size_t cap, uint64_t* out_len,
                                    uint64_t* first_bad_point) {
  return wire_key_serialize(1, vk, n_inputs, rows, n_vars, n_h, form, out, cap, out_len, first_bad_point);
}
int groth16_serialize_proof_bw6_761(const uint64_t a_xyz[36], const uint64_t b_xyz[36], const uint64_t c_xyz[36], uint8_t out[288]) {
  return wire761_proof_serialize(a_xyz, b_xyz, c_xyz, out);
}
int groth16_serialize_proof_bls12_377(const uint64_t a_xyz[18], const uint64_t b_xyz[36], const uint64_t c_xyz[18], uint8_t out[192]) {
  return wire377_proof_serialize(a_xyz, b_xyz, c_xyz, out);
}
int celo_amd_wire_encode_last_ms(float* ms) { if (!ms) return 2; *ms = wire_encode_last_ms(); return 0; }
int celo_amd_wire_encode_key_timings(float ms[3]) { if (!ms) return 2; wire_encode_key_timings(ms); return 0; }
int hash_to_g1_direct_bls12_377(const uint8_t domain[8], const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* extras, const uint64_t* extra_off,
                                size_t n, uint64_t* out_xy, uint8_t* attempts) {
  return hash_to_g1_direct_run(domain, msgs, msg_off, extras, extra_off, n, out_xy, attempts, 0);
}
int hash_to_g1_cip22_tail_bls12_377(const uint8_t domain[8], const uint8_t* inner, const uint64_t* inner_off, const uint8_t* extras, const uint64_t* extra_off,
                                    size_t n, uint64_t* out_xy, uint8_t* attempts) {
  return hash_to_g1_direct_run(domain, inner, inner_off, extras, extra_off, n, out_xy, attempts, 1);
}
int hash_to_g1_composite_bls12_377(const uint8_t domain[8], const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* extras, const uint64_t* extra_off,
                                   size_t n, int cip22, uint64_t* out_xy, uint8_t* attempts) {
  return hash_to_g1_direct_run(domain, msgs, msg_off, extras, extra_off, n, out_xy, attempts, cip22 ? 3 : 2);
}
int hash_to_g2_direct_bls12_377(const uint8_t domain[8], const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* extras, const uint64_t* extra_off,
                                size_t n, int compat, uint64_t* out_xy, uint8_t* attempts) {
  return hash_to_g2_run(domain, msgs, msg_off, extras, extra_off, n, compat, out_xy, attempts, 0);
}
int hash_to_g2_cip22_tail_bls12_377(const uint8_t domain[8], const uint8_t* inner, const uint64_t* inner_off, const uint8_t* extras, const uint64_t* extra_off,
                                    size_t n, int compat, uint64_t* out_xy, uint8_t* attempts) {
  return hash_to_g2_run(domain, inner, inner_off, extras, extra_off, n, compat, out_xy, attempts, 1);
}
int hash_to_g2_composite_bls12_377(const uint8_t domain[8], const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* extras, const uint64_t* extra_off,
                                   size_t n, int cip22, int compat, uint64_t* out_xy, uint8_t* attempts) {
  return hash_to_g2_run(domain, msgs, msg_off, extras, extra_off, n, compat, out_xy, attempts, cip22 ? 3 : 2);
}
int hash_to_g2_one_bls12_377(const uint8_t domain[8], const uint8_t* msg, size_t mlen, const uint8_t* extra, size_t elen, int mode, int compat, uint64_t out_xy[24],
                             int* attempt) {
  return hash_to_g2_one_run(domain, msg, mlen, extra, elen, mode, compat, out_xy, attempt);
}
int celo_amd_hash_g2_set_lane_budget_log(int log) { return hash_g2_set_lane_budget_log(log); }
int celo_amd_hash_g2_last_split(float ms[2]) { if (!ms) return 2; hash_g2_last_split(ms); return 0; }
int composite_crh_bls12_377(const uint8_t* msgs, const uint64_t* msg_off, size_t n, uint8_t* out48) { return pedersen_crh_run(msgs, msg_off, n, out48); }
int composite_crh_bls12_377_dev(const void* d_msgs, const uint64_t* msg_off, size_t n, void* d_out48, void* hip_stream) {
  return pedersen_crh_run((const uint8_t*)d_msgs, msg_off, n, (uint8_t*)d_out48, 1, hip_stream);
}
int hash_to_g1_direct_bls12_377_dev(const uint8_t domain[8], const void* d_msgs, const uint64_t* msg_off, const void* d_extras, const uint64_t* extra_off, size_t n,
                                    void* d_out_xy, void* d_attempts, void* hip_stream) {
  return hash_to_g1_direct_run(domain, (const uint8_t*)d_msgs, msg_off, (const uint8_t*)d_extras, extra_off, n, (uint64_t*)d_out_xy, (uint8_t*)d_attempts, 0, 1, hip_stream);
}
int hash_to_g1_cip22_tail_bls12_377_dev(const uint8_t domain[8], const void* d_inner, const uint64_t* inner_off, const void* d_extras, const uint64_t* extra_off, size_t n,
                                        void* d_out_xy, void* d_attempts, void* hip_stream) {
  return hash_to_g1_direct_run(domain, (const uint8_t*)d_inner, inner_off, (const uint8_t*)d_extras, extra_off, n, (uint64_t*)d_out_xy, (uint8_t*)d_attempts, 1, 1, hip_stream);
}
int hash_to_g1_composite_bls12_377_dev(const uint8_t domain[8], const void* d_msgs, const uint64_t* msg_off, const void* d_extras, const uint64_t* extra_off, size_t n,
                                       int cip22, void* d_out_xy, void* d_attempts, void* hip_stream) {
  return hash_to_g1_direct_run(domain, (const uint8_t*)d_msgs, msg_off, (const uint8_t*)d_extras, extra_off, n, (uint64_t*)d_out_xy, (uint8_t*)d_attempts, cip22 ? 3 : 2, 1,
                               hip_stream);
}
int celo_amd_hash_last_ms(float* ms) { if (!ms) return 2; *ms = hash_last_ms(); return 0; }
int celo_amd_hash_last_rounds(int* rounds) { if (!rounds) return 2; *rounds = hash_last_rounds(); return 0; }
int celo_amd_crh_set_lanes(int lanes) { return crh_set_lanes(lanes); }
int celo_amd_crh_last_lanes(int* lanes) { if (!lanes) return 2; *lanes = crh_last_lanes(); return 0; }
int normalize_bls12_377_g1(const uint64_t* jac, size_t n, uint64_t* out_xy, uint8_t* inf) { return wire_normalize(0, jac, n, out_xy, inf); }
int normalize_bls12_377_g2(const uint64_t* jac, size_t n, uint64_t* out_xy, uint8_t* inf) { return wire_normalize(1, jac, n, out_xy, inf); }
// ---- batched fixed-base scalar multiplication and Groth16 setup (unit_setup.hip)
int fixed_base_mul_bls12_377_g1(const uint64_t gen_xy[12], const uint64_t* scalars, size_t n, uint64_t* out_xy, uint8_t* inf) { return fixed_base_mul(0, gen_xy, scalars, n, out_xy, inf, 0, nullptr); }
int fixed_base_mul_bls12_377_g2(const uint64_t gen_xy[24], const uint64_t* scalars, size_t n, uint64_t* out_xy, uint8_t* inf) { return fixed_base_mul(1, gen_xy, scalars, n, out_xy, inf, 0, nullptr); }
int fixed_base_mul_bw6_761_g1(const uint64_t gen_xy[24], const uint64_t* scalars, size_t n, uint64_t* out_xy, uint8_t* inf) { return fixed_base_mul(2, gen_xy, scalars, n, out_xy, inf, 0, nullptr); }
int fixed_base_mul_bw6_761_g2(const uint64_t gen_xy[24], const uint64_t* scalars, size_t n, uint64_t* out_xy, uint8_t* inf) { return fixed_base_mul(2, gen_xy, scalars, n, out_xy, inf, 0, nullptr); }
int fixed_base_mul_bls12_377_g1_dev(const uint64_t* gen_xy, const void* d_scalars, size_t n, void* d_out_xy, void* d_inf, void* hip_stream) {
  return fixed_base_mul(0, gen_xy, d_scalars, n, d_out_xy, d_inf, 1, hip_stream);
}
int fixed_base_mul_bls12_377_g2_dev(const uint64_t* gen_xy, const void* d_scalars, size_t n, void* d_out_xy, void* d_inf, void* hip_stream) {
  return fixed_base_mul(1, gen_xy, d_scalars, n, d_out_xy, d_inf, 1, hip_stream);
}
int fixed_base_mul_bw6_761_g1_dev(const uint64_t* gen_xy, const void* d_scalars, size_t n, void* d_out_xy, void* d_inf, void* hip_stream) {
  return fixed_base_mul(2, gen_xy, d_scalars, n, d_out_xy, d_inf, 1, hip_stream);
}
int fixed_base_mul_bw6_761_g2_dev(const uint64_t* gen_xy, const void* d_scalars, size_t n, void* d_out_xy, void* d_inf, void* hip_stream) {
  return fixed_base_mul(2, gen_xy, d_scalars, n, d_out_xy, d_inf, 1, hip_stream);
}
int normalize_bw6_761_g1(const uint64_t* jac, size_t n, uint64_t* out_xy, uint8_t* inf) { return wire_normalize(2, jac, n, out_xy, inf); }
int normalize_bw6_761_g2(const uint64_t* jac, size_t n, uint64_t* out_xy, uint8_t* inf) { return wire_normalize(2, jac, n, out_xy, inf); }
int groth16_setup_bw6_761(const uint64_t* qap_a, const uint64_t* qap_b, const uint64_t* qap_c, size_t n_vars, size_t n_inputs, const uint64_t zt[6], const uint64_t tau[6],
                          size_t n_h, const uint64_t toxic[24], const uint64_t g1_xy[24], const uint64_t g2_xy[24], int window_bits, uint64_t* out_vk,
                          uint64_t* out_rows, void** out_key) {
  return groth16_setup(0, qap_a, qap_b, qap_c, n_vars, n_inputs, zt, tau, n_h, toxic, g1_xy, g2_xy, window_bits, out_vk, out_rows, (ProvingKey**)out_key);
}
int groth16_setup_bls12_377(const uint64_t* qap_a, const uint64_t* qap_b, const uint64_t* qap_c, size_t n_vars, size_t n_inputs, const uint64_t zt[4],
                            const uint64_t tau[4], size_t n_h, const uint64_t toxic[16], const uint64_t g1_xy[12], const uint64_t g2_xy[24], int window_bits,
                            uint64_t* out_vk, uint64_t* out_rows, void** out_key) {
  return groth16_setup(1, qap_a, qap_b, qap_c, n_vars, n_inputs, zt, tau, n_h, toxic, g1_xy, g2_xy, window_bits, out_vk, out_rows, (ProvingKey**)out_key);
}
int celo_amd_fixed_base_set_window(int window_bits) { return fixed_base_set_window(window_bits); }
int celo_amd_setup_last_timings(float ms[8]) { if (!ms) return 2; setup_last_timings(ms); return 0; }
// ---- batched variable-base scalar multiplication and batched signing (unit_varbase.hip)
#define SCALAR_MUL(NAME, GROUP, SUBGROUP)                                                                                                                   \
  int scalar_mul_batch_##NAME(const uint64_t* xy, const uint8_t* inf, const uint64_t* scalars, size_t n_scalars, size_t n, uint64_t* out_xy, uint8_t* out_inf) { \
    return scalar_mul_batch(GROUP, SUBGROUP, xy, inf, scalars, n_scalars, n, out_xy, out_inf, 0, nullptr);                                                 \
  }                                                                                                                                                        \
  int scalar_mul_batch_##NAME##_dev(const void* d_xy, const void* d_inf, const void* d_scalars, size_t n_scalars, size_t n, void* d_out_xy, void* d_out_inf, \
                                    void* hip_stream) {                                                                                                    \
    return scalar_mul_batch(GROUP, SUBGROUP, d_xy, d_inf, d_scalars, n_scalars, n, d_out_xy, d_out_inf, 1, hip_stream);                                    \
  }
SCALAR_MUL(bls12_377_g1, 0, 0)
SCALAR_MUL(bls12_377_g1_subgroup, 0, 1)
SCALAR_MUL(bls12_377_g2, 1, 0)
SCALAR_MUL(bw6_761_g1, 2, 0)
SCALAR_MUL(bw6_761_g2, 2, 0)
#undef SCALAR_MUL
int sign_batch_bls12_377(const uint64_t* sk, size_t n_sk, const uint8_t domain[8], const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* extras,
                         const uint64_t* extra_off, size_t n, int mode, uint8_t* out_sig48, uint8_t* attempts) {
  return sign_batch_377(sk, n_sk, domain, msgs, msg_off, extras, extra_off, n, mode, out_sig48, attempts);
}
int celo_amd_scalar_mul_set_window(int c) { return scalar_mul_set_window(c); }
int celo_amd_scalar_mul_set_chunk_rows(uint32_t rows) { return scalar_mul_set_chunk_rows(rows); }
int celo_amd_scalar_mul_last_ms(float ms[4]) { if (!ms) return 2; scalar_mul_last_ms(ms); return 0; }
// ---- masked segmented point sums and aggregated seals (unit_seals.hip)
#define AGG_BITMAP(NAME, GROUP)                                                                                                                            \
  int aggregate_by_bitmap_##NAME(const uint64_t* pk_xy, const uint8_t* pk_inf, const uint32_t* offsets, size_t n_sets, const uint8_t* bits, size_t m,      \
                                 uint64_t* out_xy, uint8_t* out_inf, uint32_t* out_count) {                                                                \
    return aggregate_by_bitmap(GROUP, pk_xy, pk_inf, offsets, n_sets, bits, m, out_xy, out_inf, out_count, 0, nullptr);                                    \
  }                                                                                                                                                        \
  int aggregate_by_bitmap_##NAME##_dev(const void* d_pk_xy, const void* d_pk_inf, const uint32_t* offsets, size_t n_sets, const void* d_bits, size_t m,    \
                                       void* d_out_xy, void* d_out_inf, void* d_out_count, void* hip_stream) {                                             \
    return aggregate_by_bitmap(GROUP, d_pk_xy, d_pk_inf, offsets, n_sets, d_bits, m, d_out_xy, d_out_inf, d_out_count, 1, hip_stream);                     \
  }
AGG_BITMAP(bls12_377_g1, 0)
AGG_BITMAP(bls12_377_g2, 1)
#undef AGG_BITMAP
int verify_aggregated_seals_bls12_377(const uint64_t* pk_xy, const uint8_t* pk_inf, const uint32_t* offsets, size_t n_sets, const uint8_t* bits, const uint32_t* min_signers,
                                      const uint8_t domain[8], const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* extras, const uint64_t* extra_off, int hash_mode,
                                      const uint8_t* sig48, const uint64_t neg_g2_xy[24], size_t m, int mode, const uint32_t* key, uint8_t* out_ok, uint8_t* out_status) {
  return verify_aggregated_seals_377(pk_xy, pk_inf, offsets, n_sets, bits, min_signers, domain, msgs, msg_off, extras, extra_off, hash_mode, sig48, neg_g2_xy, m, mode, key,
                                     out_ok, out_status);
}
int celo_amd_aggregate_set_lanes(int lanes) { return aggregate_set_lanes(lanes); }
int celo_amd_aggregate_set_complement(int mode) { return aggregate_set_complement(mode); }
int celo_amd_seals_last(int* path, int* lanes, float ms[8]) { if (!path || !lanes || !ms) return 2; seals_last(path, lanes, ms); return 0; }
// ---- epoch blocks to bytes, public inputs and verdicts (unit_epoch.hip); celo_epoch_blocks is EpochBlocks field for field
static_assert(sizeof(celo_epoch_blocks) == sizeof(celo::EpochBlocks), "celo_epoch_blocks and EpochBlocks are one layout");
int epoch_encoded_size(int kind, uint64_t n_keys, uint64_t max_validators, uint64_t* bytes) { return celo::epoch_encoded_size(kind, n_keys, max_validators, bytes); }
int epoch_encode_blocks_bls12_377(const celo_epoch_blocks* blocks, size_t nb, int kind, const uint64_t* out_off, uint8_t* out, uint8_t* extras, uint8_t* status) {
  return epoch_encode_blocks((const EpochBlocks*)blocks, nb, kind, out_off, out, extras, status, 0, nullptr);
}
int epoch_encode_blocks_bls12_377_dev(const celo_epoch_blocks* blocks, size_t nb, int kind, const uint64_t* out_off, void* d_out, void* d_extras, void* d_status,
                                      void* hip_stream) {
  return epoch_encode_blocks((const EpochBlocks*)blocks, nb, kind, out_off, d_out, d_extras, d_status, 1, hip_stream);
}
int epoch_public_inputs_bw6_761(const celo_epoch_blocks* first, const celo_epoch_blocks* last, size_t m, uint64_t* out_inputs, uint8_t* out_status) {
  return epoch_public_inputs((const EpochBlocks*)first, (const EpochBlocks*)last, m, out_inputs, out_status, 0, nullptr);
}
int epoch_public_inputs_bw6_761_dev(const celo_epoch_blocks* first, const celo_epoch_blocks* last, size_t m, void* d_out_inputs, void* d_out_status, void* hip_stream) {
  return epoch_public_inputs((const EpochBlocks*)first, (const EpochBlocks*)last, m, d_out_inputs, d_out_status, 1, hip_stream);
}
int verify_epoch_proofs_bw6_761(const void* vk, const uint8_t* proofs, const celo_epoch_blocks* first, const celo_epoch_blocks* last, size_t m, int mode,
                                const uint32_t* key, uint8_t* out_ok, uint8_t* out_status) {
  return verify_epoch_proofs((const VerifyingKey*)vk, proofs, (const EpochBlocks*)first, (const EpochBlocks*)last, m, mode, key, out_ok, out_status);
}
int celo_amd_epoch_last(float ms[8]) { if (!ms) return 2; epoch_last(ms); return 0; }
// ---- chains of epoch transitions (unit_transitions.hip)
int verify_epoch_transitions_bls12_377(const celo_epoch_blocks* blocks, size_t nb, const uint32_t* chain_off, size_t n_chains, const uint8_t* bits, const uint8_t* sig48,
                                       const uint8_t domain[8], const uint64_t neg_g2_xy[24], int mode, uint8_t* out_ok, uint8_t* out_status, uint8_t* out_chain_ok,
                                       uint8_t* out_crh, uint8_t* out_attempts, uint64_t* out_asig_xy, uint8_t* out_asig_inf) {
  return verify_epoch_transitions((const EpochBlocks*)blocks, nb, chain_off, n_chains, bits, sig48, domain, neg_g2_xy, mode, out_ok, out_status, out_chain_ok, out_crh,
                                  out_attempts, out_asig_xy, out_asig_inf);
}
int celo_amd_transitions_last(int* path, float ms[8]) { if (!path || !ms) return 2; transitions_last(path, ms); return 0; }
// ---- R1CS matrices on the device (unit_r1cs.hip)
#define R1CS_LOAD(NAME, CURVE)                                                                                                                              \
  int NAME(size_t n_constraints, size_t n_vars, size_t n_inputs, const uint64_t* a_row_ptr, const uint32_t* a_col, const uint64_t* a_val, size_t a_nnz,     \
           const uint64_t* b_row_ptr, const uint32_t* b_col, const uint64_t* b_val, size_t b_nnz, const uint64_t* c_row_ptr, const uint32_t* c_col,          \
           const uint64_t* c_val, size_t c_nnz, void** out_r1cs, uint64_t* first_bad) {                                                                     \
    if (!out_r1cs) return 2;                                                                                                                                \
    *out_r1cs = nullptr;                                                                                                                                    \
    const uint64_t* const rp[3] = {a_row_ptr, b_row_ptr, c_row_ptr};                                                                                       \
    const uint32_t* const col[3] = {a_col, b_col, c_col};                                                                                                   \
    const uint64_t* const val[3] = {a_val, b_val, c_val};                                                                                                   \
    const uint64_t nnz[3] = {a_nnz, b_nnz, c_nnz};                                                                                                          \
    return r1cs_load(CURVE, n_constraints, n_vars, n_inputs, rp, col, val, nnz, (R1cs**)out_r1cs, first_bad);                                               \
  }
R1CS_LOAD(groth16_r1cs_load_bw6_761, 0) R1CS_LOAD(groth16_r1cs_load_bls12_377, 1)
#undef R1CS_LOAD
int groth16_r1cs_info(const void* r1cs, uint64_t out[8]) { return r1cs_info((const R1cs*)r1cs, out); }
int groth16_r1cs_free(void* r1cs) { if (!r1cs) return 2; r1cs_free((R1cs*)r1cs); return 0; }
int groth16_r1cs_rows(const void* r1cs, const uint64_t* z, unsigned log_n, uint64_t* out_a, uint64_t* out_b, uint64_t* out_c) {
  return r1cs_rows((const R1cs*)r1cs, z, log_n, out_a, out_b, out_c, 0, nullptr);
}
int groth16_r1cs_rows_dev(const void* r1cs, const uint64_t* d_z, unsigned log_n, uint64_t* d_out_a, uint64_t* d_out_b, uint64_t* d_out_c, void* hip_stream) {
  return r1cs_rows((const R1cs*)r1cs, d_z, log_n, d_out_a, d_out_b, d_out_c, 1, hip_stream);
}
int groth16_r1cs_check(const void* r1cs, const uint64_t* z, int64_t* first_unsatisfied) { return r1cs_check((const R1cs*)r1cs, z, first_unsatisfied); }
int groth16_r1cs_qap_at_tau(const void* r1cs, unsigned log_n, const uint64_t* omega, const uint64_t* tau, uint64_t* out_a, uint64_t* out_b, uint64_t* out_c,
                            uint64_t* out_zt) {
  return r1cs_qap_at_tau((const R1cs*)r1cs, log_n, omega, tau, out_a, out_b, out_c, out_zt, 0, nullptr);
}
int groth16_r1cs_qap_at_tau_dev(const void* r1cs, unsigned log_n, const uint64_t* omega, const uint64_t* tau, uint64_t* d_out_a, uint64_t* d_out_b, uint64_t* d_out_c,
                                uint64_t* out_zt, void* hip_stream) {
  return r1cs_qap_at_tau((const R1cs*)r1cs, log_n, omega, tau, d_out_a, d_out_b, d_out_c, out_zt, 1, hip_stream);
}
int groth16_prove_r1cs_with_key(const void* key, const void* r1cs, const uint64_t* z, unsigned log_n, const uint64_t* omega, const uint64_t* omega_inv,
                                const uint64_t* coset, const uint64_t* coset_inv, const uint64_t* size_inv, const uint64_t* vanishing_inv, uint64_t* out_a,
                                uint64_t* out_b, uint64_t* out_c) {
  return groth16_prove_r1cs((const ProvingKey*)key, (const R1cs*)r1cs, z, 0, log_n, omega, omega_inv, coset, coset_inv, size_inv, vanishing_inv, out_a, out_b, out_c);
}
int groth16_prove_r1cs_with_key_dev(const void* key, const void* r1cs, const uint64_t* d_z, unsigned log_n, const uint64_t* omega, const uint64_t* omega_inv,
                                    const uint64_t* coset, const uint64_t* coset_inv, const uint64_t* size_inv, const uint64_t* vanishing_inv, uint64_t* out_a,
                                    uint64_t* out_b, uint64_t* out_c) {
  return groth16_prove_r1cs((const ProvingKey*)key, (const R1cs*)r1cs, d_z, 1, log_n, omega, omega_inv, coset, coset_inv, size_inv, vanishing_inv, out_a, out_b, out_c);
}
int groth16_setup_r1cs_bw6_761(const void* r1cs, unsigned log_n, const uint64_t omega[6], const uint64_t tau[6], const uint64_t toxic[24], const uint64_t g1_xy[24],
                               const uint64_t g2_xy[24], int window_bits, uint64_t* out_vk, uint64_t* out_rows, void** out_key) {
  return groth16_setup_r1cs(0, (const R1cs*)r1cs, log_n, omega, tau, toxic, g1_xy, g2_xy, window_bits, out_vk, out_rows, (ProvingKey**)out_key);
}
int groth16_setup_r1cs_bls12_377(const void* r1cs, unsigned log_n, const uint64_t omega[4], const uint64_t tau[4], const uint64_t toxic[16], const uint64_t g1_xy[12],
                                 const uint64_t g2_xy[24], int window_bits, uint64_t* out_vk, uint64_t* out_rows, void** out_key) {
  return groth16_setup_r1cs(1, (const R1cs*)r1cs, log_n, omega, tau, toxic, g1_xy, g2_xy, window_bits, out_vk, out_rows, (ProvingKey**)out_key);
}
int celo_amd_r1cs_last_timings(float ms[8]) { if (!ms) return 2; r1cs_last_timings(ms); return 0; }

// ---- the HashToBits circuit of the hash-helper proof (unit_hashbits.hip)
int hash_to_bits_r1cs_size_bls12_377(size_t n_epochs, uint64_t out[8]) { return hashbits_sizes(n_epochs, out); }
int hash_to_bits_r1cs_bls12_377(size_t n_epochs, uint64_t* a_row_ptr, uint32_t* a_col, uint64_t* a_val, uint64_t* b_row_ptr, uint32_t* b_col, uint64_t* b_val,
                                uint64_t* c_row_ptr, uint32_t* c_col, uint64_t* c_val) {
  uint64_t* const rp[3] = {a_row_ptr, b_row_ptr, c_row_ptr};
  uint32_t* const col[3] = {a_col, b_col, c_col};
  uint64_t* const val[3] = {a_val, b_val, c_val};
  return hashbits_write_csr(n_epochs, rp, col, val);
}
int hash_to_bits_r1cs_load_bls12_377(size_t n_epochs, void** out_r1cs) {
  if (!out_r1cs) return 2;
  *out_r1cs = nullptr;
  return hashbits_r1cs_load(n_epochs, (R1cs**)out_r1cs);
}
int hash_to_bits_assignment_bls12_377(const uint8_t* rows48, size_t n_epochs, int bit_order, uint64_t* z) {
  return hashbits_assignment(rows48, n_epochs, bit_order, z, 0, nullptr);
}
int hash_to_bits_assignment_bls12_377_dev(const uint8_t* d_rows48, size_t n_epochs, int bit_order, uint64_t* d_z, void* hip_stream) {
  return hashbits_assignment(d_rows48, n_epochs, bit_order, d_z, 1, hip_stream);
}
int celo_amd_hash_to_bits_assignment_host(const uint8_t* rows48, size_t n_epochs, int bit_order, uint64_t* z) {
  return hashbits_assignment_host(rows48, n_epochs, bit_order, z);
}
int hash_to_bits_public_inputs_bls12_377(const uint8_t* rows48, size_t n_proofs, size_t n_epochs, int bit_order, uint64_t* out) {
  return hashbits_public_inputs(rows48, n_proofs, n_epochs, bit_order, out, 0, nullptr);
}
int hash_to_bits_public_inputs_bls12_377_dev(const uint8_t* d_rows48, size_t n_proofs, size_t n_epochs, int bit_order, uint64_t* d_out, void* hip_stream) {
  return hashbits_public_inputs(d_rows48, n_proofs, n_epochs, bit_order, d_out, 1, hip_stream);
}
int groth16_hash_helper_prove_bls12_377(const void* key, const void* r1cs, const uint8_t* rows48, size_t n_epochs, int bit_order, unsigned log_n, const uint64_t* omega,
                                        const uint64_t* omega_inv, const uint64_t* coset, const uint64_t* coset_inv, const uint64_t* size_inv,
                                        const uint64_t* vanishing_inv, uint64_t* out_a, uint64_t* out_b, uint64_t* out_c, uint64_t* out_inputs) {
  return hash_helper_prove((const ProvingKey*)key, (const R1cs*)r1cs, rows48, n_epochs, bit_order, log_n, omega, omega_inv, coset, coset_inv, size_inv, vanishing_inv,
                           out_a, out_b, out_c, out_inputs);
}
int groth16_hash_helper_verify_bls12_377(const void* vk, const uint8_t* rows48, size_t n_proofs, size_t n_epochs, int bit_order, const uint8_t* proofs, int mode,
                                         const uint32_t* key, uint8_t* out_ok) {
  return hash_helper_verify((const VerifyingKey*)vk, rows48, n_proofs, n_epochs, bit_order, proofs, mode, key, out_ok);
}
int celo_amd_hash_helper_last(float ms[8]) { if (!ms) return 2; hash_helper_last(ms); return 0; }
int celo_amd_decompress_last_ms(float* ms) { if (!ms) return 2; *ms = wire_last_ms(); return 0; }
int celo_amd_msm_last_timings(int group, float ms[5], int cfg[3]) {
  return by_group(group, 1, [&](auto g) { return MsmAuxApi<typename decltype(g)::type>::timings(ms, cfg); });
}
int celo_amd_selftest_accumulate(int group, const uint64_t* gen_xy, uint32_t runs, uint32_t len, uint32_t seed, uint32_t check, int chunked, uint32_t* differ) {
  return by_group(group, 2, [&](auto g) { return MsmApi<typename decltype(g)::type>::selftest_accumulate(gen_xy, runs, len, seed, check, chunked, differ); });
}
int celo_amd_ubench_fp(float out[9]) {
  if (!out) return 2;
  return celo::ubench_fp_run(out);
}
int celo_amd_msm_set_host_chunks(int chunks) {
  if (chunks < -1 || (chunks >= 0 && ((chunks & 0xFF) > 64 || ((chunks >> 8) & 15) > 9 || ((chunks >> 12) & 15) > 9 || (chunks >> 16)))) return 1;      // (chunks | (head_split + 1) << 8 | (tail_split + 1) << 12)
  celo::host_chunks_override().store(chunks);
  return 0;
}
int celo_amd_msm_set_batched_affine(int on) {
  if (on < -1 || on > 1) return 1;
  celo::batched_affine_override().store(on);
  return 0;
}
int celo_amd_msm_host_chunk_plan(uint64_t n, int chunks, int head_split, int tail_split, uint32_t* cm, uint32_t lens[80]) {
  if (!cm || !lens || chunks < 1 || chunks > 64 || head_split < 0 || head_split > 8 || tail_split < 0 || tail_split > 8 || n < ((uint64_t)chunks << 16) || n >= (uint64_t(1) << 30)) return -1;
  return (int)celo::host_chunk_plan((size_t)n, (uint32_t)chunks, (uint32_t)head_split, (uint32_t)tail_split, *cm, lens);
}
int celo_amd_msm_set_window_bits(int group, int c) {
  if (c != 0 && (c < 3 || c > 16)) return 1;
  return by_group(group, 1, [&](auto g) { return MsmAuxApi<typename decltype(g)::type>::set_c(c); });
}
int celo_amd_sum_jacobian_bls12_377_g1(const uint64_t* j, size_t k, uint64_t* out) { return MsmAuxApi<G1_377>::sum_jac(j, k, out); }
int celo_amd_sum_jacobian_bls12_377_g2(const uint64_t* j, size_t k, uint64_t* out) { return MsmAuxApi<G2_377>::sum_jac(j, k, out); }
int celo_amd_sum_jacobian_bw6_761(const uint64_t* j, size_t k, uint64_t* out) { return MsmAuxApi<G_761>::sum_jac(j, k, out); }
int celo_amd_gen_points_bls12_377_g1_dev(void* d, size_t n, uint64_t seed, const uint64_t* g, void* st) { return MsmAuxApi<G1_377>::gen_points(d, n, seed, g, 1, 0, st); }
int celo_amd_gen_points_bls12_377_g2_dev(void* d, size_t n, uint64_t seed, const uint64_t* g, void* st) { return MsmAuxApi<G2_377>::gen_points(d, n, seed, g, 1, 0, st); }
int celo_amd_gen_points_bw6_761_dev(void* d, size_t n, uint64_t seed, const uint64_t* g, void* st) { return MsmAuxApi<G_761>::gen_points(d, n, seed, g, 1, 0, st); }
int celo_amd_gen_points_grouped_bls12_377_g1_dev(void* d, size_t n, uint64_t seed, const uint64_t* gens, size_t ngens, uint32_t per, void* st) {
  return MsmAuxApi<G1_377>::gen_points(d, n, seed, gens, ngens, per, st);
}
int celo_amd_gen_points_grouped_bls12_377_g2_dev(void* d, size_t n, uint64_t seed, const uint64_t* gens, size_t ngens, uint32_t per, void* st) {
  return MsmAuxApi<G2_377>::gen_points(d, n, seed, gens, ngens, per, st);
}
}
