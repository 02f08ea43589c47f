// Translation unit: Groth16 verification over BW6-761 for m proofs under one verifying key (groth16_verify_unit.h instantiated for G16Bw6;
// crates/epoch-snark/src/api/verifier.rs:35), and what both curves of the verifier share: the registry of live handles, the record of the
// last call and the exponent draw.  DESIGN.md section 6h.
#include "groth16_verify_unit.h"
#include <atomic>
#include <mutex>
#include <set>

namespace celo {
template struct G16Api<G16Bw6>;

// the handles that are alive: a freed or foreign pointer is refused, not followed; so is a handle of the other curve
static std::mutex g_vk_mu;
static std::set<const VerifyingKey*>& vk_live() { static auto* s = new std::set<const VerifyingKey*>(); return *s; }
void groth16_vk_adopt(VerifyingKey* vk) { std::lock_guard<std::mutex> lk(g_vk_mu); vk_live().insert(vk); }
bool groth16_vk_is_live(const VerifyingKey* vk, int curve) {
  std::lock_guard<std::mutex> lk(g_vk_mu);
  return vk_live().count(vk) != 0 && vk->curve == curve;
}
int groth16_vk_inputs(const VerifyingKey* vk, int curve) {
  std::lock_guard<std::mutex> lk(g_vk_mu);
  return vk_live().count(vk) != 0 && vk->curve == curve ? (int)vk->n_in : -1;
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

// the last call: path 0 = each, 1 = combined accepted, 2 = combined rejected then each; ms: [0] decoding, [1] input sums, [2] exponents
// and ladders, [3] the two MSMs and (sum r) alpha (wall), [4] pairing products (HIP events of the engine, both passes of path 2),
// [5] wall, [6] transfers to the device; lanes / n_in: the lanes per input sum and the key's input count
struct G16Last { int path = -1, c = 0, lanes = 0, n_in = 0; float ms[8] = {}; };
static Last<G16Last> g_last;
void groth16_verify_note(int path, int window_bits, const float ms[8], int lanes, int n_inputs) {
  G16Last r{path, window_bits, lanes, n_inputs};
  for (int i = 0; i < 8; i++) r.ms[i] = ms[i];
  g_last.note(r);
}
int groth16_inputs_last(int* lanes, int* n_inputs) {
  if (!lanes || !n_inputs) return 2;
  const G16Last r = g_last.read();
  *lanes = r.lanes; *n_inputs = r.n_in;
  return 0;
}
// a test and tuning switch: 0 = the rule (g16_pick_lanes), else the lanes per input sum of every BLS12-377 call; an atomic, no device needed
static std::atomic<int> g_input_lanes{0};
int groth16_set_input_lanes(int lanes) {
  if (lanes != 0 && !g16_lanes_ok(lanes)) return 2;
  g_input_lanes.store(lanes);
  return 0;
}
int groth16_input_lanes() { return g_input_lanes.load(); }

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
  hipLaunchKernelGGL((k_g16_exponents<6>), dim3(((uint32_t)m + 255) / 256), dim3(256), 0, cs.stream(), d_r4, (const uint8_t*)nullptr, (uint32_t)m, d_sc);
  HIP_TRY(hipGetLastError(), 10);
  HIP_TRY(hipMemcpyAsync(h.data(), d_sc, m * 48, hipMemcpyDeviceToHost, cs.stream()), 10);
  HIP_TRY(hipStreamSynchronize(cs.stream()), 10);
  for (size_t i = 0; i < m; i++) { out[2 * i] = h[6 * i]; out[2 * i + 1] = h[6 * i + 1]; }
  return 0;
}

int groth16_verify_last(int* path, int* window_bits, float ms[8]) {
  const G16Last r = g_last.read();
  if (path) *path = r.path;
  if (window_bits) *window_bits = r.c;
  if (ms) for (int i = 0; i < 8; i++) ms[i] = r.ms[i];
  return 0;
}

}  // namespace celo
