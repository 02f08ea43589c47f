// Translation unit: bulk ENCODING of points into arkworks' wire form (wire.h WireEnc, wire761.h), one point per lane - the twin of
// unit_wire.hip's and unit_wire761.hip's decoders - and, on top of it, the writers of a serialized ark-groth16 0.1 ProvingKey / VerifyingKey
// of either curve (what groth16_load_key_<curve>_serialized reads) and of a Proof.
#include "wire761.h"
#include <hip/hip_runtime.h>
#include <mutex>
#include "runtime.h"
#include "units.h"

namespace celo {
// bulk calls, serialised per process like the decoders' (serialisation only); host-pointer calls run on a stream of their own, the _dev forms on the caller's
static std::mutex wenc_mu;
static Last<float> g_wenc_last;              // kernel ms of the last encode call (the key writer: all its launches)
static Last<CallTimes> g_wenc_key_last;      // the last key writer call: [0] rows in, [1] encode, [2] bytes out

// E: a WireEnc instantiation.  in: n rows of E::ROW_WORDS u64; out: n x E::OUT_WORDS u64 (48 .. 192 B per point), written as 64-bit words;
// status: n bytes.  The control flow is uniform up to WireEnc::row's per-lane exits (identity, not a field element).
// Every lane stores its own row, lanes E::OUT_WORDS words apart.  A variant that passed the block's rows through LDS and stored them as
// contiguous words was measured and is not kept: never faster, up to 11 % slower (DESIGN.md 6c'', profiles/ab_wire_encode_staged.json).
template <class E> __global__ void __launch_bounds__(64)
k_encode(const uint64_t* __restrict__ in, const uint8_t* __restrict__ inf, uint64_t* __restrict__ out, uint8_t* __restrict__ status, uint32_t n, int ark_zero) {
  constexpr int OW = E::OUT_WORDS, RW = E::ROW_WORDS;
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint64_t r[RW], o[OW];
  const uint64_t* src = in + (size_t)i * RW;
#pragma unroll
  for (int j = 0; j < RW; j++) r[j] = src[j];
  status[i] = E::row(r, inf != nullptr && inf[i] != 0, ark_zero != 0, o);
  uint64_t* dst = out + (size_t)i * OW;
#pragma unroll
  for (int j = 0; j < OW; j++) dst[j] = o[j];
}
// the smallest index of a row that is no pair of field elements (status 2)
__global__ void __launch_bounds__(256) k_first_bad_encode(const uint8_t* __restrict__ status, uint32_t n, unsigned long long* first) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && status[i] == WIRE_INVALID) atomicMin(first, (unsigned long long)i);
}

template <class E> static void launch_one(const uint64_t* d_in, const uint8_t* d_inf, uint64_t* d_out, uint8_t* d_st, size_t n, int ark_zero, hipStream_t s) {
  const dim3 grid(((uint32_t)n + 63) / 64), block(64);
  hipLaunchKernelGGL((k_encode<E>), grid, block, 0, s, d_in, d_inf, d_out, d_st, (uint32_t)n, ark_zero);
}
// group 0 / 1: BLS12-377 G1 / G2, 2: BW6-761 (both groups)
static void launch_encode(int group, int compressed, const uint64_t* d_in, const uint8_t* d_inf, uint64_t* d_out, uint8_t* d_st, size_t n, int ark_zero, hipStream_t s) {
  if (group == 2) {
    if (compressed) launch_one<W761EncC>(d_in, d_inf, d_out, d_st, n, ark_zero, s);
    else launch_one<W761EncU>(d_in, d_inf, d_out, d_st, n, ark_zero, s);
  } else if (group == 1) {
    if (compressed) launch_one<WireEncG2c>(d_in, d_inf, d_out, d_st, n, ark_zero, s);
    else launch_one<WireEncG2u>(d_in, d_inf, d_out, d_st, n, ark_zero, s);
  } else {
    if (compressed) launch_one<WireEncG1c>(d_in, d_inf, d_out, d_st, n, ark_zero, s);
    else launch_one<WireEncG1u>(d_in, d_inf, d_out, d_st, n, ark_zero, s);
  }
}

int wire_encode(int group, int compressed, const uint64_t* rows, const uint8_t* inf, size_t n, uint8_t* out, uint8_t* status, int dev, void* stream_) {
  // the argument checks need no device
  if (group < 0 || group > 2) return 2;
  if (n == 0) return 0;
  if (!rows || !out || !status || n > 0x7fffffffu) return 2;
  if (dev && (((uintptr_t)out | (uintptr_t)rows) & 7)) return 2;     // the kernels move 64-bit words
  if (int rc0 = api_enter()) return rc0;
  std::lock_guard<std::mutex> lk(wenc_mu);
  const size_t rw = group == 0 ? 12 : 24, ob = (group == 0 ? 48 : 96) * (compressed ? 1 : 2);
  CallScope cs;
  HIP_TRY(cs.open(dev, stream_), 10);
  const hipStream_t stream = cs.stream();
  uint64_t *d_in, *d_out;
  uint8_t *d_inf, *d_st;
  HIP_TRY(cs.in(&d_in, rows, n * rw * 8, dev), 10);
  HIP_TRY(cs.in(&d_inf, inf, n, dev), 10);
  HIP_TRY(cs.out(&d_out, out, n * ob, dev), 10);
  HIP_TRY(cs.out(&d_st, status, n, dev), 10);
  EvLog log(stream);
  const hipEvent_t e0 = log.open();
  launch_encode(group, compressed, d_in, d_inf, d_out, d_st, n, 0, stream);
  HIP_TRY(hipGetLastError(), 10);
  log.close(0, e0);
  HIP_TRY(cs.copy_back(), 10);
  HIP_TRY(hipStreamSynchronize(stream), 10);
  float ms = 0.f;
  log.sum(&ms);
  g_wenc_last.note(ms);
  return 0;
}
float wire_encode_last_ms() { return g_wenc_last.read(); }
void wire_encode_key_timings(float ms[3]) { const CallTimes t = g_wenc_key_last.read(); for (int i = 0; i < 3; i++) ms[i] = t.ms[i]; }

int wire_key_size(int curve, size_t n_inputs, size_t n_vars, size_t n_h, int form, int vk_only, uint64_t* len) { return wkey_size(curve, n_inputs, n_vars, n_h, form, vk_only, len); }

// ProvingKey::<E>::serialize (form 0) / serialize_uncompressed (1), or VerifyingKey's when rows == NULL, from the out_vk / out_rows buffers of
// groth16_setup_<curve> (curve 0 = BW6-761: every row 24 u64; 1 = BLS12-377: G1 rows 12 u64, G2 rows - beta_g2, gamma_g2, delta_g2 and
// b_g2_query - 24).  Both buffers hold their rows in serialization order, so a point's position there is its index in the loader's index
// space.  The rows cross to the device once; each contiguous run of rows of one group (broken otherwise only by the Vec length fields) is one
// launch that writes straight to its byte offset - every offset is a multiple of 8 -; the bytes cross back once and the six length fields are
// filled in on the host.  A row (0, 1 in Montgomery form) is the identity here, as groth16_setup_* emits it and groth16_load_key_* reads it.
int wire_key_serialize(int curve, const uint64_t* vk, size_t n_inputs, const uint64_t* rows, size_t n_vars, size_t n_h, int form, uint8_t* out, size_t cap,
                       uint64_t* out_len, uint64_t* first_bad) {
  if (!vk || !out_len) return 2;
  uint64_t need = 0;
  if (int rcs = wkey_size(curve, n_inputs, n_vars, n_h, form, rows == nullptr, &need)) return rcs;
  *out_len = need;
  if (cap < need) return W761_ERR_CAPACITY;
  if (!out) return 2;
  const uint64_t P = wkey_g1_bytes(curve, form), P2 = wkey_g2_bytes(curve, form), w1 = curve ? 12 : 24, w2 = 24;   // bytes and u64 per G1 / G2 point
  const uint64_t n_vk = 4 + (uint64_t)n_inputs, n_l = rows ? n_vars - n_inputs : 0;
  const uint64_t n_rows = rows ? 2 + 3 * (uint64_t)n_vars + n_h + n_l : 0, N = n_vk + n_rows;
  if (N > 0x7fffffffu) return 2;
  if (int rc0 = api_enter()) return rc0;
  std::lock_guard<std::mutex> lk(wenc_mu);
  // the runs: {first point, its first word in the row buffer, points, byte offset}; a Vec's length field sits in the 8 bytes before its run
  struct Run { uint64_t pt, word, n, off; bool vec, g2; };
  Run runs[9];
  int nr = 0;
  uint64_t pos = 0, pt = 0, word = 0;
  auto add = [&](uint64_t cnt, bool vec, bool g2) {
    if (vec) pos += 8;
    runs[nr++] = {pt, word, cnt, pos, vec, g2};
    pt += cnt;
    word += cnt * (g2 ? w2 : w1);
    pos += cnt * (g2 ? P2 : P);
  };
  add(1, false, false);          // alpha_g1
  add(3, false, true);           // beta_g2, gamma_g2, delta_g2
  add(n_inputs, true, false);    // gamma_abc_g1
  const uint64_t vk_words = word;
  if (rows) {
    add(2, false, false);        // beta_g1, delta_g1
    add(n_vars, true, false);    // a_query
    add(n_vars, true, false);    // b_g1_query
    add(n_vars, true, true);     // b_g2_query
    add(n_h, true, false);       // h_query
    add(n_l, true, false);       // l_query
  }
  CallScope cs(nullptr);
  HIP_TRY(cs.create_stream(), 10);
  const hipStream_t stream = cs.stream();
  hipEvent_t ev[4];
  for (auto& e : ev) HIP_TRY(cs.event(&e), 10);
  uint64_t* d_rows;
  uint8_t *d_out, *d_st;
  unsigned long long* d_first;
  unsigned long long first = ~0ull;
  HIP_TRY(cs.alloc(&d_rows, word * 8), 10);
  HIP_TRY(cs.alloc(&d_out, need), 10);
  HIP_TRY(cs.alloc(&d_st, N), 10);
  HIP_TRY(cs.alloc(&d_first, sizeof first), 10);
  HIP_TRY(hipEventRecord(ev[0], stream), 10);
  HIP_TRY(hipMemcpyAsync(d_rows, vk, vk_words * 8, hipMemcpyHostToDevice, stream), 10);
  if (rows) HIP_TRY(hipMemcpyAsync(d_rows + vk_words, rows, (word - vk_words) * 8, hipMemcpyHostToDevice, stream), 10);
  HIP_TRY(hipMemcpyAsync(d_first, &first, sizeof first, hipMemcpyHostToDevice, stream), 10);
  HIP_TRY(hipEventRecord(ev[1], stream), 10);
  for (int r = 0; r < nr; r++) {
    if (!runs[r].n) continue;
    launch_encode(curve ? (runs[r].g2 ? 1 : 0) : 2, form == 0, d_rows + runs[r].word, nullptr, (uint64_t*)(d_out + runs[r].off), d_st + runs[r].pt, runs[r].n, 1, stream);
    HIP_TRY(hipGetLastError(), 10);
  }
  hipLaunchKernelGGL(k_first_bad_encode, dim3(((uint32_t)N + 255) / 256), dim3(256), 0, stream, d_st, (uint32_t)N, d_first);
  HIP_TRY(hipGetLastError(), 10);
  HIP_TRY(hipEventRecord(ev[2], stream), 10);
  HIP_TRY(hipMemcpyAsync(&first, d_first, sizeof first, hipMemcpyDeviceToHost, stream), 10);
  HIP_TRY(hipStreamSynchronize(stream), 10);
  if (first != ~0ull) {                              // nothing is written to `out`
    if (first_bad) *first_bad = first;
    return W761_ERR_POINT;
  }
  HIP_TRY(hipMemcpyAsync(out, d_out, need, hipMemcpyDeviceToHost, stream), 10);
  HIP_TRY(hipEventRecord(ev[3], stream), 10);
  HIP_TRY(hipStreamSynchronize(stream), 10);
  CallTimes t;
  for (int i = 0; i < 3; i++) HIP_TRY(hipEventElapsedTime(&t.ms[i], ev[i], ev[i + 1]), 10);
  g_wenc_key_last.note(t);
  g_wenc_last.note(t.ms[1]);
  for (int r = 0; r < nr; r++) {
    if (!runs[r].vec) continue;
    for (int b = 0; b < 8; b++) out[runs[r].off - 8 + b] = (uint8_t)(runs[r].n >> (8 * b));
  }
  return 0;
}

// Proof::<BW6_761>::serialize: A (G1), B (G2), C (G1) compressed, 3 x 96 B, from the arkworks Jacobian points groth16_prove_* returns.
// Host only: three points, through the same encoder.
int wire761_proof_serialize(const uint64_t* a_xyz, const uint64_t* b_xyz, const uint64_t* c_xyz, uint8_t* out) {
  if (!a_xyz || !b_xyz || !c_xyz || !out) return 2;
  const uint64_t* pts[3] = {a_xyz, b_xyz, c_xyz};
  for (int i = 0; i < 3; i++) {
    uint64_t w[12];
    (void)w761_encode_jacobian(pts[i], w);
    for (int j = 0; j < 96; j++) out[96 * i + j] = (uint8_t)(w[j >> 3] >> (8 * (j & 7)));
  }
  return 0;
}
// Proof::<Bls12_377>::serialize: A (G1, 48 B), B (G2, 96 B), C (G1, 48 B) compressed, from the arkworks Jacobian points groth16_prove_*
// returns (18 / 36 / 18 u64).  Host only, through the encoders of groups 0 / 1.
int wire377_proof_serialize(const uint64_t* a_xyz, const uint64_t* b_xyz, const uint64_t* c_xyz, uint8_t* out) {
  if (!a_xyz || !b_xyz || !c_xyz || !out) return 2;
  uint64_t w[24];
  (void)wire_encode_jacobian<Fq, WireEncG1c>(a_xyz, w);
  (void)wire_encode_jacobian<Fq2, WireEncG2c>(b_xyz, w + 6);
  (void)wire_encode_jacobian<Fq, WireEncG1c>(c_xyz, w + 18);
  for (int j = 0; j < 192; j++) out[j] = (uint8_t)(w[j >> 3] >> (8 * (j & 7)));
  return 0;
}
}  // namespace celo
