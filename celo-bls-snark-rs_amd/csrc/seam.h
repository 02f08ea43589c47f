// Seam A: the bls-snark-sys C ABI, rebuilt on top of the gfx950 hot path.
//
// The seam_*.hip units provide all 36 symbols of `crates/bls-snark-sys/src/{serialization,signatures}.rs` and `src/snark/{mod,epoch_block}.rs`
// under their reference names: opaque PrivateKey / PublicKey / Signature handles, arkworks CanonicalSerialize encodings,
// aggregate_*, both hashers (Blake2Xs try-and-increment, the Bowe-Hopwood composite hasher, before and after CIP22),
// sign_* / verify_* / batch_verify_*, the Groth16 `verify` and the epoch encoders.  Everything in them is host orchestration:
// group arithmetic on the hot path (MSM, pairings, bulk hashing from 256 messages up) goes to the kernels through the
// Seam B entry points, the rest (one decompression, one subgroup check, one hash) is latency-path plumbing on the host.
//
//   seam_handles.hip   the handle arenas, key generation, (de)serialisation, destructors, aggregate_*, init
//   seam_hash.hip      Blake2s / Blake2Xs, the Bowe-Hopwood CRH, hash-to-G1, hash_* / sign_* / verify_signature / verify_pop
//   seam_strict.hip    batch_verify_signature and batch_verify_strict (the per-device mirrors of the arenas)
//   seam_epoch.hip     the epoch bit encoders and the Groth16 `verify`
//
// This header is internal to those four units and declares every helper that crosses them ONCE (the rule of units.h); what a unit
// keeps to itself sits in an anonymous namespace there.  The small templates are defined here, so the single-call path inlines them.
//
// Ownership mirrors the reference: handles come from new/delete behind destroy_*; byte buffers are malloc'd and released
// by free_vec(ptr, len) (crates/bls-snark-sys/src/serialization.rs:120-140, 224-268).  Every entry returns `false`
// instead of unwinding (convert_result_to_bool, crates/bls-snark-sys/src/lib.rs:21-27).
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <cstdio>
#include <chrono>
#include <mutex>
#include <vector>
#include <thread>
#include <atomic>
#include <hip/hip_runtime.h>
#include "curve.h"
#include "fp2.h"
#include "wire.h"
#include "runtime.h"
#include "units.h"
#include "../../include/celo_bls_amd.h"
#include "../../include/celo_bls_snark_sys.h"

typedef celo::Fp<celo::P377> Fq_;
typedef celo::Fp2<celo::P377> Fq2_;

struct PrivateKey { uint64_t k[4]; };          // Fr, canonical
// PublicKey / Signature handles live in ARENAS (seam_handles.hip HandleArena): a handle is its slot of the arena plus the serial number of the
// allocation that filled the slot.  batch_verify_strict keeps a per-device mirror of the arenas' points in HBM (affine, one entry per
// slot, tagged with the serial it was uploaded for), so a call over handles the device has already seen ships 4-byte slot numbers, not
// 320 bytes per signer: validator keys recur epoch after epoch (the reason the reference memoises their decompression,
// crates/bls-crypto/src/bls/cache.rs:36), and the handle types are opaque to every caller.
struct PublicKey { uint64_t xyz[36]; uint64_t serial; uint32_t slot; };         // G2 Jacobian, arkworks Montgomery limbs (GroupProjective<g2>)
struct Signature { uint64_t xyz[18]; uint64_t serial; uint32_t slot; };         // G1 Jacobian

namespace celo {
namespace seam {
// errors are logged and mapped to `false` like the reference's convert_result_to_bool (log::error! + false)
inline void log_err(const char* what) { if (getenv("CELO_AMD_LOG")) fprintf(stderr, "[celo-amd] %s\n", what); }
const uint64_t R_ORDER[4] = {0x0a11800000000001ULL, 0x59aa76fed0000001ULL, 0x60b44d1e5c37b001ULL, 0x12ab655e9a2ca556ULL};
const uint8_t SIG_DOMAIN[8] = {'U', 'L', 'f', 'o', 'r', 'x', 'o', 'f'};  // crates/bls-crypto/src/lib.rs:75
const uint8_t POP_DOMAIN[8] = {'U', 'L', 'f', 'o', 'r', 'p', 'o', 'p'};  // lib.rs:78
inline bool hash_flags_supported(bool composite, bool cip22) {
  if (!composite && cip22) { log_err("(composite=false, cip22=true) is rejected by the reference too (signatures.rs:61)"); return false; }
  return true;
}
// comparisons, byte decoding, signs, square roots and the subgroup check live in wire.h / wire761.h (shared with the bulk GPU kernels of
// unit_wire.hip / unit_wire761.hip)
inline void fq_to_bytes(const Fq_& a, uint8_t* out) {
  uint64_t w[6];
  a.to_canonical(w);
  memcpy(out, w, 48);
}
struct B2sParams { uint8_t digest_length = 32, fanout = 1, depth = 1, node_depth = 0, inner_length = 0; uint32_t leaf_length = 0; uint64_t node_offset = 0; };
struct ChaCha20Rng {  // rand_chacha 0.2 behind rand_core 0.5 BlockRng: 64-word buffer (4 blocks), 64-bit block counter
  uint32_t key[8]; uint64_t counter = 0; uint32_t buf[64]; int idx = 64;
  static uint32_t rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }
  void block(uint32_t* out) {
    uint32_t s[16] = {0x61707865u, 0x3320646Eu, 0x79622D32u, 0x6B206574u, key[0], key[1], key[2], key[3], key[4], key[5], key[6], key[7],
                      (uint32_t)counter, (uint32_t)(counter >> 32), 0, 0};
    uint32_t w[16];
    memcpy(w, s, sizeof w);
#define CC_QR(a, b, c, d) w[a] += w[b]; w[d] = rotl(w[d] ^ w[a], 16); w[c] += w[d]; w[b] = rotl(w[b] ^ w[c], 12); \
                          w[a] += w[b]; w[d] = rotl(w[d] ^ w[a], 8);  w[c] += w[d]; w[b] = rotl(w[b] ^ w[c], 7);
    for (int r = 0; r < 10; r++) {
      CC_QR(0, 4, 8, 12) CC_QR(1, 5, 9, 13) CC_QR(2, 6, 10, 14) CC_QR(3, 7, 11, 15)
      CC_QR(0, 5, 10, 15) CC_QR(1, 6, 11, 12) CC_QR(2, 7, 8, 13) CC_QR(3, 4, 9, 14)
    }
#undef CC_QR
    for (int i = 0; i < 16; i++) out[i] = w[i] + s[i];
    counter++;
  }
  void generate() { for (int b = 0; b < 4; b++) block(buf + 16 * b); idx = 0; }
  uint32_t next_u32() { if (idx >= 64) generate(); return buf[idx++]; }
  uint64_t next_u64() {
    if (idx < 63) { uint64_t v = ((uint64_t)buf[idx + 1] << 32) | buf[idx]; idx += 2; return v; }
    if (idx >= 64) { generate(); uint64_t v = ((uint64_t)buf[1] << 32) | buf[0]; idx = 2; return v; }
    uint64_t lo = buf[63]; generate(); uint64_t hi = buf[0]; idx = 1; return (hi << 32) | lo;
  }
};
struct HashJob { const uint8_t* msg; size_t mlen; const uint8_t* extra; size_t elen; uint64_t* out_xy; };
struct PhaseLog {  // CELO_AMD_LOG=1: wall time of the host / device phases of one FFI call
  const char* fn; bool on; std::chrono::steady_clock::time_point t;
  explicit PhaseLog(const char* f) : fn(f), on(getenv("CELO_AMD_LOG") != nullptr), t(std::chrono::steady_clock::now()) {}
  void mark(const char* what) {
    if (!on) return;
    auto n = std::chrono::steady_clock::now();
    fprintf(stderr, "[celo-amd] %s: %-28s %9.3f ms\n", fn, what, std::chrono::duration<double, std::milli>(n - t).count());
    t = n;
  }
};

// ---- helpers that one unit defines and another calls
// seam_handles.hip
PublicKey* new_public_key();
Signature* new_signature();
bool drop(PublicKey* p);
bool drop(Signature* p);
uint32_t public_key_high_water();               // slots the arenas have handed out so far
uint32_t signature_high_water();
bool emit(const std::vector<uint8_t>& v, uint8_t** out_bytes, int* out_len);
bool g1_decompress(const uint8_t* in, Affine<Fq_>& p, bool& inf);
void g1_compress(const Affine<Fq_>& p, bool inf, uint8_t* out);
bool g2_decompress(const uint8_t* in, Affine<Fq2_>& p, bool& inf);
void g2_compress(const Affine<Fq2_>& p, bool inf, uint8_t* out);
bool os_seeded_rng(ChaCha20Rng& rng);
// seam_hash.hip
std::vector<uint8_t> blake2s(const uint8_t* data, size_t len, const B2sParams& p, const uint8_t* personal, size_t plen);
bool hash_to_g1(bool composite, bool cip22, const uint8_t* dom, const uint8_t* msg, size_t mlen, const uint8_t* extra, size_t elen,
                Affine<Fq_>& out, int& attempt, Affine<Fq_>* pre_cofactor = nullptr);
bool hash_many(bool composite, bool cip22, const uint8_t* dom, std::vector<HashJob>& jobs, std::vector<uint8_t>* failed = nullptr);
void neg_g2_generator(uint64_t out_xy[24]);

// fn(t) for t = 0 ... nt - 1, each on a thread of its own; one range (or none) runs on the calling thread
template <class Fn> void run_on_threads(unsigned nt, Fn fn) {
  if (nt <= 1) { fn(0u); return; }
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; t++) th.emplace_back(fn, t);
  for (auto& x : th) x.join();
}

// ---- group helpers on the host (plumbing: one decompression / subgroup check / small sums)
template <class F> Xyzz<F> scalar_mul_host(const Affine<F>& p, const uint64_t* k, int nlimbs) {
  Xyzz<F> acc = Xyzz<F>::identity();
  for (int i = nlimbs * 64 - 1; i >= 0; i--) {
    acc = xyzz_dbl(acc);
    if ((k[i >> 6] >> (i & 63)) & 1) xyzz_madd(acc, p);
  }
  return acc;
}
template <class F> bool in_subgroup(const Affine<F>& p) { return wire_in_subgroup(p, wire_consts()); }
template <class F> void affine_to_jac(const Affine<F>& p, uint64_t* out) {
  constexpr int A = F::ARK64;
  p.x.to_ark(out);
  p.y.to_ark(out + A);
  F::one().to_ark(out + 2 * A);
}
template <class F> void identity_jac(uint64_t* out) {
  constexpr int A = F::ARK64;
  F::zero().to_ark(out);
  F::one().to_ark(out + A);
  F::zero().to_ark(out + 2 * A);
}
// Jacobian (ark limbs) -> affine; returns false for the identity
template <class F> bool jac_to_affine(const uint64_t* jac, Affine<F>& out) {
  constexpr int A = F::ARK64;
  F Z = F::from_ark(jac + 2 * A);
  if (Z.is_zero_mod_p()) return false;
  F zi = F::inv(Z);
  F zi2 = F::sqr(zi);
  out.x = F::norm(F::mul(F::from_ark(jac), zi2));
  out.y = F::norm(F::mul(F::from_ark(jac + A), F::mul(zi2, zi)));
  return true;
}
// ... and for callers that must carry the identity the way arkworks does: GroupAffine::zero() is (x, y, infinity) = (0, 1, true), and the
// reference's encode_public_key (crates/epoch-snark/src/encoding.rs:23-47) reads x and y of whatever into_affine() returned - for the identity
// 754 zero bits and a clear sign bit.  (It documents "not the point at infinity" as an assumption and does not check it.)
template <class F> Affine<F> jac_to_affine_or_zero(const uint64_t* jac) {
  Affine<F> out;
  if (!jac_to_affine<F>(jac, out)) out = {F::zero(), F::one()};
  return out;
}
// Jacobian (ark limbs, stride 3*A u64) -> affine xy (ark limbs); inf[i] = 1 for the identity.  Handles that came from the wire
// (deserialize_*) carry Z = 1 and are copied without arithmetic; the rest share one inversion per chunk (Montgomery's
// trick); large inputs are cut into chunks across the host cores (at BASELINE config 3's scale - 10^6 keys and signatures
// per call - a serial pass here would cost 30x the GPU work it feeds).
template <class F> void batch_to_affine_range(const uint64_t* jac, size_t n, uint64_t* xy, uint8_t* inf) {
  constexpr int A = F::ARK64;
  uint64_t one_ark[A];
  F::one().to_ark(one_ark);
  std::vector<uint32_t> todo;
  for (size_t i = 0; i < n; i++) {
    const uint64_t* zp = jac + i * 3 * A + 2 * A;
    if (memcmp(zp, one_ark, A * 8) == 0) { memcpy(xy + i * 2 * A, jac + i * 3 * A, 2 * A * 8); inf[i] = 0; continue; }
    bool zero = true;
    for (int k = 0; k < A; k++) zero = zero && zp[k] == 0;
    if (zero) { memset(xy + i * 2 * A, 0, 2 * A * 8); inf[i] = 1; continue; }
    todo.push_back((uint32_t)i);
  }
  if (todo.empty()) return;
  std::vector<F> z(todo.size()), pre(todo.size());
  F acc = F::one();
  for (size_t t = 0; t < todo.size(); t++) {
    z[t] = F::norm(F::from_ark(jac + (size_t)todo[t] * 3 * A + 2 * A));
    inf[todo[t]] = z[t].is_zero_mod_p() ? 1 : 0;     // a non-canonical zero cannot come from this library; handled anyway
    pre[t] = acc;
    if (!inf[todo[t]]) acc = F::mul(acc, z[t]);
  }
  F ai = F::inv(acc);
  for (size_t t = todo.size(); t-- > 0;) {
    const size_t i = todo[t];
    uint64_t* o = xy + i * 2 * A;
    if (inf[i]) { memset(o, 0, 2 * A * 8); continue; }
    F zi = F::mul(ai, pre[t]);
    ai = F::mul(ai, z[t]);
    F zi2 = F::sqr(zi);
    F::mul(F::from_ark(jac + i * 3 * A), zi2).to_ark(o);
    F::mul(F::from_ark(jac + i * 3 * A + A), F::mul(zi2, zi)).to_ark(o + A);
  }
}
template <class F> void batch_to_affine(const uint64_t* jac, size_t n, uint64_t* xy, uint8_t* inf) {
  constexpr int A = F::ARK64;
  unsigned nt = std::thread::hardware_concurrency();
  if (nt > 64) nt = 64;
  if (n < 4096 || nt < 2) { batch_to_affine_range<F>(jac, n, xy, inf); return; }
  const size_t chunk = (n + nt - 1) / nt;
  run_on_threads((unsigned)((n + chunk - 1) / chunk), [=](unsigned t) {
    const size_t lo = (size_t)t * chunk, hi = lo + chunk < n ? lo + chunk : n;
    batch_to_affine_range<F>(jac + lo * 3 * A, hi - lo, xy + lo * 2 * A, inf + lo);
  });
}
}  // namespace seam
}  // namespace celo
