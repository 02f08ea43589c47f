// Seam A, the epoch side (seam.h has the map of the units): the bit encoders of an epoch block and the Groth16 `verify` over BW6-761.
#include "wire761.h"
#include "seam.h"

using namespace celo;
using namespace celo::seam;

namespace {
// ---------------------------------------------------------------- epoch encoding (crates/epoch-snark/src/{encoding,epoch_block}.rs,
// crates/bls-gadgets/src/utils.rs:2-56, crates/epoch-snark/src/gadgets/mod.rs:75-83) — byte/bit plumbing
typedef std::vector<uint8_t> Bits;
void bits_append_le(Bits& b, const uint8_t* bytes, size_t nbytes, size_t take) {  // bytes_le_to_bits_le
  for (size_t i = 0; i < take; i++) b.push_back(i / 8 < nbytes ? (bytes[i / 8] >> (i % 8)) & 1 : 0);
}
void bits_append_be(Bits& b, const uint8_t* bytes, size_t nbytes, size_t take) {  // bytes_le_to_bits_be: first `take` LE bits, reversed
  for (size_t i = take; i-- > 0;) b.push_back(i / 8 < nbytes ? (bytes[i / 8] >> (i % 8)) & 1 : 0);
}
std::vector<uint8_t> bits_be_to_bytes_le(const Bits& bits) {
  std::vector<uint8_t> out;
  size_t n = bits.size();
  for (size_t i = 0; i < n; i += 8) {
    uint8_t byte = 0;
    for (size_t k = 0; k < 8 && i + k < n; k++) byte |= (uint8_t)(bits[n - 1 - (i + k)] << k);
    out.push_back(byte);
  }
  return out;
}
void encode_uint(Bits& b, uint64_t v, size_t nbytes) {
  uint8_t le[8];
  for (size_t i = 0; i < 8; i++) le[i] = (uint8_t)(v >> (8 * i));
  bits_append_le(b, le, nbytes, 8 * nbytes);
}
void encode_public_key_bits(Bits& b, const Affine<Fq2_>& pk) {  // encoding.rs:23-47
  uint8_t x0[48], x1[48];
  fq_to_bytes(pk.x.c0, x0);
  fq_to_bytes(pk.x.c1, x1);
  bits_append_be(b, x0, 48, 377);
  bits_append_be(b, x1, 48, 377);
  bool over_half = wire_lex_largest(pk.y.c1) || (pk.y.c1.is_zero_mod_p() && wire_lex_largest(pk.y.c0));
  b.push_back(over_half ? 1 : 0);
}
void encode_entropy_bits(Bits& b, const uint8_t* entropy) {  // epoch_block.rs:140-148 (None -> zero bits)
  uint8_t zero[16];
  memset(zero, 0, 16);
  bits_append_le(b, entropy ? entropy : zero, 16, 128);
}
struct EpochBlockHost {
  uint16_t index; uint8_t round; const uint8_t* epoch_entropy; const uint8_t* parent_entropy;
  uint32_t maximum_non_signers; size_t maximum_validators; std::vector<Affine<Fq2_>> pubkeys; std::vector<uint64_t> pubkeys_jac;
};
Affine<Fq2_> g2_generator_affine() {
  return {{Fq_::from_limbs(T377::G2_GEN_X0), Fq_::from_limbs(T377::G2_GEN_X1)}, {Fq_::from_limbs(T377::G2_GEN_Y0), Fq_::from_limbs(T377::G2_GEN_Y1)}};
}
void epoch_bits_cip22(const EpochBlockHost& e, bool first, Bits& b) {  // epoch_block.rs:118-138
  encode_uint(b, e.index, 2);
  encode_entropy_bits(b, first ? e.parent_entropy : e.epoch_entropy);
  encode_uint(b, e.maximum_non_signers, 4);
  for (const auto& pk : e.pubkeys) encode_public_key_bits(b, pk);
  for (size_t i = e.pubkeys.size(); i < e.maximum_validators; i++) encode_public_key_bits(b, g2_generator_affine());
}
std::vector<uint8_t> blake2s_out_domain(const std::vector<uint8_t>& data) {  // epoch_block.rs:226-236, OUT_DOMAIN = "ULforout"
  static const uint8_t OUT_DOMAIN[8] = {'U', 'L', 'f', 'o', 'r', 'o', 'u', 't'};
  B2sParams p;
  return blake2s(data.data(), data.size(), p, OUT_DOMAIN, 8);
}
bool epoch_from_ffi(const EpochBlockFFI& src, EpochBlockHost& e) {  // snark/epoch_block.rs:129-146
  e.index = src.index; e.round = src.round; e.epoch_entropy = src.epoch_entropy; e.parent_entropy = src.parent_entropy;
  e.maximum_non_signers = src.maximum_non_signers; e.maximum_validators = src.maximum_validators;
  e.pubkeys.resize(src.pubkeys_num);
  e.pubkeys_jac.resize(src.pubkeys_num * 36);
  // one square root in Fq2 + one subgroup check per key (~0.5 ms each): spread over the host cores for real validator sets
  std::atomic<bool> ok(true);
  auto decode = [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi && ok; i++) {
      bool inf;
      if (!g2_decompress(src.pubkeys + 96 * i, e.pubkeys[i], inf)) { ok = false; return; }
      if (inf) {      // read_pubkeys (snark/epoch_block.rs:187-196) takes G2Affine::deserialize's zero() as it comes: (0, 1), the identity in the sum
        e.pubkeys[i] = {Fq2_::zero(), Fq2_::one()};
        identity_jac<Fq2_>(&e.pubkeys_jac[i * 36]);
        continue;
      }
      if (!in_subgroup(e.pubkeys[i])) { ok = false; return; }
      affine_to_jac(e.pubkeys[i], &e.pubkeys_jac[i * 36]);
    }
  };
  unsigned nt = std::thread::hardware_concurrency();
  if (nt > 32) nt = 32;
  if (nt > src.pubkeys_num / 2) nt = (unsigned)(src.pubkeys_num / 2);
  if (nt < 1) nt = 1;
  if (nt > 1) (void)wire_consts();   // shared constants before the threads start
  run_on_threads(nt, [&](unsigned t) { decode(src.pubkeys_num * t / nt, src.pubkeys_num * (t + 1) / nt); });
  return ok;
}
}  // namespace

extern "C" {

// ---------------------------------------------------------------- Groth16 verification over BW6-761 through the FFI
// crates/bls-snark-sys/src/snark/mod.rs:23-45 -> crates/epoch-snark/src/api/verifier.rs:23-40 -> ark_groth16::verify_proof.
// Decoding, hashing and packing are host plumbing; the two input scalar-muls go through msm_bw6_761_g1 and the check
//   e(A,B) * e(acc,-gamma) * e(C,-delta) * e(-alpha,beta) == 1   through pairing_product_is_one_bw6_761 (GPU).
bool verify(const uint8_t* vk, uint32_t vk_len, const uint8_t* proof, uint32_t proof_len, EpochBlockFFI first_epoch, EpochBlockFFI last_epoch) {
  if (!vk || !proof || proof_len < 288 || vk_len < 392) return false;
  PhaseLog ph("verify");
  // ---- VerifyingKey = alpha_g1 | beta_g2 | gamma_g2 | delta_g2 | u64 len | gamma_abc_g1[len];  Proof = A | B | C
  uint64_t nabc;
  memcpy(&nabc, vk + 384, 8);
  if (nabc != 3 || vk_len < 392 + 96 * nabc) { log_err("verify: vk must carry 2 public inputs"); return false; }
  // ten BW6-761 decodings (GroupAffine::deserialize: a 761-bit square root and the r P == O ladder each, wire761.h) and the two blocks'
  // validator keys: independent, so they share the host cores instead of queueing on one (they were a fifth of the call).  The points
  // land in the rows of the input MSM (gamma_abc) and of the product e(A,B) e(acc,-gamma) e(C,-delta) e(-alpha,beta); infinity is rejected.
  EpochBlockHost first, last;
  uint64_t bases[3 * 24], g1[4 * 24], g2[4 * 24];
  const uint8_t* src[10] = {vk, vk + 96, vk + 192, vk + 288, vk + 392, vk + 488, vk + 584, proof, proof + 96, proof + 192};
  uint64_t* const row[10] = {g1 + 72, g2 + 72, g2 + 24, g2 + 48, bases, bases + 24, bases + 48, g1, g2, g1 + 48};   // alpha, beta, gamma, delta, abc[0..2], A, B, C
  const bool on_g2[10] = {false, true, true, true, false, false, false, false, true, false};
  bool okp[10], ok_first = false, ok_last = false;
  {
    std::vector<std::thread> th;
    th.emplace_back([&]() { ok_first = epoch_from_ffi(first_epoch, first); });
    th.emplace_back([&]() { ok_last = epoch_from_ffi(last_epoch, last); });
    for (int i = 0; i < 10; i++)
      th.emplace_back([&, i]() { okp[i] = (on_g2[i] ? w761_decode_row<4, true>(src[i], true, row[i]) : w761_decode_row<-1, true>(src[i], true, row[i])) == WIRE_OK; });
    for (auto& x : th) x.join();
  }
  if (!ok_first || !ok_last) { log_err("verify: bad epoch public keys"); return false; }
  for (int i = 0; i < 10; i++) if (!okp[i]) { log_err(i < 7 ? "verify: bad vk" : "verify: bad proof"); return false; }
  for (uint64_t* r : {row[2], row[3], row[0]}) w761_neg(Fw761::from_ark(r + 12)).to_ark(r + 12);      // -gamma, -delta, -alpha
  // ---- public inputs: Blake2s("ULforout") of the first epoch and of the last epoch + aggregated key, 512 bits, packed 376|136
  Bits fb, lb;
  epoch_bits_cip22(first, true, fb);
  epoch_bits_cip22(last, false, lb);
  uint64_t agg[36];
  if (celo_amd_sum_jacobian_bls12_377_g2(last.pubkeys_jac.data(), last.pubkeys.size(), agg) != 0) return false;
  encode_public_key_bits(lb, jac_to_affine_or_zero<Fq2_>(agg));   // (an aggregate that is the identity encodes as arkworks' zero(), as in the reference)
  std::vector<uint8_t> h1 = blake2s_out_domain(bits_be_to_bytes_le(fb)), h2 = blake2s_out_domain(bits_be_to_bytes_le(lb));
  Bits hb;
  bits_append_le(hb, h1.data(), 32, 256);
  bits_append_le(hb, h2.data(), 32, 256);
  uint64_t scalars[3 * 6];
  memset(scalars, 0, sizeof scalars);
  scalars[0] = 1;  // gamma_abc[0] enters with scalar 1
  for (int chunk = 0; chunk < 2; chunk++) {  // pack::<Fr, CAPACITY = 376>: big-endian bits
    size_t lo = chunk * 376, hi = lo + 376 < hb.size() ? lo + 376 : hb.size();
    uint64_t* sc = scalars + 6 * (chunk + 1);
    size_t nb = hi - lo;
    for (size_t i = 0; i < nb; i++)
      if (hb[lo + i]) { size_t bit = nb - 1 - i; sc[bit >> 6] |= 1ULL << (bit & 63); }
  }
  uint64_t accj[36];
  ph.mark("decode keys, vk, proof; public inputs");
  if (msm_bw6_761_g1(bases, nullptr, scalars, 3, accj) != 0) return false;
  ph.mark("3-term input MSM (GPU)");
  // ---- the 4-pair product (acc the second G1 row)
  uint8_t i1[4] = {0, 0, 0, 0}, i2[4] = {0, 0, 0, 0};
  batch_to_affine<Fw761>(accj, 1, g1 + 24, &i1[1]);
  int one = 0;
  if (pairing_product_is_one_bw6_761(g1, i1, g2, i2, 4, &one) != 0) return false;
  ph.mark("4-pair product check (GPU)");
  return one != 0;
}

static bool collect_pubkeys(const PublicKey* const* in, int n, std::vector<Affine<Fq2_>>& out) {
  if (n < 0 || (n > 0 && !in)) return false;
  out.resize((size_t)n);
  for (int i = 0; i < n; i++) {
    if (!in[i]) return false;
    out[(size_t)i] = jac_to_affine_or_zero<Fq2_>(in[i]->xyz);
  }
  return true;
}
bool encode_epoch_block_to_bytes_cip22(unsigned short index, unsigned char round, const uint8_t* epoch_entropy, const uint8_t* parent_entropy,
                                       unsigned int maximum_non_signers, unsigned int maximum_validators, const PublicKey* const* added_public_keys,
                                       int added_public_keys_len, uint8_t** out_bytes, int* out_len, uint8_t** out_extra, int* out_extra_len) {
  if (!out_bytes || !out_len || !out_extra || !out_extra_len) return false;                                  /* snark/epoch_block.rs:17 */
  std::vector<Affine<Fq2_>> pks;
  if (!collect_pubkeys(added_public_keys, added_public_keys_len, pks)) return false;
  Bits eb, xb;                                                                                                /* epoch_block.rs:150-169 */
  encode_uint(xb, index, 2); encode_uint(xb, round, 1); encode_uint(xb, maximum_non_signers, 4);
  encode_entropy_bits(eb, epoch_entropy);
  encode_entropy_bits(eb, parent_entropy);
  for (const auto& pk : pks) encode_public_key_bits(eb, pk);
  for (size_t i = pks.size(); i < maximum_validators; i++) encode_public_key_bits(eb, g2_generator_affine());
  return emit(bits_be_to_bytes_le(eb), out_bytes, out_len) && emit(bits_be_to_bytes_le(xb), out_extra, out_extra_len);
}
bool encode_epoch_block_to_bytes(unsigned short index, unsigned int maximum_non_signers, const PublicKey* const* added_public_keys,
                                 int added_public_keys_len, uint8_t** out_bytes, int* out_len) {              /* snark/epoch_block.rs:69 */
  if (!out_bytes || !out_len) return false;
  std::vector<Affine<Fq2_>> pks;
  if (!collect_pubkeys(added_public_keys, added_public_keys_len, pks)) return false;
  Bits b;                                                                                                     /* epoch_block.rs:106-114 */
  encode_uint(b, index, 2); encode_uint(b, maximum_non_signers, 4);
  for (const auto& pk : pks) encode_public_key_bits(b, pk);
  return emit(bits_be_to_bytes_le(b), out_bytes, out_len);
}
}
