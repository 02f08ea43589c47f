// Groth16 verification for many proofs under one verifying key (ark_groth16::prepare_verifying_key + verify_proof), over BW6-761
// (crates/epoch-snark/src/api/verifier.rs:35) and over BLS12-377 (the hash-helper proof of crates/epoch-snark/src/api/prover.rs:83-118):
// the curve descriptions, the lane routines of groth16_verify_unit.h's kernels as host+device templates, and the host parse of a serialized
// VerifyingKey.  The kernels and the host twins of host_test.cpp (-DCELO_FP_TRACK) run the same code.
//
//   acc_i = abc_0 + sum_j x_ij abc_j     g16_input_row: one signed-digit window table per input base (fixed_base.h, generalised from one
//                                        generator to n_abc - 1 bases), one mixed addition per non-zero digit, no doublings
//   r_i A_i                              g16_scale128: a 128-bit exponent whose top bit is set, MSB-first over XYZZ (wire761.h's ladder shape)
// DESIGN.md section 6h.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "aggregate.h"
#include "fixed_base.h"
#include "wire761.h"

namespace celo {

constexpr size_t G16_MAX_INPUTS = 64;                 // n_abc - 1; more is refused with G16_ERR_INPUTS
constexpr size_t G16_MAX_INPUTS_WIDE = 1024;          // the same for the wide loaders of BLS12-377: at 4 window bits their tables fill the budget exactly
constexpr int G16_ERR_INPUTS = 36;                    // (30 .. 35: the serialized-key and R1CS codes of wire761.h / r1cs.h)
constexpr size_t G16_TABLE_BUDGET = size_t(64) << 20; // bytes of window tables per key
constexpr int G16_C_MAX = 10, G16_C_MIN = 4;

// ---- what the verifier needs to know of a curve.  F / F2: the coordinate fields of G1 / G2; G1W / G2W: u64 of an affine row of arkworks
// limbs; N64: limbs of a scalar; order() / SCALAR_BITS: r, the order of the groups; G1_BYTES / G2_BYTES: a compressed point.
// decode_g1 / decode_g2: one compressed point, checked as GroupAffine::deserialize checks it (host side of the key parse).
struct G16Bw6 {
  typedef Fw761 F;
  typedef Fw761 F2;
  static constexpr int ID = 0, G1W = 24, G2W = 24, N64 = 6, SCALAR_BITS = 377, G1_BYTES = 96, G2_BYTES = 96;
  HD static const uint64_t* order() { return P377::P64; }
  static WireStatus decode_g1(const uint8_t* in, uint64_t* row) { return w761_decode_row<-1, true>(in, true, row); }
  static WireStatus decode_g2(const uint8_t* in, uint64_t* row) { return w761_decode_row<4, true>(in, true, row); }
};
struct G16Bls {
  typedef Fq F;
  typedef Fq2 F2;
  static constexpr int ID = 1, G1W = 12, G2W = 24, N64 = 4, SCALAR_BITS = 253, G1_BYTES = 48, G2_BYTES = 96;
  HD static const uint64_t* order() { return P253::P64; }
  static WireStatus decode_g1(const uint8_t* in, uint64_t* row) {
    Affine<Fq> p = {Fq::zero(), Fq::zero()};
    const WireStatus st = wire_decode_g1(in, wire_consts(), true, p);
    for (int j = 0; j < G1W; j++) row[j] = 0;
    if (st == WIRE_OK) { p.x.to_ark(row); p.y.to_ark(row + 6); }
    return st;
  }
  static WireStatus decode_g2(const uint8_t* in, uint64_t* row) {
    Affine<Fq2> p = {Fq2::zero(), Fq2::zero()};
    const WireStatus st = wire_decode_g2(in, wire_consts(), true, p);
    for (int j = 0; j < G2W; j++) row[j] = 0;
    if (st == WIRE_OK) { p.x.to_ark(row); p.y.to_ark(row + 12); }
    return st;
  }
};
// rows of the key and of a parsed key are KW u64 apart on both curves (a G1 row of BLS12-377 fills the first half of its slot)
constexpr int G16_KW = 24;

// bytes of the tables of n_in bases at c window bits: W 2^(c-1) affine entries of 2 x F::WORDS words each (28 for BW6-761; the 14 limbs
// of BLS12-377 are stored as 16 words, the field's own stored form)
template <class C> inline size_t g16_table_bytes(size_t n_in, int c) {
  return n_in * (size_t)fb_windows(C::SCALAR_BITS, c) * (size_t(1) << (c - 1)) * 2 * C::F::WORDS * 4;
}
// the widest window (fewest additions per input) whose tables stay within the budget.  BW6-761: 10 bits up to 15 inputs ... 7 bits at
// 64; BLS12-377: the last input count of 10 .. 4 bits is 39 | 70 | 128 | 221 | 381 | 642 | 1024 (the narrow loaders stop at 64)
template <class C> inline int g16_window_bits(size_t n_in) {
  int c = G16_C_MAX;
  while (c > G16_C_MIN && g16_table_bytes<C>(n_in, c) > G16_TABLE_BUDGET) c--;
  return c;
}

// 1 when s < m (N64 little-endian limbs), by the borrow of s - m: no branch
template <int N64> HD uint32_t g16_below(const uint64_t* s, const uint64_t* m) {
  uint64_t borrow = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int k = 0; k < N64; k++) {
    const uint64_t d = s[k] - m[k];
    const uint64_t b = (uint64_t)(s[k] < m[k]) | (uint64_t)(d < borrow);
    borrow = b;
  }
  return (uint32_t)borrow;
}

// acc += x T for one input x (N64 canonical limbs) and the table T of its base: fb_scalar_mul's loop on a running accumulator
template <class F, int N64> HD void g16_add_input(Xyzz<F>& acc, const uint64_t* s, const uint32_t* table, const uint8_t* tinf, int c, int W) {
  constexpr int FW = F::WORDS;
  const uint32_t H = 1u << (c - 1);
  uint32_t carry = 0;
  for (int j = 0; j < W; j++) {
    const int32_t d = fb_digit<N64>(s, j, c, carry);
    if (d == 0) continue;
    const uint32_t e = (uint32_t)j * H + (uint32_t)(d < 0 ? -d : d) - 1u;
    if (tinf[e]) continue;
    Affine<F> p = fb_load_entry<F>(table + (size_t)e * 2 * FW);
    if (d < 0) p = affine_neg(p);
    xyzz_madd(acc, p);
  }
}
// acc += x_j abc_j for input j of a proof (x: its inputs, N64 canonical limbs each): the range test, then the table walk.  An input that is
// not below r sets bit 0 of b and enters as zero.
template <class C>
HD void g16_take_input(Xyzz<typename C::F>& acc, const uint64_t* x, uint32_t j, const uint32_t* table, const uint8_t* tinf, int c, int W, uint32_t& b) {
  typedef typename C::F F;
  constexpr int N64 = C::N64;
  const size_t E = (size_t)W << (c - 1);
  uint64_t s[N64];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int k = 0; k < N64; k++) s[k] = x[(size_t)j * N64 + k];
  const uint64_t keep = (uint64_t)0 - (uint64_t)g16_below<N64>(s, C::order());      // all ones when x < r
  b |= (uint32_t)(~keep & 1u);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int k = 0; k < N64; k++) s[k] &= keep;
  g16_add_input<F, N64>(acc, s, table + j * E * 2 * F::WORDS, tinf + j * E, c, W);
}
// One proof's input sum.  x: n_in inputs of N64 limbs; abc0: gamma_abc[0] as a table entry (2 F::WORDS canonical words), abc0_inf its
// identity flag; table / tinf: n_in tables of W 2^(c-1) entries, base-major.  An input that is not below r sets *bad and enters as zero.
template <class C>
HD Xyzz<typename C::F> g16_input_row(const uint64_t* x, uint32_t n_in, const uint32_t* abc0, bool abc0_inf, const uint32_t* table, const uint8_t* tinf, int c, int W, uint32_t* bad) {
  typedef typename C::F F;
  Xyzz<F> acc = Xyzz<F>::identity();
  if (!abc0_inf) acc = Xyzz<F>::from_affine(fb_load_entry<F>(abc0));
  uint32_t b = 0;
  for (uint32_t j = 0; j < n_in; j++) g16_take_input<C>(acc, x, j, table, tinf, c, W, b);
  *bad = b;
  return acc;
}

// ---- one input sum as the work of L lanes (k_g16_inputs_lanes), L a power of two from 2 to G16_MAX_LANES; aggregate.h's two phases:
//   phase 1   lane l sums the inputs j = l, l + L, ..; lane 0 starts from gamma_abc[0]; a lane without inputs carries the identity;
//   phase 2   the round of stride s = L/2 .. 1: lanes [s, 2 s) store their partial into slot lane - s (g16_fold_put), and when those stores
//             have landed lanes [0, s) add the partial of slot `lane` with a full addition that reads it where it lies (g16_fold_take).
// Only the upper half of a round's lanes stores, so a sum needs L/2 slots (at L = 256: 34 KiB of LDS where L slots would be 68 KiB), and a
// round's stores must wait for the previous round's reads of the same slots: two barriers a round.  Doubling (equal partials), cancelling
// (opposite ones) and the identity are live branches of the full addition.
constexpr uint32_t G16_MAX_LANES = 256;
HD bool g16_lanes_ok(int L) { return L >= 1 && L <= (int)G16_MAX_LANES && (L & (L - 1)) == 0; }
template <class C>
HD Xyzz<typename C::F> g16_lane_sum(const uint64_t* x, uint32_t n_in, uint32_t lane, uint32_t L, const uint32_t* abc0, bool abc0_inf, const uint32_t* table,
                                    const uint8_t* tinf, int c, int W, uint32_t* bad) {
  typedef typename C::F F;
  Xyzz<F> acc = Xyzz<F>::identity();
  if (lane == 0 && !abc0_inf) acc = Xyzz<F>::from_affine(fb_load_entry<F>(abc0));
  uint32_t b = 0;
  for (uint32_t j = lane; j < n_in; j += L) g16_take_input<C>(acc, x, j, table, tinf, c, W, b);     // (n_in <= 1024: j + L does not wrap)
  *bad = b;
  return acc;
}
// slots: the L/2 slots of this sum, agg_slot_words<F>() words each
template <class F> HD void g16_fold_put(uint32_t* slots, const Xyzz<F>& acc, uint32_t lane, uint32_t s) { agg_store<F>(slots + (size_t)(lane - s) * agg_slot_words<F>(), acc); }
template <class F> HD void g16_fold_take(Xyzz<F>& acc, const uint32_t* slots, uint32_t lane) { agg_add_stored<F>(acc, slots + (size_t)lane * agg_slot_words<F>()); }

// The lanes per sum of a call of m proofs under a key of n_in inputs, in the shape of agg_pick_lanes:
//   L = min( G16_MAX_LANES, smallest power of two >= n_in / G16_INPUTS_PER_LANE, largest power of two <= G16_FILL_LANES / m ), at least 1
// and 1 (k_g16_inputs, the kernel every narrow key has always run) for a key of at most G16_MAX_INPUTS inputs.
// The input sums are latency-bound: one lane takes about 9.7 us per dependent mixed addition, so the time falls as 1 / L until every lane
// has one input, and a lane more than the inputs costs nothing but an idle lane and a fold round.  Both constants are read off a same-run
// A/B over all nine widths, every row of which is in profiles/bench_groth16_verify_wide.json (tools/bench_groth16_verify_wide.py; DESIGN.md
// 6h; kernel + normalisation in ms at L = 1 | 16 | 32 | 64 | 128 | 256, and the width the rule picks):
//   509 inputs, m = 1       241 | 16.8 | 8.48 | 4.23 | 2.24 | 1.27    rule 256
//   509 inputs, m = 64      244 | 16.2 | 8.35 | 4.38 | 2.40 | 1.42    rule 256
//   509 inputs, m = 1 024   244 | 16.3 | 8.57 | 4.97 | 4.64 | 4.60    rule 64
//   509 inputs, m = 4 096   244 | 17.2 | 15.8 | 15.5 | 15.7 | 15.5    rule 16
//   509 inputs, m = 16 384  247 | 57.8 | 57.0 | 56.9 | 58.4 | 57.9    rule 4
//   509 inputs, m = 65 536  250 | 214 | 214 | 216 | 222 | 222    rule 1
//    65 inputs, m = 1       20.3 | 1.82 | 1.20 | 0.85 | 0.55 | 0.54    rule 128
//    65 inputs, m = 64      18.3 | 1.84 | 1.31 | 1.03 | 0.67 | 0.71    rule 128
//    65 inputs, m = 1 024   18.3 | 1.86 | 1.50 | 1.48 | 1.01 | 1.47    rule 64
//    65 inputs, m = 4 096   18.2 | 2.37 | 2.48 | 3.02 | 2.89 | 3.92    rule 16
// G16_INPUTS_PER_LANE = 1: at 65 inputs 128 lanes (less than one input a lane) beat 64 at every batch size up to 1 024; at 509 inputs the
// cap of 256 lanes decides.  G16_FILL_LANES = 2^16 is one wave on every SIMD of the device, aggregate.h's figure, and the largest power
// of two under which a batch of 2^16 proofs runs one lane per proof, which the rule promises (tests/test_groth16_wide_host.py).  The table
// would admit 2^17: in every row where that changes the width it is level or ahead - by 1.07 to 1.10 x at 509 inputs from 1 024 proofs up,
// by 1.47 x (0.5 ms of a 5.9 ms call) at 65 inputs and 1 024 proofs.  Past 2^17 nothing is gained.
constexpr uint32_t G16_INPUTS_PER_LANE = 1;
constexpr uint32_t G16_FILL_LANES = 1u << 16;
inline uint32_t g16_pick_lanes(size_t n_in, size_t m) {
  if (n_in <= G16_MAX_INPUTS) return 1;
  uint32_t work = 1, fill = G16_MAX_LANES;
  while (work < G16_MAX_LANES && (uint64_t)work * G16_INPUTS_PER_LANE < n_in) work <<= 1;
  while (fill > 1 && (uint64_t)fill * m > G16_FILL_LANES) fill >>= 1;
  return work < fill ? work : fill;
}

// k p for k = 2^127 + (hi : lo without its top bit) - 128 bits, the top one always set, so the ladder starts from p and every exponent
// takes 127 doublings.  One group operation per turn and one doubling site, as w761_in_subgroup: stage 0 doubles, stage 1 adds p where
// bit i is set, stage 2 is the doubling that replaces an addition of acc == p (p of small order only).
template <class F> HD Xyzz<F> g16_scale128(const Affine<F>& p, uint64_t lo, uint64_t hi) {
  Xyzz<F> acc = Xyzz<F>::from_affine(p);
  int i = 126, stage = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  while (i >= 0) {
    if (stage == 1) {
      const uint64_t w = i >= 64 ? hi : lo;
      const bool bit = (w >> (i & 63)) & 1;
      if (!bit || xyzz_madd_unless_equal(acc, p)) { stage = 0; i--; continue; }
      stage = 2;
    }
    acc = xyzz_dbl(acc);
    if (stage == 2) { stage = 0; i--; }
    else stage = 1;
  }
  return acc;
}

// the exponent of proof i from the first 16 bytes of its ChaCha20 block (two little-endian u64): 2^127 | the low 127 bits
HD void g16_exponent(uint64_t w0, uint64_t w1, uint64_t& lo, uint64_t& hi) { lo = w0; hi = w1 | (1ull << 63); }

// arkworks' identity as a row of limbs of the field F (Fq2: c0 then c1 per coordinate): all zero (what the decoders and normalize_* write)
// or GroupAffine::zero() = (0, 1)
template <class F> inline bool g16_row_is_identity(const uint64_t* xy) {
  constexpr int A = F::ARK64;
  uint64_t one[A];
  F::one().to_ark(one);
  bool x0 = true, y0 = true, y1 = true;
  for (int k = 0; k < A; k++) { x0 = x0 && xy[k] == 0; y0 = y0 && xy[A + k] == 0; y1 = y1 && xy[A + k] == one[k]; }
  return x0 && (y0 || y1);
}
HD Fw761 g16_neg(const Fw761& a) { return w761_neg(a); }
HD Fq g16_neg(const Fq& a) { return wire_neg(a); }
HD Fq2 g16_neg(const Fq2& a) { return {wire_neg(a.c0), wire_neg(a.c1)}; }
template <class F> inline void g16_negate_row(uint64_t* xy) { g16_neg(F::from_ark(xy + F::ARK64)).to_ark(xy + F::ARK64); }

// ---- host: VerifyingKey::deserialize (compressed, checked):
//   alpha_g1 | beta_g2 | gamma_g2 | delta_g2 | u64 LE n_abc | gamma_abc_g1[n_abc]      96 B per point (BW6-761); 48 / 96 B (BLS12-377)
// rows: (4 + n_abc) x 24 u64 in that order, inf: their identity flags (the encoding of the point at infinity is a valid one).
// 2: a NULL pointer or n_abc == 0; 30 / 31: the bytes end early / go on after the last point; 36: more than max_inputs public inputs
// (G16_MAX_INPUTS, or G16_MAX_INPUTS_WIDE for the wide loaders); 33: a point that does not decode or lies outside the prime-order
// subgroup, *first_bad = its index in serialization order.
template <class C>
inline int g16_vk_parse(const uint8_t* bytes, size_t len, std::vector<uint64_t>& rows, std::vector<uint8_t>& inf, uint64_t* first_bad, size_t max_inputs = G16_MAX_INPUTS) {
  constexpr size_t B1 = C::G1_BYTES, B2 = C::G2_BYTES, HEAD = B1 + 3 * B2;
  if (!bytes) return 2;
  if (len < HEAD + 8) return W761_ERR_TRUNCATED;
  uint64_t n_abc = 0;
  for (int b = 7; b >= 0; b--) n_abc = (n_abc << 8) | bytes[HEAD + b];
  if (n_abc == 0) return 2;
  if (n_abc - 1 > max_inputs) return G16_ERR_INPUTS;
  if (len - (HEAD + 8) < B1 * n_abc) return W761_ERR_TRUNCATED;
  if (len - (HEAD + 8) > B1 * n_abc) return W761_ERR_TRAILING;
  rows.assign((size_t)(4 + n_abc) * G16_KW, 0);
  inf.assign((size_t)(4 + n_abc), 0);
  for (uint64_t i = 0; i < 4 + n_abc; i++) {
    const uint8_t* src = bytes + (i == 0 ? 0 : i < 4 ? B1 + B2 * (i - 1) : HEAD + 8 + B1 * (i - 4));
    const bool g2 = i >= 1 && i <= 3;
    uint64_t* row = rows.data() + i * G16_KW;
    const WireStatus st = g2 ? C::decode_g2(src, row) : C::decode_g1(src, row);
    if (st == WIRE_INFINITY) inf[i] = 1;
    else if (st != WIRE_OK) { if (first_bad) *first_bad = i; return W761_ERR_POINT; }
  }
  return 0;
}

}  // namespace celo
