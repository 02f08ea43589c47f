// Point decoding for BW6-761 G1 / G2 (arkworks 0.1 CanonicalDeserialize: coordinates little-endian, 96 B each, flags in the two top bits
// of the last byte) as host+device templates over the 28-limb field Fp<P761> the MSM uses.  What ark-groth16 0.1 runs per point when it
// reads a ProvingKey<BW6_761> / VerifyingKey / Proof (crates/epoch-snark/src/api/setup.rs:12,17-20 Groth16Parameters; the "serialized
// byte arrays of compressed elements" of crates/bls-snark-sys/src/snark/mod.rs:13-17): GroupAffine::deserialize (compressed, checked),
// deserialize_uncompressed (checked) and deserialize_unchecked (uncompressed, range only).  One source for both sides: Seam A's verify
// (seam_epoch.hip) decodes its vk and proof points on the host with w761_decode_row; the bulk form is k_decode761 (unit_wire761.hip), one point per lane.
//
// Curves (both over Fq, q = 3 mod 4):  G1  y^2 = x^3 - 1,   G2 (M-twist)  y^2 = x^3 + 4.   One template, b as its parameter.
//
// Status, in this order (the same codes and order as wire.h WireStatus / wire_decode_g1 and oracle/py/ecc.deser_point):
//   flags = the top two bits of the last byte (0x40 infinity, 0x80 "y is the lexicographically largest root"; uncompressed: y's last byte)
//   flags 0xC0                                   -> WIRE_INVALID (2)
//   infinity flag                                -> WIRE_INFINITY (1), before any range check
//   a coordinate >= q                            -> 2
//   compressed: rhs has no square root           -> 2
//   uncompressed, checked: (x, y) not on the curve -> 2
//   checked: r P != O (r = r_BW6 = q_BLS12-377)  -> WIRE_NOT_IN_SUBGROUP (3)   (w761_in_subgroup_endo; w761_in_subgroup is its definition)
//   otherwise                                    -> WIRE_OK (0)
// The uncompressed checked form tests the curve equation before the subgroup: stricter than ark 0.1's deserialize_uncompressed, which
// runs only is_in_correct_subgroup_assuming_on_curve - an off-curve (x, y) is rejected here (2) where ark may accept or reject it.
// The unchecked form (deserialize_unchecked) tests nothing past the canonical range of x and y.
#pragma once
#include <cstdint>
#include "curve.h"
#include "wire.h"

namespace celo {

typedef Fq761d Fw761;

// (q + 1) / 4, the exponent of the square root (q = 3 mod 4), and its width-3 sliding-window program: FIRST is the leading odd digit,
// then STEP[i] = "square once, then multiply by a^d" for d in {0, 1, 3, 5, 7}.  Built at compile time from P761::P64, so the program is
// the same constant in every lane (the branches below are scalar) and a^1, a^3, a^5, a^7 stay in registers - no run-time-indexed table.
struct W761Chain {
  int first = 0, len = 0;
  uint8_t step[768] = {};
};
constexpr int w761_exp_bit(const uint64_t* e, int i) { return (int)((e[i >> 6] >> (i & 63)) & 1); }
constexpr W761Chain w761_sqrt_chain() {
  uint64_t e[12] = {};
  for (int i = 0; i < 12; i++) e[i] = P761::P64[i];
  e[0] += 1;                                        // no carry: the low limb of q ends in 0x8b
  for (int i = 0; i < 12; i++) e[i] = (e[i] >> 2) | (i + 1 < 12 ? e[i + 1] << 62 : 0);
  W761Chain c;
  int i = 767;
  while (!w761_exp_bit(e, i)) i--;
  bool first = true;
  while (i >= 0) {
    if (!w761_exp_bit(e, i)) { c.step[c.len++] = 0; i--; continue; }
    int j = i - 2 < 0 ? 0 : i - 2;                  // the window [i .. j] ends on a set bit
    while (!w761_exp_bit(e, j)) j++;
    int v = 0;
    for (int b = i; b >= j; b--) v = 2 * v + w761_exp_bit(e, b);
    if (first) { c.first = v; first = false; }
    else {
      for (int b = i; b > j; b--) c.step[c.len++] = 0;
      c.step[c.len++] = (uint8_t)v;
    }
    i = j - 1;
  }
  return c;
}
struct W761Sqrt { static constexpr W761Chain C = w761_sqrt_chain(); };

HD bool w761_eq(const Fw761& a, const Fw761& b) { return Fw761::eq_mod_p(Fw761::norm(a), Fw761::norm(b)); }
HD Fw761 w761_neg(const Fw761& a) { return Fw761::wred(Fw761::norm(Fw761::neg<64, 1>(Fw761::norm(a)))); }
// 96 canonical little-endian bytes -> field element; false when the integer is not below q (Fp::deserialize's from_repr failure).
// flags: the last byte carries the two flag bits, which are not part of the integer.  (Read in place: a private copy of the bytes
// would be indexed memory.)
HD bool w761_from_bytes(const uint8_t* in, Fw761& out, bool flags) {
  uint64_t w[12];
  for (int i = 0; i < 12; i++) {
    uint64_t v = 0;
    for (int b = 7; b >= 0; b--) v = (v << 8) | in[8 * i + b];
    w[i] = v;
  }
  if (flags) w[11] &= ~(0xC0ull << 56);
  if (wire_cmp(w, P761::P64, 12) >= 0) return false;
  out = Fw761::from_canonical(w);
  return true;
}
HD bool w761_lex_largest(const Fw761& a) {   // canonical(a) > (q - 1) / 2
  uint64_t w[12];
  a.to_canonical(w);
  return wire_cmp(w, P761::PM1_HALF64, 12) > 0;
}
// x^3 + b for b = -1 (G1) or 4 (G2); [1, <= 10]
template <int B> HD Fw761 w761_rhs(const Fw761& x) {
  static_assert(B == -1 || B == 4, "BW6-761: G1 has b = -1, the M-twist G2 b = 4");
  const Fw761 x3 = Fw761::mul(Fw761::sqr(x), x);
  if constexpr (B < 0) return Fw761::norm(Fw761::sub<4, 1>(x3, Fw761::one()));
  else return Fw761::norm(Fw761::add(x3, Fw761::norm(Fw761::dbl(Fw761::dbl(Fw761::one())))));
}
// y = a^((q+1)/4) and the check y^2 == a (false: a is a non-residue).  758 squarings and 176 products after the four of the odd powers,
// the same program in every lane.
HD bool w761_sqrt(const Fw761& a_, Fw761& out) {
  constexpr const W761Chain& C = W761Sqrt::C;
  const Fw761 t1 = Fw761::norm(a_), a2 = Fw761::sqr(t1);
  const Fw761 t3 = Fw761::mul(t1, a2), t5 = Fw761::mul(t3, a2), t7 = Fw761::mul(t5, a2);
  static_assert(C.first == 1 || C.first == 3 || C.first == 5 || C.first == 7, "odd leading window");
  Fw761 r = C.first == 1 ? t1 : C.first == 3 ? t3 : C.first == 5 ? t5 : t7;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int i = 0; i < C.len; i++) {
    r = Fw761::sqr(r);
    const int d = C.step[i];
    if (d == 1) r = Fw761::mul(r, t1);
    else if (d == 3) r = Fw761::mul(r, t3);
    else if (d == 5) r = Fw761::mul(r, t5);
    else if (d == 7) r = Fw761::mul(r, t7);
  }
  if (!w761_eq(Fw761::sqr(r), t1)) return false;
  out = r;
  return true;
}
// acc += p, except when acc == p: false, and acc is left for the caller to double (curve.h xyzz_madd_unless_equal, which began here)
HD bool w761_madd(Xyzz<Fw761>& a, const Affine<Fw761>& p) { return xyzz_madd_unless_equal(a, p); }
// r P == O with r = q_BLS12-377 (377 bits), MSB-first double-and-add over XYZZ: ark-ec 0.1 is_in_correct_subgroup_assuming_on_curve as
// written.  The XYZZ formulas of curve.h do not depend on b, so one ladder serves both groups.
// One group operation per iteration (stage 0: double for bit i; 1: add p for bit i; 2: acc was p, double instead of adding).
// Kept word for word as the definition w761_in_subgroup_endo below is checked against (tests/test_subgroup_host.py,
// tests/test_check_points_gpu.py), as wire.h keeps wire_in_subgroup_ladder for BLS12-377; hook 1 of celo_amd_wire761_set_subgroup_test runs it.
HD bool w761_in_subgroup(const Affine<Fw761>& p) {
  Xyzz<Fw761> acc = Xyzz<Fw761>::from_affine(p);     // bit 376, the top bit of r
  int i = 375, stage = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  while (i >= 0) {
    if (stage == 1) {
      if (w761_madd(acc, p)) { stage = 0; i--; continue; }
      stage = 2;
    }
    acc = xyzz_dbl(acc);
    if (stage == 2) { stage = 0; i--; }
    else if (w761_exp_bit(P377::P64, i)) stage = 1;
    else i--;
  }
  return acc.is_identity() || acc.ZZ.is_zero_mod_p();
}

// ---- The same predicate through the endomorphism phi(x, y) = (beta x, y), beta a primitive cube root of unity in Fq (both curves have
// j = 0), so phi^2 + phi + 1 = 0 on all of E(Fq).  With x = 0x8508c00000000001 (the BLS12-377 parameter; r = q_BLS12-377) take
//     a = (2 x^3 - 2 x^2 - x + 1) / 3   (189 bits)        b = (x^3 - x^2 - 2 x - 1) / 3   (188 bits).
// Norm and exactness.  a^2 - a b + b^2 = r exactly (asserted below), and that is the degree of the endomorphism a + b phi (Z[phi] is the
//   ring of Eisenstein integers).  A separable endomorphism of degree r has a kernel of exactly r points.  beta is the cube root whose phi
//   acts on the order-r subgroup as the eigenvalue lambda with a + b lambda = 0 (mod r) - so the subgroup lies in the kernel, and having r
//   points it IS the kernel:  [a]P + [b]phi(P) == O  holds exactly when  r P == O, for every point of the curve.  No cofactor condition.
// Which beta.  G1 (y^2 = x^3 - 1) and G2 (y^2 = x^3 + 4) need different roots: with g = 2, G1 takes g^((q-1)/3) and G2 its square
//   (tests/test_subgroup_cases.py derives both and pins them on a subgroup point).
// Not the better-known short vector (x + 1, x^3 - x^2 + 1): its norm is 3 r, so its kernel has 3 r points.  On G1 that is still exact
//   (3 does not divide the cofactor h1); on G2 it is wrong: 3 | h2, T = (0, 2) has order 3 with phi(T) = T, and T, G + T, G - T all pass.
// Cost: one two-scalar ladder over separate NAFs of a and b (weights 36 and 37 over 190 columns): 189 doublings and 73 mixed additions
//   (one of them the first, a copy), about 2 430 field products where the 377-bit ladder (376 doublings, 134 additions) takes about 4 720.
//
// Compile-time integers of up to 512 bits, for the digit program and the identities asserted on it
struct W761Wide { uint64_t w[8] = {}; };
constexpr W761Wide w761w(uint64_t v) { W761Wide r; r.w[0] = v; return r; }
constexpr W761Wide w761w_add(const W761Wide& a, const W761Wide& b) {
  W761Wide r;
  unsigned __int128 c = 0;
  for (int i = 0; i < 8; i++) { c += (unsigned __int128)a.w[i] + b.w[i]; r.w[i] = (uint64_t)c; c >>= 64; }
  return r;
}
constexpr W761Wide w761w_sub(const W761Wide& a, const W761Wide& b) {   // a >= b
  W761Wide r;
  uint64_t borrow = 0;
  for (int i = 0; i < 8; i++) {
    const uint64_t d = a.w[i] - b.w[i], e = d - borrow;
    borrow = (a.w[i] < b.w[i]) || (d < borrow) ? 1 : 0;
    r.w[i] = e;
  }
  return r;
}
constexpr W761Wide w761w_mul(const W761Wide& a, const W761Wide& b) {   // the low 512 bits (every product below fits)
  W761Wide r;
  for (int i = 0; i < 8; i++) {
    unsigned __int128 c = 0;
    for (int j = 0; i + j < 8; j++) { c += (unsigned __int128)a.w[i] * b.w[j] + r.w[i + j]; r.w[i + j] = (uint64_t)c; c >>= 64; }
  }
  return r;
}
constexpr W761Wide w761w_div3(const W761Wide& a) {                      // floor(a / 3); exactness is asserted by multiplying back
  W761Wide r;
  unsigned __int128 rem = 0;
  for (int i = 7; i >= 0; i--) { const unsigned __int128 t = (rem << 64) | a.w[i]; r.w[i] = (uint64_t)(t / 3); rem = t % 3; }
  return r;
}
constexpr bool w761w_eq(const W761Wide& a, const W761Wide& b) {
  for (int i = 0; i < 8; i++) if (a.w[i] != b.w[i]) return false;
  return true;
}
constexpr bool w761w_is_zero(const W761Wide& a) { return w761w_eq(a, W761Wide{}); }
// The program of [a]P + [b]phi(P): columns from the top, one step each.  0: double; 1 / 2: add +P / -P; 3 / 4: add +phi(P) / -phi(P).
// Built at compile time from x, as W761Chain is: the same constant in every lane, branches scalar, nothing indexed at run time but the program.
struct W761EndoProgram {
  W761Wide a, b, three_a, three_b;
  int len = 0, doublings = 0, additions = 0;
  uint8_t step[320] = {};
};
constexpr int w761_naf(W761Wide k, int8_t* digits) {                    // non-adjacent form, least significant digit first; the length
  int n = 0;
  while (!w761w_is_zero(k)) {
    int d = 0;
    if (k.w[0] & 1) {
      d = (k.w[0] & 3) == 1 ? 1 : -1;
      k = d == 1 ? w761w_sub(k, w761w(1)) : w761w_add(k, w761w(1));
    }
    digits[n++] = (int8_t)d;
    for (int i = 0; i < 8; i++) k.w[i] = (k.w[i] >> 1) | (i + 1 < 8 ? k.w[i + 1] << 63 : 0);
  }
  return n;
}
constexpr W761EndoProgram w761_endo_program() {
  const W761Wide x = w761w(0x8508c00000000001ULL), x2 = w761w_mul(x, x), x3 = w761w_mul(x2, x), one = w761w(1);
  W761EndoProgram c;
  c.three_a = w761w_add(w761w_sub(w761w_sub(w761w_add(x3, x3), w761w_add(x2, x2)), x), one);                 // 2 x^3 - 2 x^2 - x + 1
  c.three_b = w761w_sub(w761w_sub(w761w_sub(x3, x2), w761w_add(x, x)), one);                                 // x^3 - x^2 - 2 x - 1
  c.a = w761w_div3(c.three_a);
  c.b = w761w_div3(c.three_b);
  int8_t da[512] = {}, db[512] = {};
  const int na = w761_naf(c.a, da), nb = w761_naf(c.b, db);
  for (int col = (na > nb ? na : nb) - 1; col >= 0; col--) {
    if (c.len) { c.step[c.len++] = 0; c.doublings++; }
    if (da[col]) { c.step[c.len++] = da[col] > 0 ? 1 : 2; c.additions++; }
    if (db[col]) { c.step[c.len++] = db[col] > 0 ? 3 : 4; c.additions++; }
  }
  return c;
}
constexpr bool w761_endo_norm_is_r(const W761EndoProgram& c) {          // a^2 - a b + b^2 == r = q_BLS12-377
  const W761Wide n = w761w_sub(w761w_add(w761w_mul(c.a, c.a), w761w_mul(c.b, c.b)), w761w_mul(c.a, c.b));
  W761Wide r;
  for (int i = 0; i < 6; i++) r.w[i] = P377::P64[i];
  return w761w_eq(n, r);
}
struct W761Endo {
  static constexpr W761EndoProgram C = w761_endo_program();
  // g^((q-1)/3) for g = 2 and its square, canonical, little-endian words: the beta of G1 and of G2
  static constexpr uint64_t BETA_G1[12] = {0x962140000000002a, 0xc547ba8a4000002f, 0xb6290012d96f8819, 0xf2f082d4dcb5e37c, 0xc65759fc45183151, 0x8e0a235a0a398300,
                                           0xab5e57926fa70184, 0xee4a737f73b6f952, 0x2d17be416c5e4426, 0x6c1f31e53bd9603c, 0xaa846c61024e4cca, 0x531dc16c6ecd27};
  static constexpr uint64_t BETA_G2[12] = {0x5e7bc00000000060, 0x214983de30000053, 0x5fe3f89c11811c1e, 0xa5b093ed79b1c57b, 0xab8579e02ed3cddc, 0xf87fa59308c07a8f,
                                           0x5870636cb60d217f, 0x823132b971cdefc6, 0x256ab7ae14297a1a, 0x4d06e68545f7e64c, 0x27035cdf02acb274, 0xcfca638f1500e3};
};
static_assert(w761w_eq(w761w_mul(W761Endo::C.a, w761w(3)), W761Endo::C.three_a), "3 a = 2 x^3 - 2 x^2 - x + 1");
static_assert(w761w_eq(w761w_mul(W761Endo::C.b, w761w(3)), W761Endo::C.three_b), "3 b = x^3 - x^2 - 2 x - 1");
static_assert(w761_endo_norm_is_r(W761Endo::C), "a^2 - a b + b^2 = r: the endomorphism a + b phi has degree r");
static_assert(W761Endo::C.doublings == 189 && W761Endo::C.additions == 73 && W761Endo::C.len == 262, "190 columns, NAF weights 36 and 37");
static_assert(W761Endo::C.step[0] != 0 && W761Endo::C.len <= 320, "the program starts with an addition and fits its array");

// [a]P + [b]phi(P) == O for a finite point p of the curve with b = B (the curve constant picks beta).  One group operation per step, through
// one addition site and one doubling site.  The addition is complete on every input: an accumulator at the identity takes the addend
// (xyzz_madd_unless_equal), one opposite to the addend becomes the identity, one EQUAL to it is doubled at the doubling site (which maps a
// point with y = 0 to the identity) - so points of low order, where these branches are taken constantly, and phi(P) == P (x = 0) need no case of
// their own.  The addends are (x or beta x, y or -y): phi(P) costs the one product beta x, kept for the whole ladder; -y is formed per addition.
template <int B> HD bool w761_in_subgroup_endo(const Affine<Fw761>& p) {
  static_assert(B == -1 || B == 4, "BW6-761: G1 has b = -1, the M-twist G2 b = 4");
  constexpr const W761EndoProgram& C = W761Endo::C;
  const Fw761 bx = Fw761::norm(Fw761::mul(Fw761::from_canonical(B < 0 ? W761Endo::BETA_G1 : W761Endo::BETA_G2), p.x));
  Xyzz<Fw761> acc = Xyzz<Fw761>::identity();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int i = 0; i < C.len; i++) {
    const int op = C.step[i];
    bool dbl = op == 0;
    if (!dbl) {
      const Affine<Fw761> q = {op >= 3 ? bx : p.x, (op & 1) ? p.y : w761_neg(p.y)};
      dbl = !w761_madd(acc, q);
    }
    if (dbl) acc = xyzz_dbl(acc);
  }
  return acc.is_identity() || acc.ZZ.is_zero_mod_p();
}

// one point up to the subgroup test: in = 96 B (compressed: x with the flags) or 192 B (uncompressed: x, then y with the flags); check:
// the curve equation of the uncompressed form.  p is set when WIRE_OK.
template <int B, bool COMPRESSED> HD WireStatus w761_parse(const uint8_t* in, bool check, Affine<Fw761>& p) {
  constexpr int NB = COMPRESSED ? 96 : 192;
  const uint8_t flags = in[NB - 1] & 0xC0;
  if (flags == 0xC0) return WIRE_INVALID;          // ark-serialize SWFlags::from_u8: (sign, infinity) both set is no encoding at all
  if (flags & 0x40) return WIRE_INFINITY;
  Fw761 x, y;
  if (!w761_from_bytes(in, x, COMPRESSED)) return WIRE_INVALID;
  if constexpr (COMPRESSED) {
    if (!w761_sqrt(w761_rhs<B>(x), y)) return WIRE_INVALID;
    if (w761_lex_largest(y) != ((flags & 0x80) != 0)) y = w761_neg(y);
  } else {
    if (!w761_from_bytes(in + 96, y, true)) return WIRE_INVALID;
    if (check && !w761_eq(Fw761::sqr(y), w761_rhs<B>(x))) return WIRE_INVALID;
  }
  p = {Fw761::norm(x), Fw761::norm(y)};
  return WIRE_OK;
}
// the whole decoding (the kernels run it in two passes, w761_parse and the subgroup test: unit_wire761.hip, unit_check.hip)
template <int B, bool COMPRESSED> HD WireStatus w761_decode(const uint8_t* in, bool check, Affine<Fw761>& p) {
  const WireStatus st = w761_parse<B, COMPRESSED>(in, check, p);
  if (st == WIRE_OK && check && !w761_in_subgroup_endo<B>(p)) return WIRE_NOT_IN_SUBGROUP;
  return st;
}
// the row form the MSM entry points take: 24 u64, (x, y) as arkworks Montgomery limbs; zeros unless WIRE_OK
template <int B, bool COMPRESSED> HD WireStatus w761_decode_row(const uint8_t* in, bool check, uint64_t* out) {
  Affine<Fw761> p = {Fw761::zero(), Fw761::zero()};
  const WireStatus st = w761_decode<B, COMPRESSED>(in, check, p);
  if (st == WIRE_OK) { p.x.to_ark(out); p.y.to_ark(out + 12); }
  else for (int j = 0; j < 24; j++) out[j] = 0;
  return st;
}

// ---- encoding (GroupAffine::serialize / serialize_uncompressed): wire.h's WireEnc over the 12-word field.  G1 and G2 share the
// coordinate field and the encoder never touches the curve constant, so one instantiation per form serves both groups.
typedef WireEnc<P761, 1, true> W761EncC;     // 24 u64 -> 12 words (96 B)
typedef WireEnc<P761, 1, false> W761EncU;    // 24 u64 -> 24 words (192 B)
// an arkworks Jacobian point (X, Y, Z: 36 u64, what groth16_prove_* returns) -> its compressed encoding; Z == 0 is the identity
HD WireStatus w761_encode_jacobian(const uint64_t* xyz, uint64_t* out12) {
  const Fw761 Z = Fw761::norm(Fw761::from_ark(xyz + 24));
  uint64_t row[24];
  for (int j = 0; j < 24; j++) row[j] = 0;
  const bool inf = Z.is_zero_mod_p();
  if (!inf) {
    const Fw761 zi = Fw761::norm(Fw761::inv(Z)), zi2 = Fw761::sqr(zi);
    Fw761::mul(Fw761::from_ark(xyz), zi2).to_ark(row);
    Fw761::mul(Fw761::from_ark(xyz + 12), Fw761::mul(zi2, zi)).to_ark(row + 12);
  }
  return W761EncC::row(row, inf, false, out12);
}

// ---- host: the layout of a serialized ark-groth16 0.1 ProvingKey<E> (its derive order; Vec = u64 LE length, then the elements):
//   vk { alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1: Vec<G1> }, beta_g1, delta_g1,
//   a_query: Vec<G1>, b_g1_query: Vec<G1>, b_g2_query: Vec<G2>, h_query: Vec<G1>, l_query: Vec<G1>
// One walk for both curves (curve 0 = BW6-761, 1 = BLS12-377); they differ in the two point sizes alone.  A G1 point is P bytes and a G2
// point P2: BW6-761 P = P2 = 96 compressed / 192 uncompressed (both groups over Fq); BLS12-377 P = 48 / 96 and P2 = 2 P (G2 over Fq2), so
// there only the three G2 elements of the vk and b_g2_query have the double stride.
// The length fields are input: no count * size is formed before count is known to fit what is left.
enum W761Layout { W761_PT = 0, W761_LEN = 1, W761_ABC = 2, W761_A = 4, W761_BG1 = 6, W761_BG2 = 8, W761_H = 10, W761_L = 12, W761_BETA_G1 = 14, W761_NPOINTS = 15 };
constexpr int W761_ERR_TRUNCATED = 30, W761_ERR_TRAILING = 31, W761_ERR_LENGTH = 32, W761_ERR_POINT = 33;
constexpr int W761_ERR_CAPACITY = 35;             // the key writer: the output buffer is smaller than the serialization (34 is the R1CS loader's)
constexpr uint64_t wkey_g1_bytes(int curve, int form) { return (curve ? 48 : 96) * (form == 0 ? 1 : 2); }
constexpr uint64_t wkey_g2_bytes(int curve, int form) { return 96 * (form == 0 ? 1 : 2); }
inline int wkey_layout(int curve, const uint8_t* bytes, size_t len, int form, uint64_t out[16]) {
  if (!out || (!bytes && len) || form < 0 || form > 2 || curve < 0 || curve > 1) return 2;
  for (int i = 0; i < 16; i++) out[i] = 0;
  const uint64_t P = wkey_g1_bytes(curve, form), P2 = wkey_g2_bytes(curve, form);
  uint64_t pos = 0, points = 0;
  auto take = [&](uint64_t count, uint64_t size) -> int {   // count points of `size` bytes at pos
    if (count > UINT64_MAX / size) return W761_ERR_LENGTH;
    if (count * size > len - pos) return W761_ERR_TRUNCATED;
    pos += count * size;
    points += count;
    return 0;
  };
  auto vec = [&](int slot, uint64_t size) -> int {  // u64 length, then the points
    if (len - pos < 8) return W761_ERR_TRUNCATED;
    uint64_t n = 0;
    for (int b = 7; b >= 0; b--) n = (n << 8) | bytes[pos + b];
    pos += 8;
    out[slot] = n;
    out[slot + 1] = pos;
    return take(n, size);
  };
  int rc = take(1, P);                              // alpha_g1
  if (!rc) rc = take(3, P2);                        // beta_g2, gamma_g2, delta_g2
  if (!rc) rc = vec(W761_ABC, P);
  if (!rc) { out[W761_BETA_G1] = pos; rc = take(2, P); }   // beta_g1, delta_g1
  if (!rc) rc = vec(W761_A, P);
  if (!rc) rc = vec(W761_BG1, P);
  if (!rc) rc = vec(W761_BG2, P2);
  if (!rc) rc = vec(W761_H, P);
  if (!rc) rc = vec(W761_L, P);
  if (rc) return rc;
  if (pos != len) return W761_ERR_TRAILING;
  out[W761_PT] = P;
  out[W761_LEN] = len;
  out[W761_NPOINTS] = points;
  return 0;
}

// The byte length of what wkey_layout parses, from the counts (the key writer's side): form 0 = compressed points, 1 = uncompressed; vk_only:
// the VerifyingKey prefix alone (n_vars and n_h are not looked at).  l_query has n_vars - n_inputs rows.  2: no such key, or a length past 64 bits.
inline int wkey_size(int curve, uint64_t n_inputs, uint64_t n_vars, uint64_t n_h, int form, int vk_only, uint64_t* len) {
  if (!len || form < 0 || form > 1 || curve < 0 || curve > 1 || n_inputs == 0 || (!vk_only && n_inputs > n_vars)) return 2;
  const unsigned __int128 P = wkey_g1_bytes(curve, form), P2 = wkey_g2_bytes(curve, form);
  unsigned __int128 t = (1 + (unsigned __int128)n_inputs) * P + 3 * P2 + 8;
  if (!vk_only) t += (2 + 2 * (unsigned __int128)n_vars + n_h + (n_vars - n_inputs)) * P + (unsigned __int128)n_vars * P2 + 5 * 8;
  if (t > UINT64_MAX) return 2;
  *len = (uint64_t)t;
  return 0;
}

}  // namespace celo
