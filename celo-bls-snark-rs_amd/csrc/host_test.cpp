// Host-only build of the product's field/curve templates with run-time bounds tracking
// (-DCELO_FP_TRACK): every mul/sub asserts the limb/value bounds of fp.h's contract.
// Driven by tests/test_host_field.py through ctypes; never shipped.
#include <memory>
#include <mutex>
#include <vector>
#include "curve.h"
#include "gls.h"
#include "fp2.h"
#include "pairing.h"
#include "curve_lanes.h"
#include "wire.h"
#include "wire761.h"
#include "check.h"
#include "dedup.h"
#include "fixed_base.h"
#include "var_base.h"
#include "aggregate.h"
#include "groth16_verify.h"
#include "r1cs.h"
#include "hash_direct.h"
#include "epoch.h"
#include "transitions.h"
#include "host64.h"
#include <cstring>
using namespace celo;

template <class F> static void xyzz_to_jac(const Xyzz<F>& p, uint64_t* out) {
  constexpr int A = F::ARK64;
  if (p.is_identity()) { F::zero().to_ark(out); F::one().to_ark(out + A); F::zero().to_ark(out + 2 * A); return; }
  F::mul(p.X, p.ZZ).to_ark(out);
  F::mul(p.Y, p.ZZZ).to_ark(out + A);
  p.ZZ.to_ark(out + 2 * A);
}
template <class F> static Affine<F> load_aff(const uint64_t* xy) { return {F::from_ark(xy), F::from_ark(xy + F::ARK64)}; }

// op: 0 mul, 1 sqr, 2 add(norm), 3 sub, 4 inv, 5 roundtrip ark->dev->ark, 6 canonical roundtrip
template <class F> static void field_op(int op, const uint64_t* a, const uint64_t* b, uint64_t* out) {
  F x = F::from_ark(a), y = F::from_ark(b), r;
  switch (op) {
    case 0: r = F::mul(x, y); break;
    case 1: r = F::sqr(x); break;
    case 2: r = F::norm(F::add(x, y)); break;
    case 3: r = F::norm(F::template sub<4, 1>(x, y)); break;
    case 4: r = F::inv(x); break;
    default: r = x; break;
  }
  r.to_ark(out);
}
// chained stress: exercises lazy bounds across many dependent ops like the curve formulas do
template <class F> static void point_op(int op, const uint64_t* p1, const uint64_t* p2, uint32_t k, uint64_t* out) {
  Affine<F> a = load_aff<F>(p1), b = load_aff<F>(p2);
  Xyzz<F> acc = Xyzz<F>::from_affine(a);
  switch (op) {
    case 0: xyzz_madd(acc, b); break;                       // a + b
    case 1: acc = xyzz_dbl(acc); break;                     // 2a
    case 2: { Xyzz<F> t = Xyzz<F>::from_affine(b); t = xyzz_dbl(t); xyzz_madd(t, a); xyzz_add(acc, t); } break;  // a + (2b + a)
    case 3: acc = xyzz_mul_small(acc, k); break;            // k*a
    case 4: xyzz_madd(acc, affine_neg(a)); break;           // a - a = 0
    case 5: xyzz_madd(acc, a); break;                       // a + a via madd (doubling branch)
    case 6: { for (uint32_t i = 0; i < k; i++) xyzz_madd(acc, b); } break;  // a + k*b by repeated madd
    case 7: { Xyzz<F> t = acc; xyzz_add(acc, t); } break;   // add-with-self (doubling branch of add)
    case 8: { for (uint32_t i = 0; i < k; i++) acc = xyzz_dbl(acc); xyzz_madd(acc, b); } break;  // 2^k a + b (a Horner step)
    case 9: acc = xyzz_add_affine(a, b); break;             // a + b, both affine (the first addition of a bucket run)
    case 10: acc = xyzz_add_affine(a, a); break;            // its doubling branch
    case 11: acc = xyzz_add_affine(a, affine_neg(a)); break;  // its cancellation branch
    case 12: { acc = xyzz_add_affine(affine_neg(a), affine_neg(b)); for (uint32_t i = 0; i < k; i++) xyzz_madd(acc, b); } break;  // -a - b + k b
    // 13 .. 17: xyzz_add_mem (the second point read from its stored form where its coordinates are used): t = 2b + a stored, then
    // a + t; the identity stored as zeros; into an identity accumulator; the doubling and the cancellation branch
    case 13: case 14: case 15: case 16: case 17: {
      Xyzz<F> t = Xyzz<F>::from_affine(b); t = xyzz_dbl(t); xyzz_madd(t, a);
      if (op == 14) t = Xyzz<F>::identity();
      if (op == 16) t = acc;                                           // a + a
      if (op == 17) t = Xyzz<F>::from_affine(affine_neg(a));           // a - a
      if (op == 15) acc = Xyzz<F>::identity();                         // 0 + t
      alignas(16) uint32_t buf[4 * F::WORDS];
      t.X.store(buf); t.Y.store(buf + F::WORDS); t.ZZ.store(buf + 2 * F::WORDS); t.ZZZ.store(buf + 3 * F::WORDS);
      xyzz_add_mem(acc, buf);
    } break;
    default: break;
  }
  xyzz_to_jac(acc, out);
}

// lane-parallel XYZZ arithmetic (curve_lanes.h) on the three-explicit-lanes host backend: the same ops as point_op
template <class F> static void lane_point_op(int op, const uint64_t* p1, const uint64_t* p2, uint32_t k, uint64_t* out) {
  typedef QHostT<FieldBase<F>> QB;
  typedef LanePoint<QB> LP;
  Affine<F> a = load_aff<F>(p1), b = load_aff<F>(p2);
  auto lift = [](const Affine<F>& p) { typename LP::P r = {QB::uni(p.x), QB::uni(p.y), QB::uni(F::one()), QB::uni(F::one())}; return r; };
  typename LP::Pt acc = {lift(a), false};
  switch (op) {
    case 0: LP::add(acc, lift(b), false); break;                                            // a + b
    case 1: LP::dbl(acc); break;                                                            // 2a
    case 2: { typename LP::Pt t = {lift(b), false}; LP::dbl(t); LP::add(t, lift(a), false); LP::add(acc, t.p, t.inf); } break;  // a + (2b + a)
    case 4: LP::add(acc, lift(affine_neg(a)), false); break;                                // a - a = 0
    case 6: { for (uint32_t i = 0; i < k; i++) LP::add(acc, lift(b), false); } break;        // a + k*b
    case 7: { typename LP::P t = acc.p; LP::add(acc, t, false); } break;                    // a + a through add (doubling branch)
    case 8: { for (uint32_t i = 0; i < k; i++) LP::dbl(acc); LP::add(acc, lift(b), false); } break;  // 2^k a + b (a Horner step)
    default: break;
  }
  Xyzz<F> r = acc.inf ? Xyzz<F>::identity() : Xyzz<F>{acc.p.X.v[0], acc.p.Y.v[0], acc.p.ZZ.v[0], acc.p.ZZZ.v[0]};
  for (int l = 1; l < 3 && !acc.inf; l++) {   // the lanes must agree
    if (!F::norm(F::template sub<64, 1>(F::norm(acc.p.X.v[l]), F::norm(r.X))).is_zero_mod_p() ||
        !F::norm(F::template sub<64, 1>(F::norm(acc.p.ZZZ.v[l]), F::norm(r.ZZZ))).is_zero_mod_p()) r = Xyzz<F>::identity();
  }
  xyzz_to_jac(r, out);
}

// the same ops for G2 of BLS12-377 on the SIX-lane host backend (halves of an Fq2 in adjacent lanes: msm.h k_batch_horner_hex)
static void lane_point_op_hex(int op, const uint64_t* p1, const uint64_t* p2, uint32_t k, uint64_t* out) {
  typedef Fp2<P377> F;
  typedef QHostHex377 QB;
  typedef LanePoint<QB> LP;
  Affine<F> a = load_aff<F>(p1), b = load_aff<F>(p2);
  auto lift = [](const Affine<F>& p) { LP::P r = {QB::uni2(p.x.c0, p.x.c1), QB::uni2(p.y.c0, p.y.c1), QB::uni2(Fq::one(), Fq::zero()), QB::uni2(Fq::one(), Fq::zero())}; return r; };
  LP::Pt acc = {lift(a), false};
  switch (op) {
    case 0: LP::add(acc, lift(b), false); break;
    case 1: LP::dbl(acc); break;
    case 2: { LP::Pt t = {lift(b), false}; LP::dbl(t); LP::add(t, lift(a), false); LP::add(acc, t.p, t.inf); } break;
    case 4: LP::add(acc, lift(affine_neg(a)), false); break;
    case 6: { for (uint32_t i = 0; i < k; i++) LP::add(acc, lift(b), false); } break;
    case 7: { LP::P t = acc.p; LP::add(acc, t, false); } break;
    case 8: { for (uint32_t i = 0; i < k; i++) LP::dbl(acc); LP::add(acc, lift(b), false); } break;
    default: break;
  }
  auto f2 = [](const QB::V& v, int j) { return F{v.v[2 * j], v.v[2 * j + 1]}; };
  Xyzz<F> r = acc.inf ? Xyzz<F>::identity() : Xyzz<F>{f2(acc.p.X, 0), f2(acc.p.Y, 0), f2(acc.p.ZZ, 0), f2(acc.p.ZZZ, 0)};
  for (int l = 1; l < 3 && !acc.inf; l++) {   // the tower lanes must agree
    if (!F::norm(F::template sub<64, 1>(F::norm(f2(acc.p.X, l)), F::norm(r.X))).is_zero_mod_p() ||
        !F::norm(F::template sub<64, 1>(F::norm(f2(acc.p.ZZZ, l)), F::norm(r.ZZZ))).is_zero_mod_p()) r = Xyzz<F>::identity();
  }
  xyzz_to_jac(r, out);
}

// pairing tower on the host with bounds tracking.  mode 0: product of pairings (GT), 1: Miller-loop product only,
// 2: final exponentiation of the given GT (in72), 3: Fq12 mul (in72 * in72b), 4: Fq12 inverse, 5: cyclotomic square,
// 6: frobenius 1, 7: frobenius 2, 8: frobenius 3, 9: Fq12 square
static void pairing_op(int mode, const uint64_t* g1, const uint64_t* g2, size_t k, const uint64_t* in72, const uint64_t* in72b,
                       uint64_t* out72, int* is_one) {
  Fq12 r;
  if (mode <= 1) {
    Fq12 acc = f12_one();
    for (size_t i = 0; i < k; i++) {
      Fq px = Fq::from_ark(g1 + i * 12), py = Fq::from_ark(g1 + i * 12 + 6);
      Fq2 qx = Fq2::from_ark(g2 + i * 24), qy = Fq2::from_ark(g2 + i * 24 + 12);
      Fq12 f, t;
      miller_loop_single(f, px, py, qx, qy);
      f12_mul(t, acc, f);
      acc = t;
    }
    if (mode == 0) final_exponentiation(r, acc);
    else r = acc;
  } else {
    Fq12 a = f12_from_ark(in72);
    switch (mode) {
      case 2: final_exponentiation(r, a); break;
      case 3: { Fq12 b = f12_from_ark(in72b); f12_mul(r, a, b); } break;
      case 4: f12_inv(r, a); break;
      case 5: f12_cyclotomic_sqr(r, a); break;
      case 6: f12_frob<1>(r, a); break;
      case 7: f12_frob<2>(r, a); break;
      case 8: f12_frob<3>(r, a); break;
      default: f12_sqr(r, a); break;
    }
  }
  f12_to_ark(r, out72);
  if (is_one) *is_one = f12_is_one(r) ? 1 : 0;
}

// the lane-parallel pairing (pairing_lanes.h) on its explicit-lanes host backends - three lanes per pairing (an Fq2 per lane)
// and six (half an Fq2 per lane); same modes as pairing_op
struct HostTri {
  typedef QHost377 QB;
  static QB::V v2(const Fq2& lane0, const Fq2& lane1, const Fq2& lane2) { QB::V r; r.v[0] = lane0; r.v[1] = lane1; r.v[2] = lane2; return r; }
  static QB::F f1(const Fq& x) { QB::F r; for (int l = 0; l < 3; l++) r.v[l] = x; return r; }
  static Fq2 get(const QB::V& v, int j) { return v.v[j]; }
};
struct HostHex {
  typedef QHostHex377 QB;
  static QB::V v2(const Fq2& lane0, const Fq2& lane1, const Fq2& lane2) {
    QB::V r;
    const Fq2* s[3] = {&lane0, &lane1, &lane2};
    for (int j = 0; j < 3; j++) { r.v[2 * j] = s[j]->c0; r.v[2 * j + 1] = s[j]->c1; }
    return r;
  }
  static QB::F f1(const Fq& x) { QB::F r; for (int l = 0; l < 6; l++) r.v[l] = x; return r; }
  static Fq2 get(const QB::V& v, int j) { return {v.v[2 * j], v.v[2 * j + 1]}; }
};
template <class H> static void pairing_op_lanes_t(int mode, const uint64_t* g1, const uint64_t* g2, size_t k, const uint64_t* in72, const uint64_t* in72b,
                                                  uint64_t* out72, int* is_one) {
  typedef typename H::QB QB;
  typedef QTower<QB> HQT;
  typedef QPairing377<QB> HQP;
  auto from_f12 = [](const Fq12& x) {
    typename HQT::E12 e;
    e.a = H::v2(x.c0.c0, x.c0.c1, x.c0.c2);
    e.b = H::v2(x.c1.c0, x.c1.c1, x.c1.c2);
    return e;
  };
  auto to_f12 = [](const typename HQT::E12& e) {
    Fq12 x;
    x.c0.c0 = H::get(e.a, 0); x.c0.c1 = H::get(e.a, 1); x.c0.c2 = H::get(e.a, 2);
    x.c1.c0 = H::get(e.b, 0); x.c1.c1 = H::get(e.b, 1); x.c1.c2 = H::get(e.b, 2);
    return x;
  };
  auto load_pair = [&](size_t i, typename QB::F& px, typename QB::F& py, typename QB::V& Qc) {
    px = H::f1(Fq::from_ark(g1 + i * 12)); py = H::f1(Fq::from_ark(g1 + i * 12 + 6));
    const Fq2 qx = Fq2::from_ark(g2 + i * 24), qy = Fq2::from_ark(g2 + i * 24 + 12);
    Qc = H::v2(qx, qy, qx);                                      // lanes 0, 2: Q.x; lane 1: Q.y
  };
  typename HQT::E12 r;
  if (mode == 10 || mode == 11) {  // whole product in one group with a shared accumulator (k <= 4); 10: GT value, 11: Miller value
    typename QB::F px[4], py[4];
    typename QB::V Qc[4];
    for (size_t i = 0; i < k && i < 4; i++) load_pair(i, px[i], py[i], Qc[i]);
    typename HQT::E12 acc = HQP::template miller_multi<4>((int)k, px, py, Qc);
    r = mode == 10 ? HQP::final_exponentiation(acc) : acc;
  } else if (mode == 13 || mode == 14) {  // exactly two pairs, the lines of every step multiplied first (miller_pair2); 13: GT value, 14: Miller value
    typename QB::F px[2], py[2];
    typename QB::V Qc[2];
    for (size_t i = 0; i < 2; i++) load_pair(i, px[i], py[i], Qc[i]);
    typename HQT::E12 acc = HQP::miller_pair2(px, py, Qc);
    r = mode == 13 ? HQP::final_exponentiation(acc) : acc;
  } else if (mode == 12) {         // the product tree of the GPU engine: Miller values multiplied with each other pairwise (bounds: value x value)
    std::vector<typename HQT::E12> m(k);
    for (size_t i = 0; i < k; i++) {
      typename QB::F px, py;
      typename QB::V Qc;
      load_pair(i, px, py, Qc);
      m[i] = HQP::miller(px, py, Qc);
    }
    for (size_t n = k; n > 1; n = (n + 1) / 2)
      for (size_t t = 0; 2 * t < n; t++) m[t] = 2 * t + 1 < n ? HQT::mul12(m[2 * t], m[2 * t + 1]) : m[2 * t];
    r = HQP::final_exponentiation(m[0]);
  } else if (mode <= 1) {
    typename HQT::E12 acc = HQT::one12();
    for (size_t i = 0; i < k; i++) {
      typename QB::F px, py;
      typename QB::V Qc;
      load_pair(i, px, py, Qc);
      acc = HQT::mul12(acc, HQP::miller(px, py, Qc));
    }
    r = mode == 0 ? HQP::final_exponentiation(acc) : acc;
  } else {
    typename HQT::E12 a = from_f12(f12_from_ark(in72));
    switch (mode) {
      case 2: r = HQP::final_exponentiation(a); break;
      case 3: r = HQT::mul12(a, from_f12(f12_from_ark(in72b))); break;
      case 4: r = HQT::inv12(a); break;
      case 5: r = HQT::cyclotomic_sqr(a); break;
      case 6: r = HQP::template frob12<1>(a); break;
      case 7: r = HQP::template frob12<2>(a); break;
      case 8: r = HQP::template frob12<3>(a); break;
      default: r = HQT::sqr12(a); break;
    }
  }
  f12_to_ark(to_f12(r), out72);
  if (is_one) *is_one = HQT::is_one12(r) ? 1 : 0;
}
static void pairing_op_lanes(int mode, const uint64_t* g1, const uint64_t* g2, size_t k, const uint64_t* in72, const uint64_t* in72b,
                             uint64_t* out72, int* is_one) { pairing_op_lanes_t<HostTri>(mode, g1, g2, k, in72, in72b, out72, is_one); }
static void pairing_op_hex(int mode, const uint64_t* g1, const uint64_t* g2, size_t k, const uint64_t* in72, const uint64_t* in72b,
                           uint64_t* out72, int* is_one) { pairing_op_lanes_t<HostHex>(mode, g1, g2, k, in72, in72b, out72, is_one); }
// the lane-parallel BW6-761 pairing on three host lanes.  mode 0 / 1: per-pair Miller values multiplied in input order (GT / Miller value);
// 10 / 11: the whole product (k <= 4; more is refused) through miller_multi<4>, what k_miller_product_lanes<LP761> runs (GT / Miller value); 12: the value-by-value
// product tree of k_gt_tree_lanes (an unpaired last value of an odd level is carried), then the final exponentiation
static void pairing_op_761_lanes(int mode, const uint64_t* g1, const uint64_t* g2, size_t k, uint64_t* out72, int* is_one) {
  typedef QTower<QHost761> T6;
  typedef QPairing761<QHost761> P6;
  auto load_pair = [&](size_t i, QHost761::V& px, QHost761::V& py, QHost761::V& Qc) {
    for (int l = 0; l < 3; l++) {
      px.v[l] = Fw::from_ark(g1 + i * 24); py.v[l] = Fw::from_ark(g1 + i * 24 + 12);
      Qc.v[l] = Fw::from_ark(g2 + i * 24 + (l & 1) * 12);
    }
  };
  T6::E12 acc = T6::one12();
  if (mode == 10 || mode == 11) {
    QHost761::V px[4], py[4], Qc[4];
    if (k > 4) {        // miller_multi<4> holds four pairs: refused, not clamped (out72 stays zero, is_one = -1)
      for (int i = 0; i < 72; i++) out72[i] = 0;
      if (is_one) *is_one = -1;
      return;
    }
    for (size_t i = 0; i < k; i++) load_pair(i, px[i], py[i], Qc[i]);
    acc = P6::miller_multi<4>((int)k, px, py, Qc);
  } else if (mode == 12) {
    std::vector<T6::E12> m(k ? k : 1, T6::one12());
    for (size_t i = 0; i < k; i++) {
      QHost761::V px, py, Qc;
      load_pair(i, px, py, Qc);
      m[i] = P6::miller(px, py, Qc);
    }
    for (size_t n = k; n > 1; n = (n + 1) / 2)
      for (size_t t = 0; 2 * t < n; t++) m[t] = 2 * t + 1 < n ? T6::mul12(m[2 * t], m[2 * t + 1]) : m[2 * t];
    acc = m[0];
  } else {
    for (size_t i = 0; i < k; i++) {
      QHost761::V px, py, Qc;
      load_pair(i, px, py, Qc);
      acc = T6::mul12(acc, P6::miller(px, py, Qc));
    }
  }
  T6::E12 r = (mode == 0 || mode == 10 || mode == 12) ? P6::final_exponentiation(acc) : acc;
  Fw6 x;
  Fw* c[6] = {&x.c0.c0, &x.c0.c1, &x.c0.c2, &x.c1.c0, &x.c1.c1, &x.c1.c2};
  for (int j = 0; j < 3; j++) { *c[j] = r.a.v[j]; *c[3 + j] = r.b.v[j]; }
  QuadIO<Base761>::to_ark(x, out72);
  if (is_one) *is_one = T6::is_one12(r) ? 1 : 0;
}

static void pairing_op_761(int mode, const uint64_t* g1, const uint64_t* g2, size_t k, uint64_t* out72, int* is_one) {
  Fw6 acc = quad_one<Base761>();
  for (size_t i = 0; i < k; i++) {
    Fw6 f, t;
    { Fw px = Fw::from_ark(g1 + i * 24), py = Fw::from_ark(g1 + i * 24 + 12), qx = Fw::from_ark(g2 + i * 24), qy = Fw::from_ark(g2 + i * 24 + 12);
      bw6_miller_loop_single(f, px, py, qx, qy); }
    quad_mul(t, acc, f);
    acc = t;
  }
  Fw6 r;
  if (mode == 0) bw6_final_exponentiation(r, acc);
  else r = acc;
  QuadIO<Base761>::to_ark(r, out72);
  if (is_one) *is_one = quad_is_one(r) ? 1 : 0;
}

extern "C" int celo_ifma_available();
extern "C" int celo_ifma_horner_377(const uint64_t* pts, size_t stride, const int32_t* order, int steps, uint64_t* out, int* inf);
extern "C" int celo_ifma_horner_761(const uint64_t* pts, size_t stride, const int32_t* order, int steps, uint64_t* out, int* inf);
extern "C" {
// wire.h under bounds tracking: n compressed points -> affine ark limbs + status (the GPU kernels run the same functions)
void ht_wire_decode(int g2, const uint8_t* in, size_t n, int check, uint64_t* out, uint8_t* status) {
  const WireConsts& k = wire_consts();
  for (size_t i = 0; i < n; i++) {
    uint64_t* o = out + i * (g2 ? 24 : 12);
    memset(o, 0, (g2 ? 24 : 12) * 8);
    if (g2) {
      Affine<Fq2> p = {Fq2::zero(), Fq2::zero()};
      status[i] = wire_decode_g2(in + i * 96, k, check != 0, p);
      if (status[i] == WIRE_OK) { p.x.c0.to_ark(o); p.x.c1.to_ark(o + 6); p.y.c0.to_ark(o + 12); p.y.c1.to_ark(o + 18); }
    } else {
      Affine<Fq> p = {Fq::zero(), Fq::zero()};
      status[i] = wire_decode_g1(in + i * 48, k, check != 0, p);
      if (status[i] == WIRE_OK) { p.x.to_ark(o); p.y.to_ark(o + 6); }
    }
  }
}
// the uncompressed forms of wire.h under bounds tracking: n x 96 B (G1) / n x 192 B (G2) -> 12 / 24 u64 rows + status (k_decode377u runs the same templates)
void ht_wire377_decode_uncompressed(int g2, int check, const uint8_t* in, size_t n, uint64_t* out, uint8_t* status) {
  const WireConsts& k = wire_consts();
  for (size_t i = 0; i < n; i++) {
    if (g2) status[i] = wire_decode_row_g2<false>(in + i * 192, k, check != 0, out + i * 24);
    else status[i] = wire_decode_row_g1<false>(in + i * 96, k, check != 0, out + i * 12);
  }
}
// wire761.h under bounds tracking: n BW6-761 points (compressed 96 B / uncompressed 192 B) -> 24 u64 rows + status (k_decode761 runs the same template)
void ht_wire761_decode(int g2, int compressed, int check, const uint8_t* in, size_t n, uint64_t* out, uint8_t* status) {
  const size_t ib = compressed ? 96 : 192;
  for (size_t i = 0; i < n; i++) {
    const uint8_t* src = in + i * ib;
    uint64_t* o = out + i * 24;
    if (g2) status[i] = compressed ? w761_decode_row<4, true>(src, check != 0, o) : w761_decode_row<4, false>(src, check != 0, o);
    else status[i] = compressed ? w761_decode_row<-1, true>(src, check != 0, o) : w761_decode_row<-1, false>(src, check != 0, o);
  }
}
// the encoders (wire.h WireEnc, wire761.h) under bounds tracking: n rows -> wire bytes + status, what k_encode runs per lane.
// group 0 / 1: BLS12-377 G1 / G2 (rows 12 / 24 u64), 2: BW6-761 (24 u64); ark_zero: a row (0, 1 in Montgomery form) is the identity (the key writer's rule)
extern "C++" {
template <class E> static void encode_host(const uint64_t* rows, const uint8_t* inf, size_t n, int ark_zero, uint8_t* out, uint8_t* status) {
  for (size_t i = 0; i < n; i++) {
    uint64_t w[E::OUT_WORDS];
    status[i] = E::row(rows + i * E::ROW_WORDS, inf && inf[i], ark_zero != 0, w);
    memcpy(out + i * E::OUT_WORDS * 8, w, E::OUT_WORDS * 8);
  }
}
}  // extern "C++"
int ht_wire_encode(int group, int compressed, const uint64_t* rows, const uint8_t* inf, size_t n, int ark_zero, uint8_t* out, uint8_t* status) {
  switch (group * 2 + (compressed ? 1 : 0)) {
    case 0: encode_host<WireEncG1u>(rows, inf, n, ark_zero, out, status); break;
    case 1: encode_host<WireEncG1c>(rows, inf, n, ark_zero, out, status); break;
    case 2: encode_host<WireEncG2u>(rows, inf, n, ark_zero, out, status); break;
    case 3: encode_host<WireEncG2c>(rows, inf, n, ark_zero, out, status); break;
    case 4: encode_host<W761EncU>(rows, inf, n, ark_zero, out, status); break;
    case 5: encode_host<W761EncC>(rows, inf, n, ark_zero, out, status); break;
    default: return 2;
  }
  return 0;
}
// one arkworks Jacobian BW6-761 point (36 u64) -> 96 compressed bytes (the proof writer's per-point step); returns the status
int ht_wire761_encode_jacobian(const uint64_t* xyz, uint8_t* out96) {
  uint64_t w[12];
  const int st = w761_encode_jacobian(xyz, w);
  memcpy(out96, w, 96);
  return st;
}
int ht_wire761_key_size(size_t n_inputs, size_t n_vars, size_t n_h, int form, int vk_only, uint64_t* len) { return wkey_size(0, n_inputs, n_vars, n_h, form, vk_only, len); }
// the two forms of the subgroup test on one affine on-curve point (ark limbs): bit 0 = endomorphism form (what the decoders run),
// bit 1 = the r * P ladder (the reference's definition)
int ht_wire_subgroup_both(int g2, const uint64_t* xy) {
  const WireConsts& k = wire_consts();
  if (g2) {
    const Affine<Fq2> p = {{Fq::from_ark(xy), Fq::from_ark(xy + 6)}, {Fq::from_ark(xy + 12), Fq::from_ark(xy + 18)}};
    const Affine<Fq2> q = {Fq2::norm(p.x), Fq2::norm(p.y)};
    return (wire_in_subgroup(q, k) ? 1 : 0) | (wire_in_subgroup_ladder(q, k) ? 2 : 0);
  }
  const Affine<Fq> q = {Fq::norm(Fq::from_ark(xy)), Fq::norm(Fq::from_ark(xy + 6))};
  return (wire_in_subgroup(q, k) ? 1 : 0) | (wire_in_subgroup_ladder(q, k) ? 2 : 0);
}
// the two forms of the BW6-761 subgroup test on one affine on-curve point (24 u64, ark limbs): bit 0 = the endomorphism form
// (w761_in_subgroup_endo, what the decoders and check_points_* run), bit 1 = the r * P ladder (w761_in_subgroup, the definition)
int ht_w761_subgroup_both(int g2, const uint64_t* xy) {
  const Affine<Fw761> p = {Fw761::norm(Fw761::from_ark(xy)), Fw761::norm(Fw761::from_ark(xy + 12))};
  return ((g2 ? w761_in_subgroup_endo<4>(p) : w761_in_subgroup_endo<-1>(p)) ? 1 : 0) | (w761_in_subgroup(p) ? 2 : 0);
}
// check.h under bounds tracking: n rows of group cg (0 / 1: BLS12-377 G1 / G2, 2 / 3: BW6-761 G1 / G2) -> status, what k_check_rows and
// k_endo761 run per lane; inf may be NULL; ladder761: the BW6-761 rows take the ladder.  2 for a group or level that does not exist
int ht_check_rows(int cg, const uint64_t* xy, const uint8_t* inf, size_t n, int level, int ladder761, uint8_t* status) {
  if (cg < 0 || cg > 3 || level < 1 || level > 2) return 2;
  const WireConsts& k = wire_consts();
  for (size_t i = 0; i < n; i++) {
    const uint64_t* row = xy + i * check_row_words(cg);
    const bool f = inf && inf[i];
    status[i] = cg == 0 ? check_row<0>(row, f, level, k) : cg == 1 ? check_row<1>(row, f, level, k) : cg == 2 ? check_row<2>(row, f, level, k, ladder761 != 0)
                                                                                                       : check_row<3>(row, f, level, k, ladder761 != 0);
  }
  return 0;
}
// hash_direct.h under bounds tracking: one try-and-increment hash; returns the attempt counter, -1 when none succeeds
int ht_hash_to_g1_direct(const uint8_t* dom, const uint8_t* msg, size_t mlen, const uint8_t* extra, size_t elen, uint64_t* out_xy) {
  Affine<Fq> p = {Fq::zero(), Fq::zero()};
  int c = -1;
  if (!hash_to_g1_direct_tai(dom, msg, mlen, extra, elen, wire_consts(), p, c)) return -1;
  p.x.to_ark(out_xy);
  p.y.to_ark(out_xy + 6);
  return c;
}
// the other two modes of the same loop (hash_direct.h: TAI_XOF_ONLY, TAI_COMPOSITE) and the Pedersen CRH (pedersen.h) under bounds tracking.
// The generator table comes from the caller: gens_ark = nchunks x 4 points (g, 2g, 3g, 4g of chunk ch at rows 4 ch .. 4 ch + 3) x (X, Y, Z, T) x 6 ark
// limbs, the layout k_pedersen_crh indexes; a byte string longer than the table covers is refused (-2), as the entry points refuse one
// longer than the full table.
static std::vector<EdPoint> ht_load_gens(const uint64_t* gens_ark, size_t nchunks) {
  std::vector<EdPoint> g(nchunks * PEDERSEN_MULTIPLES);
  for (size_t i = 0; i < g.size(); i++) {
    const uint64_t* r = gens_ark + i * 24;
    g[i] = {SF::from(Fq::from_ark(r)), SF::from(Fq::from_ark(r + 6)), SF::from(Fq::from_ark(r + 12)), SF::from(Fq::from_ark(r + 18))};
  }
  return g;
}
int ht_hash_to_g1(int mode, const uint8_t* dom, const uint8_t* msg, size_t mlen, const uint8_t* extra, size_t elen, const uint64_t* gens_ark, size_t nchunks,
                  uint64_t* out_xy) {
  if (mode < TAI_DIRECT || mode > TAI_COMPOSITE) return -2;
  std::vector<EdPoint> gens;
  if (mode == TAI_COMPOSITE) {
    if (!gens_ark || ((1 + elen + mlen) * 8 + 2) / 3 > nchunks) return -2;
    gens = ht_load_gens(gens_ark, nchunks);
  }
  Affine<Fq> p = {Fq::zero(), Fq::zero()};
  int c = -1;
  if (!hash_to_g1_direct_tai(dom, msg, mlen, extra, elen, wire_consts(), p, c, 0, mode, gens.data())) return -1;
  p.x.to_ark(out_xy);
  p.y.to_ark(out_xy + 6);
  return c;
}
int ht_pedersen_crh(const uint64_t* gens_ark, size_t nchunks, const uint8_t* msg, size_t len, uint8_t* out48) {
  if ((len * 8 + 2) / 3 > nchunks) return -2;
  const std::vector<EdPoint> gens = ht_load_gens(gens_ark, nchunks);
  pedersen_crh(gens.data(), msg, len, out48);
  return 0;
}
// k_pedersen_crh_lanes of unit_hash_lanes.hip in host loops: the L lane sums one after the other, their partials folded through a buffer of L slots
// in the kernel's rounds, lane 0 finishing.  L: a power of two from 1 to 256 (-2 otherwise)
int ht_pedersen_crh_lanes(const uint64_t* gens_ark, size_t nchunks, const uint8_t* msg, size_t len, int L, uint8_t* out48) {
  if ((len * 8 + 2) / 3 > nchunks || !crh_lanes_ok(L)) return -2;
  const std::vector<EdPoint> gens = ht_load_gens(gens_ark, nchunks);
  std::vector<EdPoint> acc(L, ed_zero());
  std::vector<uint4> slots((size_t)L * CRH_SLOT_WORDS / 4);
  uint32_t* sl = reinterpret_cast<uint32_t*>(slots.data());
  for (int l = 0; l < L; l++) {
    acc[l] = pedersen_crh_lane_sum(gens.data(), PtrBytes{msg, len}, (uint32_t)l, (uint32_t)L);
    ed_store(sl + (size_t)l * CRH_SLOT_WORDS, acc[l]);
  }
  for (int s = L >> 1; s; s >>= 1) {
    for (int l = 0; l < s; l++) acc[l] = ed_add(acc[l], ed_load(sl + (size_t)(l + s) * CRH_SLOT_WORDS));
    if (s > 1) for (int l = 0; l < s; l++) ed_store(sl + (size_t)l * CRH_SLOT_WORDS, acc[l]);
  }
  pedersen_crh_finish(acc[0], out48);
  return 0;
}
uint32_t ht_crh_pick_lanes(uint32_t request, size_t max_chunks, size_t n) { return crh_pick_lanes(request, max_chunks, n); }
// scale_by_cofactor of one affine curve point (ark limbs): 1 and the affine multiple, 0 when the multiple is the identity (points of the
// cofactor subgroup: what k_hash_finish flags for the serial loop)
int ht_tai_finish(const uint64_t* xy, uint64_t* out_xy) {
  const Affine<Fq> p = {Fq::norm(Fq::from_ark(xy)), Fq::norm(Fq::from_ark(xy + 6))};
  Affine<Fq> r = {Fq::zero(), Fq::zero()};
  if (!tai_finish(p, r)) return 0;
  r.x.to_ark(out_xy);
  r.y.to_ark(out_xy + 6);
  return 1;
}
// the G2 twins (hash_direct.h: hash_to_g2_tai, tai_finish_g2): rows of 24 ark limbs x.c0, x.c1, y.c0, y.c1; compat as in the entry points
int ht_hash_to_g2(int mode, int compat, const uint8_t* dom, const uint8_t* msg, size_t mlen, const uint8_t* extra, size_t elen, const uint64_t* gens_ark,
                  size_t nchunks, uint64_t* out_xy) {
  if (mode < TAI_DIRECT || mode > TAI_COMPOSITE) return -2;
  std::vector<EdPoint> gens;
  if (mode == TAI_COMPOSITE) {
    if (!gens_ark || ((1 + elen + mlen) * 8 + 2) / 3 > nchunks) return -2;
    gens = ht_load_gens(gens_ark, nchunks);
  }
  Affine<Fq2> p = {Fq2::zero(), Fq2::zero()};
  int c = -1;
  if (!hash_to_g2_tai(dom, msg, mlen, extra, elen, compat, wire_consts(), p, c, 0, mode, gens.data())) return -1;
  p.x.to_ark(out_xy);
  p.y.to_ark(out_xy + 12);
  return c;
}
int ht_tai_finish_g2(const uint64_t* xy, uint64_t* out_xy) {
  const Affine<Fq2> p = {Fq2::norm(Fq2::from_ark(xy)), Fq2::norm(Fq2::from_ark(xy + 12))};
  Affine<Fq2> r = {Fq2::zero(), Fq2::zero()};
  if (!tai_finish_g2(p, r)) return 0;
  r.x.to_ark(out_xy);
  r.y.to_ark(out_xy + 12);
  return 1;
}
// table-driven root vs the Tonelli-Shanks loop on one Fq element (ark limbs): returns 1 + 2*(roots agree up to sign) when a root
// exists for both, 0 when both say non-residue, -1 on disagreement
int ht_wire_fq_sqrt_both(const uint64_t* a, uint64_t* out) {
  const Fq x = Fq::from_ark(a);
  Fq r1, r2;
  const bool o1 = wire_fq_sqrt(x, wire_consts(), r1), o2 = wire_fq_sqrt_ts(x, wire_consts(), r2);
  if (o1 != o2) return -1;
  if (!o1) return 0;
  r1.to_ark(out);
  const bool same = wire_eq(r1, r2) || wire_eq(r1, wire_neg(r2));
  return wire_eq(Fq::sqr(r1), x) && same ? 3 : -1;
}
// square root in Fq2 (ark limbs in and out); returns 1 when a root exists
int ht_wire_fq2_sqrt(const uint64_t* a, uint64_t* out) {
  Fq2 r;
  const Fq2 x = {Fq::from_ark(a), Fq::from_ark(a + 6)};
  if (!wire_fq2_sqrt(x, wire_consts(), r)) return 0;
  r.c0.to_ark(out);
  r.c1.to_ark(out + 6);
  return 1;
}
void ht_pairing_761_lanes(int mode, const uint64_t* g1, const uint64_t* g2, size_t k, uint64_t* out72, int* is_one) { pairing_op_761_lanes(mode, g1, g2, k, out72, is_one); }
void ht_pairing_761(int mode, const uint64_t* g1, const uint64_t* g2, size_t k, uint64_t* out72, int* is_one) { pairing_op_761(mode, g1, g2, k, out72, is_one); }
void ht_pairing_377(int mode, const uint64_t* g1, const uint64_t* g2, size_t k, const uint64_t* in72, const uint64_t* in72b,
                    uint64_t* out72, int* is_one) { pairing_op(mode, g1, g2, k, in72, in72b, out72, is_one); }
void ht_pairing_377_lanes(int mode, const uint64_t* g1, const uint64_t* g2, size_t k, const uint64_t* in72, const uint64_t* in72b,
                         uint64_t* out72, int* is_one) { pairing_op_lanes(mode, g1, g2, k, in72, in72b, out72, is_one); }
// modular inversion: the safegcd routine on plain integers (field 0: BLS12-377 Fq, 1: BW6-761 Fq), and Fp::inv against Fermat
void ht_modinv(int field, const uint64_t* x, uint64_t* out) {
  if (field == 0) SafeGcd<P377>::inv(x, out); else SafeGcd<P761>::inv(x, out);
}
int ht_inv_matches_fermat(int field, const uint64_t* ark) {
  if (field == 0) {
    const Fq a = Fq::from_ark(ark);
    return Fq::eq_mod_p(Fq::norm(Fq::inv(a)), Fq::norm(Fq::inv_fermat(a))) ? 1 : 0;
  }
  const Fw a = Fw::from_ark(ark);
  return Fw::eq_mod_p(Fw::norm(Fw::inv(a)), Fw::norm(Fw::inv_fermat(a))) ? 1 : 0;
}
void ht_pairing_377_hex(int mode, const uint64_t* g1, const uint64_t* g2, size_t k, const uint64_t* in72, const uint64_t* in72b,
                       uint64_t* out72, int* is_one) { pairing_op_hex(mode, g1, g2, k, in72, in72b, out72, is_one); }
void ht_fq377(int op, const uint64_t* a, const uint64_t* b, uint64_t* out) { field_op<Fp<P377>>(op, a, b, out); }
void ht_fq761(int op, const uint64_t* a, const uint64_t* b, uint64_t* out) { field_op<Fp<P761>>(op, a, b, out); }
// Fr(BLS12-377), the 10-limb field of the hash-helper proof's NTT (ntt.h); op 7 = weak reduction of a lazily grown sum (the butterfly's
// x + y path), op 8 = canonical-integer round trip
void ht_fr377(int op, const uint64_t* a, const uint64_t* b, uint64_t* out) {
  typedef Fp<P253> F;
  if (op == 7) { F x = F::from_ark(a), y = F::from_ark(b); F t = F::add(F::add(x, y), F::add(x, y)); t = F::add(t, t); F::wred(F::add(t, x)).to_ark(out); return; }   // 5x + 4y, value bound ~ 27p
  if (op == 8) { F x = F::from_canonical(a); x.to_canonical(out); return; }
  field_op<F>(op, a, b, out);
}
void ht_fq2_377(int op, const uint64_t* a, const uint64_t* b, uint64_t* out) { field_op<Fp2<P377>>(op, a, b, out); }
void ht_g1_377(int op, const uint64_t* p1, const uint64_t* p2, uint32_t k, uint64_t* out) { point_op<Fp<P377>>(op, p1, p2, k, out); }
void ht_g2_377(int op, const uint64_t* p1, const uint64_t* p2, uint32_t k, uint64_t* out) { point_op<Fp2<P377>>(op, p1, p2, k, out); }
void ht_lane_g1_377(int op, const uint64_t* p1, const uint64_t* p2, uint32_t k, uint64_t* out) { lane_point_op<Fp<P377>>(op, p1, p2, k, out); }
void ht_lane_g2_377(int op, const uint64_t* p1, const uint64_t* p2, uint32_t k, uint64_t* out) { lane_point_op<Fp2<P377>>(op, p1, p2, k, out); }
void ht_lane_g2_377_hex(int op, const uint64_t* p1, const uint64_t* p2, uint32_t k, uint64_t* out) { lane_point_op_hex(op, p1, p2, k, out); }
void ht_lane_g_761(int op, const uint64_t* p1, const uint64_t* p2, uint32_t k, uint64_t* out) { lane_point_op<Fp<P761>>(op, p1, p2, k, out); }
void ht_g_761(int op, const uint64_t* p1, const uint64_t* p2, uint32_t k, uint64_t* out) { point_op<Fp<P761>>(op, p1, p2, k, out); }
// Horner step lists (host64.h) on the 64-bit-limb path and on the IFMA path (host_ifma.cpp), field 0: BLS12-377 Fq, 1: BW6-761 Fq.
// out: X, Y, ZZ, ZZZ (arkworks form; all zero = identity).  ht_horner_ifma returns -1 without AVX-512 IFMA, 1 on a special case.
void ht_horner64(int field, const uint64_t* pts, size_t stride, const int32_t* order, int steps, uint64_t* out) {
  if (field == 0) { auto r = host64_horner<HFp<P377>>(pts, stride, 6, order, steps); r.X.store(out); r.Y.store(out + 6); r.ZZ.store(out + 12); r.ZZZ.store(out + 18); }
  else { auto r = host64_horner<HFp<P761>>(pts, stride, 12, order, steps); r.X.store(out); r.Y.store(out + 12); r.ZZ.store(out + 24); r.ZZZ.store(out + 36); }
}
int ht_horner_ifma(int field, const uint64_t* pts, size_t stride, const int32_t* order, int steps, uint64_t* out) {
  if (!celo_ifma_available()) return -1;
  int inf = 0;
  return field == 0 ? celo_ifma_horner_377(pts, stride, order, steps, out, &inf) : celo_ifma_horner_761(pts, stride, order, steps, out, &inf);
}
// base-x digits (gls.h) of a scalar of nw significant words into nd digits: d[4][2] words; the (nw, nd) pairs the batched MSM uses
int ht_gls_digits(int nw, int nd, const uint32_t* k8, uint32_t* d8) {
  uint32_t d[4][2];
  switch (nw * 10 + nd) {
    case 32: gls_digits_base_x<3, 2>(k8, d); break;
    case 42: gls_digits_base_x<4, 2>(k8, d); break;
    case 43: gls_digits_base_x<4, 3>(k8, d); break;
    case 53: gls_digits_base_x<5, 3>(k8, d); break;
    case 63: gls_digits_base_x<6, 3>(k8, d); break;
    case 64: gls_digits_base_x<6, 4>(k8, d); break;
    case 74: gls_digits_base_x<7, 4>(k8, d); break;
    case 84: gls_digits_base_x<8, 4>(k8, d); break;
    default: return 1;
  }
  for (int j = 0; j < 4; j++) { d8[2 * j] = d[j][0]; d8[2 * j + 1] = d[j][1]; }
  return 0;
}
void ht_glv_split(const uint32_t* k8, uint32_t* k0, uint32_t* k1) { glv_split_x2<8>(k8, k0, k1); }
void ht_fq377_canon(const uint64_t* canon, uint64_t* out_ark, uint64_t* out_canon) {
  Fp<P377> x = Fp<P377>::from_canonical(canon);
  x.to_ark(out_ark);
  x.to_canonical(out_canon);
}
// xyzz_add_affine on RAW device limbs (14 x 28 bits per coordinate, not necessarily on the curve: the formulas are rational functions
// of the coordinates): -(x1, y1) + (x2, y2) through the affine + affine start and through from_affine + xyzz_madd, both exported as
// Jacobian ark limbs.  The top-limb edge of ADVICE r3 (a negated y whose top limb is 4 p's own against a y whose top limb is zero)
// cannot be reached through from_ark, whose products pick the representative.
void ht_add_affine_raw_377(const uint32_t* x1, const uint32_t* y1, const uint32_t* x2, const uint32_t* y2, uint64_t* out_start, uint64_t* out_madd,
                           uint32_t* neg_y_top) {
  typedef Fp<P377> F;
  Affine<F> p = affine_neg(Affine<F>{F::from_limbs(x1), F::from_limbs(y1)}), q = {F::from_limbs(x2), F::from_limbs(y2)};
  *neg_y_top = p.y.l[F::L - 1];
  Xyzz<F> a = xyzz_add_affine(p, q);
  Xyzz<F> b = Xyzz<F>::from_affine(p);
  xyzz_madd(b, q);
  xyzz_to_jac(a, out_start);
  xyzz_to_jac(b, out_madd);
}

// ---- fixed_base.h: the table build, the digit recoding, the table lookup and the accumulation of unit_setup.hip's kernels, run in host loops
// (the affine form of each row by its own inversion, where the device batches them).  group: 0 BLS12-377 G1, 1 BLS12-377 G2, 2 BW6-761.
extern "C++" {
template <class F, int N64> static void fbm_host(const uint64_t* gen, const uint64_t* sc, size_t n, int c, int bits, uint64_t* out, uint8_t* inf) {
  constexpr int FW = F::WORDS, A = F::ARK64;
  const int W = fb_windows(bits, c);
  const uint32_t H = 1u << (c - 1), E = (uint32_t)W * H;
  std::vector<uint32_t> bases((size_t)W * 2 * FW), table((size_t)E * 2 * FW);
  std::vector<uint8_t> binf(W), tinf(E);
  const Affine<F> g = {F::norm(F::from_ark(gen)), F::norm(F::from_ark(gen + A))};
  for (int w = 0; w < W; w++) {
    Affine<F> b = {F::zero(), F::zero()};
    binf[w] = fb_to_affine(fb_window_base(g, w, c), b) ? 0 : 1;
    fb_store_entry(&bases[(size_t)w * 2 * FW], b);
  }
  for (uint32_t e = 0; e < E; e++) {
    const uint32_t w = e / H, d = e - w * H + 1;
    Affine<F> r = {F::zero(), F::zero()};
    bool ok = false;
    if (!binf[w]) ok = fb_to_affine(fb_table_entry(fb_load_entry<F>(&bases[(size_t)w * 2 * FW]), d), r);
    fb_store_entry(&table[(size_t)e * 2 * FW], r);
    tinf[e] = ok ? 0 : 1;
  }
  for (size_t i = 0; i < n; i++) {
    const Xyzz<F> a = fb_scalar_mul<F, N64>(sc + i * N64, table.data(), tinf.data(), c, W);
    Affine<F> r;
    uint64_t* o = out + i * 2 * A;
    if (fb_to_affine(a, r)) { r.x.to_ark(o); r.y.to_ark(o + A); inf[i] = 0; }
    else { for (int k = 0; k < 2 * A; k++) o[k] = 0; inf[i] = 1; }
  }
}
}  // extern "C++"
void ht_fixed_base_mul(int group, const uint64_t* gen, const uint64_t* sc, size_t n, int c, uint64_t* out, uint8_t* inf) {
  if (group == 0) fbm_host<Fp<P377>, 4>(gen, sc, n, c, 253, out, inf);
  else if (group == 1) fbm_host<Fp2<P377>, 4>(gen, sc, n, c, 253, out, inf);
  else fbm_host<Fp<P761>, 6>(gen, sc, n, c, 377, out, inf);
}
// ---- var_base.h: the per-lane table, the plain ladder, the subgroup (GLV) ladder and the shared-scalar form of unit_varbase.hip's kernels, run in
// host loops over the SAME lane-interleaved workspace (stride = n lanes); the affine form of each row by its own inversion, where the device
// batches them.  group: 0 BLS12-377 G1, 1 BLS12-377 G2, 2 BW6-761.  n_sc: n, or 1 for one scalar shared by every row.
extern "C++" {
template <class F> struct VbHost {
  static constexpr int FW = F::WORDS, A = F::ARK64;
  std::vector<uint4> chain, table;
  std::vector<uint8_t> tinf;
  size_t n;
  uint32_t H;
  VbHost(const uint64_t* xy, const uint8_t* inf, size_t n_, int c) : n(n_), H(1u << (c - 1)) {
    chain.resize((size_t)H * FW * n); table.resize((size_t)H * (2 * FW / 4) * n); tinf.resize((size_t)H * n);
    for (size_t i = 0; i < n; i++) {
      const Affine<F> p = {F::norm(F::from_ark(xy + i * 2 * A)), F::norm(F::from_ark(xy + i * 2 * A + A))};
      vb_build_table<F>(p, inf && inf[i], H, chain.data(), table.data(), tinf.data(), n, (uint32_t)i);
    }
  }
  static void row(const Xyzz<F>& a, uint64_t* o, uint8_t* inf) {
    Affine<F> r;
    if (fb_to_affine(a, r)) { r.x.to_ark(o); r.y.to_ark(o + A); *inf = 0; }
    else { for (int k = 0; k < 2 * A; k++) o[k] = 0; *inf = 1; }
  }
};
template <class F> static void vb_table_host(const uint64_t* xy, int inf, int c, uint64_t* out, uint8_t* oinf) {
  const uint8_t f = inf ? 1 : 0;
  VbHost<F> t(xy, &f, 1, c);
  for (uint32_t e = 0; e < t.H; e++) {
    oinf[e] = t.tinf[e];
    const Affine<F> p = vb_load_entry<F>(t.table.data(), 1, 0, e);
    uint64_t* o = out + (size_t)e * 2 * VbHost<F>::A;
    if (oinf[e]) for (int k = 0; k < 2 * VbHost<F>::A; k++) o[k] = 0;
    else { p.x.to_ark(o); p.y.to_ark(o + VbHost<F>::A); }
  }
}
template <class F, int N64> static void vb_mul_host(const uint64_t* xy, const uint8_t* inf, const uint64_t* sc, size_t n_sc, size_t n, int c, int bits, int glv,
                                                    uint64_t* out, uint8_t* oinf) {
  VbHost<F> t(xy, inf, n, c);
  for (size_t i = 0; i < n; i++) {
    const uint64_t* s = sc + (n_sc == 1 ? 0 : i) * N64;
    Xyzz<F> a;
    if constexpr (N64 == 4 && sizeof(F) <= 64) a = glv ? vb_ladder_glv<F>(s, c, t.table.data(), t.tinf.data(), n, (uint32_t)i)
                                                        : vb_ladder<F, N64>(s, bits, c, t.table.data(), t.tinf.data(), n, (uint32_t)i);
    else a = vb_ladder<F, N64>(s, bits, c, t.table.data(), t.tinf.data(), n, (uint32_t)i);
    VbHost<F>::row(a, out + i * 2 * VbHost<F>::A, oinf + i);
  }
}
}  // extern "C++"
// the table of ONE point: out 2^(c-1) rows [e + 1]P (affine arkworks limbs, zero rows for identities), oinf their flags
void ht_var_base_table(int group, const uint64_t* xy, int inf, int c, uint64_t* out, uint8_t* oinf) {
  if (group == 0) vb_table_host<Fp<P377>>(xy, inf, c, out, oinf);
  else if (group == 1) vb_table_host<Fp2<P377>>(xy, inf, c, out, oinf);
  else vb_table_host<Fp<P761>>(xy, inf, c, out, oinf);
}
// out[i] = [k_i] P_i by the plain ladder (glv = 0) or, group 0 only, the subgroup ladder (glv = 1)
void ht_var_base_mul(int group, int glv, const uint64_t* xy, const uint8_t* inf, const uint64_t* sc, size_t n_sc, size_t n, int c, uint64_t* out, uint8_t* oinf) {
  if (group == 0) vb_mul_host<Fp<P377>, 4>(xy, inf, sc, n_sc, n, c, 253, glv, out, oinf);
  else if (group == 1) vb_mul_host<Fp2<P377>, 4>(xy, inf, sc, n_sc, n, c, 253, 0, out, oinf);
  else vb_mul_host<Fp<P761>, 6>(xy, inf, sc, n_sc, n, c, 377, 0, out, oinf);
}
// ---- aggregate.h: k_seal_count and k_masked_sum of unit_seals.hip in host loops - the L lanes of a sum one after the other, their partials
// folded through a buffer of L slots in the kernel's rounds, the complement by the kernel's rule - and each row's affine form by its own
// inversion.  group 0 / 1: BLS12-377 G1 / G2.  offsets, n_sets, bits, m: as aggregate_by_bitmap_*; complement: -1 / 0 / 1.
extern "C++" {
template <class F>
static Xyzz<F> agg_sum_host(const uint64_t* xy, const uint8_t* inf, const uint8_t* bits, uint32_t n, uint32_t L, bool neg, const uint32_t* total) {
  const size_t SW = agg_slot_words<F>();
  std::vector<Xyzz<F>> acc(L);
  std::vector<uint4> slots(L * SW / 4);
  uint32_t* sl = reinterpret_cast<uint32_t*>(slots.data());
  for (uint32_t l = 0; l < L; l++) {
    acc[l] = agg_lane_sum<F>(xy, inf, bits, n, l, L, neg);
    agg_store<F>(sl + l * SW, acc[l]);
  }
  for (uint32_t s = L >> 1; s; s >>= 1) {
    for (uint32_t l = 0; l < s; l++) agg_fold_step<F>(acc[l], sl, l, s);
    if (s > 1) for (uint32_t l = 0; l < s; l++) agg_store<F>(sl + l * SW, acc[l]);
  }
  agg_finish<F>(acc[0], neg, total);
  return acc[0];
}
template <class F>
static void agg_host(const uint64_t* xy, const uint8_t* inf, const uint32_t* off, size_t n_sets, const uint8_t* bits, size_t m, int L, int complement, uint64_t* out,
                     uint8_t* oinf, uint32_t* count) {
  constexpr int A = F::ARK64;
  const bool shared = n_sets == 1;
  std::vector<uint4> total(F::WORDS);
  uint32_t* tw = reinterpret_cast<uint32_t*>(total.data());
  if (shared) agg_store<F>(tw, agg_sum_host<F>(xy + (size_t)off[0] * 2 * A, inf ? inf + off[0] : nullptr, nullptr, off[1] - off[0], AGG_MAX_LANES, false, nullptr));
  for (size_t i = 0; i < m; i++) {
    const uint32_t row0 = shared ? off[0] : off[i], n = shared ? off[1] - off[0] : off[i + 1] - off[i];
    const uint8_t* b = bits + (shared ? i * (size_t)n : (size_t)off[i]);
    const uint32_t c = agg_count(b, n);
    const bool neg = agg_side(c, n, complement, shared);
    const uint32_t lanes = L ? (uint32_t)L : agg_pick_lanes(neg ? n - c : c, m);
    const Xyzz<F> a = agg_sum_host<F>(xy + (size_t)row0 * 2 * A, inf ? inf + row0 : nullptr, b, n, lanes, neg, tw);
    count[i] = c;
    Affine<F> r;
    uint64_t* o = out + i * 2 * A;
    if (fb_to_affine(a, r)) { r.x.to_ark(o); r.y.to_ark(o + A); oinf[i] = 0; }
    else { for (int k = 0; k < 2 * A; k++) o[k] = 0; oinf[i] = 1; }
  }
}
}  // extern "C++"
void ht_aggregate_by_bitmap(int group, const uint64_t* xy, const uint8_t* inf, const uint32_t* off, size_t n_sets, const uint8_t* bits, size_t m, int lanes, int complement,
                            uint64_t* out, uint8_t* oinf, uint32_t* count) {
  if (group == 0) agg_host<Fp<P377>>(xy, inf, off, n_sets, bits, m, lanes, complement, out, oinf, count);
  else agg_host<Fp2<P377>>(xy, inf, off, n_sets, bits, m, lanes, complement, out, oinf, count);
}
uint32_t ht_aggregate_pick_lanes(uint32_t max_adds, size_t m) { return agg_pick_lanes(max_adds, m); }
// ---- groth16_verify.h: the lane routines of groth16_verify_unit.h's kernels in host loops, one template over the curve description; the
// exported twins are its two instantiations (BW6-761: rows of 24 u64, inputs of 6; BLS12-377: G1 rows of 12 u64, inputs of 4).
// g16_input_row_host: abc n_abc G1 rows (affine arkworks limbs, none the identity), inputs n x (n_abc - 1) canonical scalars, window bits c ->
// out n G1 rows (a zero row and inf = 1 for the identity), status[i] = 1 for a row with an input that is not below r.  The tables are built as
// k_fbm_bases / k_fbm_table build them, one per base.
extern "C++" {
// the affine forms of a list of XYZZ points by one inversion for the whole list (Montgomery's trick); ok[k] = 0: the identity
template <class F> static void g16_batch_affine(const std::vector<Xyzz<F>>& pts, std::vector<Affine<F>>& out, std::vector<uint8_t>& ok) {
  const size_t n = pts.size();
  std::vector<F> t(n, F::zero()), pre(n, F::zero());
  out.assign(n, Affine<F>{F::zero(), F::zero()});
  ok.assign(n, 0);
  F run = F::one();
  for (size_t k = 0; k < n; k++) {
    if (pts[k].is_identity() || pts[k].ZZ.is_zero_mod_p()) continue;
    ok[k] = 1;
    t[k] = F::norm(F::mul(pts[k].ZZ, pts[k].ZZZ));
    pre[k] = run;
    run = F::norm(F::mul(run, t[k]));
  }
  F inv = F::norm(F::inv(run));
  for (size_t k = n; k-- > 0;) {
    if (!ok[k]) continue;
    const F ti = F::norm(F::mul(inv, pre[k]));
    inv = F::norm(F::mul(inv, t[k]));
    out[k] = {F::norm(F::mul(pts[k].X, F::mul(ti, pts[k].ZZZ))), F::norm(F::mul(pts[k].Y, F::mul(ti, pts[k].ZZ)))};
  }
}
// the key's side of an input sum as vk_build leaves it: gamma_abc[0] as a table entry and one window table per input base - the points of
// k_fbm_bases / k_fbm_table (fb_window_base, fb_table_entry), made affine list by list: the W window bases of a base, then its W 2^(c-1)
// entries - two inversions per base where one per entry took 20 s for the 10^5 entries of a 257-input key
template <class C> struct G16HostTables {
  typedef typename C::F F;
  static constexpr int FW = F::WORDS, A = F::ARK64, W1 = C::G1W;
  size_t n_in;
  int c, W;
  std::vector<uint64_t> rows;          // the gamma_abc rows the tables were made from
  std::vector<uint32_t> table, abc0;
  std::vector<uint8_t> tinf;
  G16HostTables(const uint64_t* abc, size_t n_abc, int c_) : n_in(n_abc - 1), c(c_), W(fb_windows(C::SCALAR_BITS, c_)), rows(abc, abc + n_abc * W1) {
    const uint32_t H = 1u << (c - 1), E = (uint32_t)W * H;
    table.resize((size_t)(n_in ? n_in : 1) * E * 2 * FW);
    abc0.resize(2 * FW);
    tinf.resize((size_t)(n_in ? n_in : 1) * E);
    fb_store_entry(abc0.data(), Affine<F>{F::norm(F::from_ark(abc)), F::norm(F::from_ark(abc + A))});
    std::vector<Xyzz<F>> wb(W), ent(E);
    std::vector<Affine<F>> wa, ea;
    std::vector<uint8_t> wok, eok;
    for (size_t j = 0; j < n_in; j++) {
      const uint64_t* gen = abc + (j + 1) * W1;
      const Affine<F> g = {F::norm(F::from_ark(gen)), F::norm(F::from_ark(gen + A))};
      for (int w = 0; w < W; w++) wb[w] = fb_window_base(g, w, c);
      g16_batch_affine(wb, wa, wok);
      for (int w = 0; w < W; w++)
        for (uint32_t d = 1; d <= H; d++) ent[(size_t)w * H + d - 1] = wok[w] ? fb_table_entry(wa[w], d) : Xyzz<F>::identity();
      g16_batch_affine(ent, ea, eok);
      for (uint32_t e = 0; e < E; e++) {
        fb_store_entry(&table[(j * E + e) * 2 * FW], ea[e]);
        tinf[j * E + e] = eok[e] ? 0 : 1;
      }
    }
  }
  // the tables of the last key, kept: a key whose rows are a prefix of it (tables are base-major) at the same window bits reuses them
  static std::shared_ptr<const G16HostTables> of(const uint64_t* abc, size_t n_abc, int c) {
    static std::mutex mu;
    static std::shared_ptr<const G16HostTables> last;
    std::lock_guard<std::mutex> lk(mu);
    if (!last || last->c != c || last->rows.size() < n_abc * W1 || memcmp(last->rows.data(), abc, n_abc * W1 * 8) != 0) last.reset(new G16HostTables(abc, n_abc, c));
    return last;
  }
  static void write_row(const Xyzz<F>& a, uint64_t* o, uint8_t* inf) {
    Affine<F> r;
    if (fb_to_affine(a, r)) { r.x.to_ark(o); r.y.to_ark(o + A); *inf = 0; }
    else { for (int k = 0; k < W1; k++) o[k] = 0; *inf = 1; }
  }
};
template <class C>
static void g16_input_row_host(const uint64_t* abc, size_t n_abc, const uint64_t* inputs, size_t n, int c, uint64_t* out, uint8_t* inf, uint8_t* status) {
  const auto tables = G16HostTables<C>::of(abc, n_abc, c);
  const G16HostTables<C>& T = *tables;
  const size_t n_in = n_abc - 1;
  for (size_t i = 0; i < n; i++) {
    uint32_t bad = 0;
    const Xyzz<typename C::F> a = g16_input_row<C>(inputs + i * n_in * C::N64, (uint32_t)n_in, T.abc0.data(), false, T.table.data(), T.tinf.data(), c, T.W, &bad);
    G16HostTables<C>::write_row(a, out + i * C::G1W, &inf[i]);
    status[i] = bad ? 1 : 0;
  }
}
// k_g16_inputs_lanes in host loops: the L lanes of a sum one after the other, their partials folded through a buffer of L / 2 slots in the
// kernel's rounds (the upper half of a round's lanes stores, then the lower half adds)
template <class C>
static void g16_input_lanes_host(const uint64_t* abc, size_t n_abc, const uint64_t* inputs, size_t n, int c, uint32_t L, uint64_t* out, uint8_t* inf, uint8_t* status) {
  typedef typename C::F F;
  const auto tables = G16HostTables<C>::of(abc, n_abc, c);
  const G16HostTables<C>& T = *tables;
  const size_t n_in = n_abc - 1;
  const size_t SW = agg_slot_words<F>();
  std::vector<Xyzz<F>> acc(L);
  std::vector<uint4> slots((L / 2 ? L / 2 : 1) * SW / 4);
  uint32_t* sl = reinterpret_cast<uint32_t*>(slots.data());
  for (size_t i = 0; i < n; i++) {
    uint32_t bad = 0;
    for (uint32_t l = 0; l < L; l++) {
      uint32_t b = 0;
      acc[l] = g16_lane_sum<C>(inputs + i * n_in * C::N64, (uint32_t)n_in, l, L, T.abc0.data(), false, T.table.data(), T.tinf.data(), c, T.W, &b);
      bad |= b;
    }
    for (uint32_t s = L >> 1; s; s >>= 1) {
      for (uint32_t l = s; l < 2 * s; l++) g16_fold_put<F>(sl, acc[l], l, s);
      for (uint32_t l = 0; l < s; l++) g16_fold_take<F>(acc[l], sl, l);
    }
    G16HostTables<C>::write_row(acc[0], out + i * C::G1W, &inf[i]);
    status[i] = bad ? 1 : 0;
  }
}
// out[i] = (2^127 | low 127 bits of r2[i]) xy[i] for n affine G1 points and n pairs of u64
template <class C> static void g16_scale_host(const uint64_t* xy, const uint64_t* r2, size_t n, uint64_t* out, uint8_t* inf) {
  typedef typename C::F F;
  constexpr int A = F::ARK64, W1 = C::G1W;
  for (size_t i = 0; i < n; i++) {
    const Affine<F> p = {F::norm(F::from_ark(xy + i * W1)), F::norm(F::from_ark(xy + i * W1 + A))};
    uint64_t lo, hi;
    g16_exponent(r2[2 * i], r2[2 * i + 1], lo, hi);
    const Xyzz<F> a = g16_scale128(p, lo, hi);
    Affine<F> r;
    uint64_t* o = out + i * W1;
    if (fb_to_affine(a, r)) { r.x.to_ark(o); r.y.to_ark(o + A); inf[i] = 0; }
    else { for (int k = 0; k < W1; k++) o[k] = 0; inf[i] = 1; }
  }
}
// the host parse of a serialized verifying key.  rows: (4 + n_abc) x 24 u64 on both curves, with room for cap rows; *n_abc out; *first_bad
// (may be NULL): the index of the point that was refused with 33
template <class C>
static int g16_vk_parse_host(const uint8_t* bytes, size_t len, size_t cap, uint64_t* rows, uint8_t* inf, uint64_t* n_abc, uint64_t* first_bad, size_t max_inputs = G16_MAX_INPUTS) {
  std::vector<uint64_t> r;
  std::vector<uint8_t> f;
  const int rc = g16_vk_parse<C>(bytes, len, r, f, first_bad, max_inputs);
  if (rc) return rc;
  if (f.size() > cap) return 2;
  memcpy(rows, r.data(), r.size() * 8);
  memcpy(inf, f.data(), f.size());
  *n_abc = f.size() - 4;
  return 0;
}
}  // extern "C++"
void ht_g16_input_row(const uint64_t* abc, size_t n_abc, const uint64_t* inputs, size_t n, int c, uint64_t* out, uint8_t* inf, uint8_t* status) {
  g16_input_row_host<G16Bw6>(abc, n_abc, inputs, n, c, out, inf, status);
}
void ht_g16_input_row_377(const uint64_t* abc, size_t n_abc, const uint64_t* inputs, size_t n, int c, uint64_t* out, uint8_t* inf, uint8_t* status) {
  g16_input_row_host<G16Bls>(abc, n_abc, inputs, n, c, out, inf, status);
}
void ht_g16_scale(const uint64_t* xy, const uint64_t* r2, size_t n, uint64_t* out, uint8_t* inf) { g16_scale_host<G16Bw6>(xy, r2, n, out, inf); }
void ht_g16_scale_377(const uint64_t* xy, const uint64_t* r2, size_t n, uint64_t* out, uint8_t* inf) { g16_scale_host<G16Bls>(xy, r2, n, out, inf); }
int ht_g16_vk_parse(const uint8_t* bytes, size_t len, size_t cap, uint64_t* rows, uint8_t* inf, uint64_t* n_abc) {
  return g16_vk_parse_host<G16Bw6>(bytes, len, cap, rows, inf, n_abc, nullptr);
}
int ht_g16_vk_parse_377(const uint8_t* bytes, size_t len, size_t cap, uint64_t* rows, uint8_t* inf, uint64_t* n_abc, uint64_t* first_bad) {
  return g16_vk_parse_host<G16Bls>(bytes, len, cap, rows, inf, n_abc, first_bad);
}
int ht_g16_window_bits(size_t n_in) { return g16_window_bits<G16Bw6>(n_in); }
int ht_g16_window_bits_377(size_t n_in) { return g16_window_bits<G16Bls>(n_in); }
// the wide loaders of BLS12-377 (up to G16_MAX_INPUTS_WIDE inputs): the lane sum and fold for a given L (2: L is no power of two in 1 .. 256),
// the window rule past 64 inputs (-1 above the limit), the width rule and the parse
int ht_g16_input_lanes_377(const uint64_t* abc, size_t n_abc, const uint64_t* inputs, size_t n, int c, int lanes, uint64_t* out, uint8_t* inf, uint8_t* status) {
  if (!g16_lanes_ok(lanes) || n_abc == 0 || n_abc - 1 > G16_MAX_INPUTS_WIDE) return 2;
  g16_input_lanes_host<G16Bls>(abc, n_abc, inputs, n, c, (uint32_t)lanes, out, inf, status);
  return 0;
}
int ht_g16_window_bits_wide_377(size_t n_in) { return n_in > G16_MAX_INPUTS_WIDE ? -1 : g16_window_bits<G16Bls>(n_in); }
uint32_t ht_g16_pick_lanes(size_t n_in, size_t m) { return g16_pick_lanes(n_in, m); }
int ht_g16_vk_parse_wide_377(const uint8_t* bytes, size_t len, size_t cap, uint64_t* rows, uint8_t* inf, uint64_t* n_abc, uint64_t* first_bad) {
  return g16_vk_parse_host<G16Bls>(bytes, len, cap, rows, inf, n_abc, first_bad, G16_MAX_INPUTS_WIDE);
}
// the setup's scalar lists as unit_setup.hip lays them out: G1 [alpha, beta, delta, gamma_abc, a, b, h, l], G2 [beta, gamma, delta, b]
extern "C++" {
template <class FR> static void setup_host(const uint64_t* qa, const uint64_t* qb, const uint64_t* qc, size_t n_vars, size_t n_inputs, const uint64_t* zt,
                                           const uint64_t* tau, size_t n_h, const uint64_t* toxic, uint64_t* g1s, uint64_t* g2s) {
  constexpr int N = FR::ARK64;
  const FR alpha = FR::norm(FR::from_ark(toxic)), beta = FR::norm(FR::from_ark(toxic + N));
  const FR ginv = FR::norm(FR::inv(FR::norm(FR::from_ark(toxic + 2 * N)))), dinv = FR::norm(FR::inv(FR::norm(FR::from_ark(toxic + 3 * N))));
  setup_canon<FR>(toxic, g1s); setup_canon<FR>(toxic + N, g1s + N); setup_canon<FR>(toxic + 3 * N, g1s + 2 * N);
  setup_canon<FR>(toxic + N, g2s); setup_canon<FR>(toxic + 2 * N, g2s + N); setup_canon<FR>(toxic + 3 * N, g2s + 2 * N);
  const size_t off_abc = 3, off_a = off_abc + n_inputs, off_b = off_a + n_vars, off_h = off_b + n_vars, off_l = off_h + n_h;
  for (size_t i = 0; i < n_vars; i++) {
    const bool inst = i < n_inputs;
    setup_lc<FR>(qa + i * N, qb + i * N, qc + i * N, alpha, beta, inst ? ginv : dinv, g1s + (inst ? off_abc + i : off_l + (i - n_inputs)) * N);
    setup_canon<FR>(qa + i * N, g1s + (off_a + i) * N);
    setup_canon<FR>(qb + i * N, g1s + (off_b + i) * N);
    setup_canon<FR>(qb + i * N, g2s + (3 + i) * N);
  }
  if (n_h) {
    const FR zt_dinv = FR::norm(FR::mul(FR::from_ark(zt), dinv)), t = FR::norm(FR::from_ark(tau));
    for (size_t i0 = 0; i0 < n_h; i0 += SETUP_H_BLOCK) {
      const uint32_t cnt = n_h - i0 < SETUP_H_BLOCK ? (uint32_t)(n_h - i0) : SETUP_H_BLOCK;
      setup_h_block<FR>(zt_dinv, t, i0, cnt, g1s + (off_h + i0) * N);
    }
  }
}
}  // extern "C++"
void ht_setup_scalars(int curve, const uint64_t* qa, const uint64_t* qb, const uint64_t* qc, size_t n_vars, size_t n_inputs, const uint64_t* zt,
                      const uint64_t* tau, size_t n_h, const uint64_t* toxic, uint64_t* g1s, uint64_t* g2s) {
  if (curve == 0) setup_host<Fp<P377>>(qa, qb, qc, n_vars, n_inputs, zt, tau, n_h, toxic, g1s, g2s);
  else setup_host<Fp<P253>>(qa, qb, qc, n_vars, n_inputs, zt, tau, n_h, toxic, g1s, g2s);
}

// ---- r1cs.h: the validation of groth16_r1cs_load_*, and the bodies of unit_r1cs.hip's kernels in host loops (the product in the kernels'
// short / chunk / combine order).  curve 0 = BW6-761 (Fr 6 u64), 1 = BLS12-377 (4 u64).  Matrices: three CSR structures in a, b, c order.
int ht_r1cs_validate(int curve, size_t rows, size_t n_vars, size_t n_inputs, const uint64_t* const* row_ptr, const uint32_t* const* col, const uint64_t* const* val,
                     const uint64_t* nnz, uint64_t* first_bad) {
  const R1csCsr mats[3] = {{row_ptr[0], col[0], val[0], nnz[0]}, {row_ptr[1], col[1], val[1], nnz[1]}, {row_ptr[2], col[2], val[2], nnz[2]}};
  return curve == 0 ? r1cs_validate<6>(rows, n_vars, n_inputs, mats, P377::P64, first_bad) : r1cs_validate<4>(rows, n_vars, n_inputs, mats, P253::P64, first_bad);
}
// the constants the tests' generators must know: the list length above which a list is cut, the chunk size, terms between weak reductions
void ht_r1cs_params(uint32_t out[3]) { out[0] = R1CS_LONG; out[1] = R1CS_CHUNK; out[2] = R1CS_LAZY; }
// out = M vec over the matrix's rows (ht_r1cs_rows: vec = the assignment)
void ht_r1cs_rows(int curve, const uint64_t* row_ptr, const uint32_t* col, const uint64_t* val, size_t rows, const uint64_t* vec, uint64_t* out) {
  if (curve == 0) r1cs_matvec_host<Fp<P377>>(row_ptr, col, val, rows, vec, out);
  else r1cs_matvec_host<Fp<P253>>(row_ptr, col, val, rows, vec, out);
}
extern "C++" {
template <class FR> static void lagrange_host(unsigned log_n, const uint64_t* omega, const uint64_t* tau, uint64_t* out, uint64_t* zt) {
  const R1csLagConsts<FR> k = r1cs_lagrange_consts<FR>(log_n, omega, tau, zt);
  const uint64_t n = uint64_t(1) << log_n;
  for (uint64_t j0 = 0; j0 < n; j0 += R1CS_LAG_BLOCK)
    r1cs_lagrange_block(k.c, k.tau, k.omega, k.omega_inv, j0, n - j0 < R1CS_LAG_BLOCK ? (uint32_t)(n - j0) : R1CS_LAG_BLOCK, out);
}
// the transpose of the matrix (r1cs_transpose) times vec, over the n_vars columns; then a_i += extra_i for i < n_extra (the matrix a: L_(rows + i))
template <class FR> static void cols_host(const uint64_t* row_ptr, const uint32_t* col, const uint64_t* val, size_t rows, size_t n_vars, const uint64_t* vec,
                                          size_t n_extra, uint64_t* out) {
  constexpr int A = FR::ARK64;
  std::vector<uint64_t> t_ptr, t_val;
  std::vector<uint32_t> t_idx;
  r1cs_transpose<A>(rows, n_vars, R1csCsr{row_ptr, col, val, row_ptr[rows]}, t_ptr, t_idx, t_val);
  r1cs_matvec_host<FR>(t_ptr.data(), t_idx.data(), t_val.data(), n_vars, vec, out);
  for (size_t i = 0; i < n_extra; i++) r1cs_add_input<FR>(out + i * A, vec + (rows + i) * A);
}
}  // extern "C++"
void ht_r1cs_lagrange(int curve, unsigned log_n, const uint64_t* omega, const uint64_t* tau, uint64_t* out, uint64_t* zt) {
  if (curve == 0) lagrange_host<Fp<P377>>(log_n, omega, tau, out, zt);
  else lagrange_host<Fp<P253>>(log_n, omega, tau, out, zt);
}
void ht_r1cs_cols(int curve, const uint64_t* row_ptr, const uint32_t* col, const uint64_t* val, size_t rows, size_t n_vars, const uint64_t* vec, size_t n_extra,
                  uint64_t* out) {
  if (curve == 0) cols_host<Fp<P377>>(row_ptr, col, val, rows, n_vars, vec, n_extra, out);
  else cols_host<Fp<P253>>(row_ptr, col, val, rows, n_vars, vec, n_extra, out);
}
// (A z)_j (B z)_j == (C z)_j over n rows: the smallest failing j, or -1 (the twin of k_r1cs_check)
int64_t ht_r1cs_check_rows(int curve, const uint64_t* a, const uint64_t* b, const uint64_t* c, size_t n) {
  const int A = curve == 0 ? 6 : 4;
  for (size_t j = 0; j < n; j++) {
    const bool ok = curve == 0 ? r1cs_row_holds<Fp<P377>>(a + j * A, b + j * A, c + j * A) : r1cs_row_holds<Fp<P253>>(a + j * A, b + j * A, c + j * A);
    if (!ok) return (int64_t)j;
  }
  return -1;
}
// ---- epoch.h under bounds tracking: the twins of k_epoch_key_record, k_epoch_pack, k_epoch_blake2s and k_epoch_inputs (the same templates).
// One block of `kind` from affine rows (24 u64, inf or NULL) to its bytes (out: epoch_encoded_size of them, every word through
// epoch_pack_word) and, for kind 2, its 7 bytes of extra data.  sum_row / sum_inf: the aggregated key of the last-epoch form, from the caller.
int64_t ht_epoch_encode(int kind, uint32_t index, uint32_t round, uint32_t max_non_signers, uint32_t max_validators, const uint8_t* epoch_entropy,
                        const uint8_t* parent_entropy, const uint64_t* rows, const uint8_t* inf, uint32_t n_keys, const uint64_t* sum_row, int sum_inf, uint8_t* out,
                        uint64_t cap, uint8_t* extra) {
  if (kind < 0 || kind >= EPOCH_KINDS || !epoch_block_ok(n_keys, max_validators)) return -2;
  const uint64_t bytes = (epoch_encoded_bits(kind, n_keys, max_validators) + 7) / 8;
  if (bytes > cap) return -1;
  std::vector<uint32_t> recs((size_t)(n_keys + 1) * EPOCH_REC_WORDS);
  for (uint32_t i = 0; i < n_keys; i++) epoch_key_record(rows + (size_t)i * 24, inf && inf[i], recs.data() + (size_t)i * EPOCH_REC_WORDS);
  uint64_t gen[24];
  Fq::from_limbs(T377::G2_GEN_X0).to_ark(gen); Fq::from_limbs(T377::G2_GEN_X1).to_ark(gen + 6);
  Fq::from_limbs(T377::G2_GEN_Y0).to_ark(gen + 12); Fq::from_limbs(T377::G2_GEN_Y1).to_ark(gen + 18);
  epoch_key_record(gen, false, recs.data() + (size_t)n_keys * EPOCH_REC_WORDS);
  uint32_t sum[EPOCH_REC_WORDS] = {}, hd[EPOCH_HDR_WORDS];
  if (kind == 1) epoch_key_record(sum_row, sum_inf != 0, sum);
  epoch_header(kind, index, max_non_signers, epoch_entropy, parent_entropy, hd);
  const uint32_t nk = epoch_key_slots(kind, n_keys, max_validators);
  const uint64_t words = (bytes + 63) / 64 * 16;           // the slot of k_epoch_pack: the padding must come out zero
  for (uint64_t w = 0; w < words; w++) {
    const uint32_t v = epoch_pack_word(kind, w, n_keys, nk, hd, recs.data(), recs.data() + (size_t)n_keys * EPOCH_REC_WORDS, sum);
    for (int b = 0; b < 4; b++) {
      const uint64_t j = 4 * w + b;
      if (j < bytes) out[j] = (uint8_t)(v >> (8 * b));
      else if ((uint8_t)(v >> (8 * b))) return -3;
    }
  }
  if (kind == 2 && extra) epoch_extra(index, round, max_non_signers, extra);
  return (int64_t)bytes;
}
// transitions.h: the rule k_transition_status runs, one block from its facts.  f: initial, bad_key, pred_bad_key, index, pred_index, n_keys,
// pred_n_keys, entropy_live, entropy_equal, signers, pred_max_non_signers, padding_selected, sig_wire, attempt
int ht_transition_status(const uint32_t f[14]) {
  TransitionFacts t = {};
  t.initial = f[0] != 0; t.bad_key = f[1] != 0; t.pred_bad_key = f[2] != 0; t.index = f[3]; t.pred_index = f[4]; t.n_keys = f[5]; t.pred_n_keys = f[6];
  t.entropy_live = f[7] != 0; t.entropy_equal = f[8] != 0; t.signers = f[9]; t.pred_max_non_signers = f[10]; t.padding_selected = f[11] != 0;
  t.sig_wire = (uint8_t)f[12]; t.attempt = (uint8_t)f[13];
  return transition_status(t);
}
// the helpers that gather the facts: entropy rows (NULL = all zero) and the padding-key scan over rows of 24 u64
int ht_transition_entropy(const uint8_t* a, uint64_t i, const uint8_t* b, uint64_t j) {
  return (transition_entropy_equal(a, i, b, j) ? 1 : 0) | (transition_entropy_nonzero(a, i) ? 2 : 0);
}
int ht_transition_padding(const uint64_t* rows, const uint8_t* inf, const uint8_t* bits, uint32_t k0, uint32_t k1, const uint64_t* gen) {
  return transition_padding_selected(rows, inf, bits, k0, k1, gen) ? 1 : 0;
}
void ht_epoch_key_record(const uint64_t* row, int inf, uint32_t* rec24) { epoch_key_record(row, inf != 0, rec24); }
void ht_epoch_blake2s(const uint8_t* msg, uint64_t len, uint8_t* out32) {
  std::vector<uint32_t> slot((len + 63) / 64 * 16 + 16, 0);
  for (uint64_t j = 0; j < len; j++) slot[j / 4] |= (uint32_t)msg[j] << (8 * (j % 4));
  uint32_t h[8];
  epoch_blake2s(slot.data(), len, h);
  for (int i = 0; i < 32; i++) out32[i] = (uint8_t)(h[i / 4] >> (8 * (i % 4)));
}
void ht_epoch_inputs(const uint8_t* h_first32, const uint8_t* h_last32, uint64_t* out12) {
  uint32_t a[8] = {}, b[8] = {};
  for (int i = 0; i < 32; i++) { a[i / 4] |= (uint32_t)h_first32[i] << (8 * (i % 4)); b[i / 4] |= (uint32_t)h_last32[i] << (8 * (i % 4)); }
  epoch_inputs(a, b, out12);
}
// ---- dedup.h: the host twin of k_dedup_insert / k_dedup_rep (the same templates, key after key).  kb: 48 or 96
uint64_t ht_dedup_mix(int kb, const uint8_t* key) { return kb == 96 ? dedup_hash<96, false>(key) : dedup_hash<48, false>(key); }
uint64_t ht_dedup_slots(uint64_t n, int slack_log) { return dedup_slots(n, slack_log); }
int ht_dedup_pick(uint64_t n) { return key_dedup_pick(n) ? 1 : 0; }
uint64_t ht_dedup_n0() { return DEDUP_N0; }
// rep, slot_of, list, rank: n each; returns U, or -1 for arguments the table does not take
int64_t ht_dedup_run(int kb, const uint8_t* keys, uint32_t n, int slack_log, uint32_t max_probes, uint32_t* slot_of, uint32_t* rep, uint32_t* list, uint32_t* rank) {
  if ((kb != 48 && kb != 96) || n == 0 || n > 0x7fffffffu || slack_log < 0 || slack_log > DEDUP_SLACK_MAX || max_probes < 1 || max_probes > (uint32_t)DEDUP_PROBES_MAX) return -1;
  const uint64_t S = dedup_slots(n, slack_log);
  std::vector<uint32_t> owner(S), first(S);
  return kb == 96 ? dedup_host<96>(keys, n, slack_log, max_probes, owner.data(), first.data(), slot_of, rep, list, rank)
                  : dedup_host<48>(keys, n, slack_log, max_probes, owner.data(), first.data(), slot_of, rep, list, rank);
}
}
