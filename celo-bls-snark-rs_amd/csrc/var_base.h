// Batched variable-base scalar multiplication out[i] = [k_i] P_i: many points, each with its own scalar (PrivateKey::sign = hash * sk,
// crates/bls-crypto/src/bls/secret.rs:65, and the sign_batch / keygen_mul helpers of crates/bls-crypto/src/test_helpers.rs:20,54).
//
// One lane per row.  The lane first builds the table of its own point,
//   T[e] = [e + 1] P_i      e = 0 .. H - 1,  H = 2^(c-1)      (affine, canonical, an identity flag each)
// by a chain of mixed additions and ONE inversion (Montgomery's trick along the chain), then walks the signed c-bit digits of k_i
// (fb_digit of fixed_base.h: d_j in (-H, H]) from the top window down: c doublings, then one mixed addition per nonzero digit.
// P_i is any point of the curve: the chain and the ladder go through xyzz_madd / xyzz_dbl of curve.h, whose doubling, cancelling and
// identity branches are all live here ([2]P is a madd with acc == P; a point of order 2 or 3 fills the table with identities).
//
// The table lives in a per-call workspace, lane-interleaved in 16-byte words: word q of entry e of lane l is at
//   table[(e * (2 FW / 4) + q) * stride + l]      (uint4 units; stride = lanes of the chunk)
// so adjacent lanes read adjacent words whenever they look up the same entry.  The chain's XYZZ points use the same layout.
//
// The subgroup path (BLS12-377 G1): k = k0 + k1 x^2 (glv_split_x2 of gls.h), [k]P = [k0]P + [k1] I(P) with I(x, y) = (beta x, -y) = [x^2](x, y)
// on the prime-order subgroup.  I commutes with the group law, so I(T[e]) = [e + 1] I(P): one table serves both halves, the image costs one
// product as the entry is loaded, and the two 127-bit halves share their doublings.
// Every routine here is HD: the kernels of unit_varbase.hip and the host twins of host_test.cpp (-DCELO_FP_TRACK) run the same code.
#pragma once
#include "fixed_base.h"
#include "gls.h"

namespace celo {

constexpr int VB_MIN_C = 2, VB_MAX_C = 8;     // window bits the ladder accepts: tables of 2 .. 128 entries per lane
constexpr int VB_GLV_BITS = 127;              // both halves of the split are below 2^127

// ---- the carries of fb_digit's recoding.  fb_digit recodes from the bottom window up, the ladder walks from the top down: bit j here is
// the carry INTO window j, found in one pass of integer work before the ladder starts.  W <= 190 (377 bits at c = 2).
struct VbCarries { uint64_t m0, m1, m2; };
template <int N64> HD VbCarries vb_carries(const uint64_t* s, int c, int W) {
  VbCarries r = {0, 0, 0};
  uint32_t carry = 0;
  for (int j = 0; j < W; j++) {
    const uint64_t bit = (uint64_t)carry << (j & 63);
    if (j < 64) r.m0 |= bit;
    else if (j < 128) r.m1 |= bit;
    else r.m2 |= bit;
    (void)fb_digit<N64>(s, j, c, carry);
  }
  return r;
}
HD uint32_t vb_carry_in(const VbCarries& k, int j) {
  const uint64_t w = j < 64 ? k.m0 : j < 128 ? k.m1 : k.m2;
  return (uint32_t)(w >> (j & 63)) & 1u;
}
// digit j of s, top-down: the same value fb_digit gives in its bottom-up pass
template <int N64> HD int32_t vb_digit(const uint64_t* s, const VbCarries& k, int j, int c) {
  uint32_t carry = vb_carry_in(k, j);
  return fb_digit<N64>(s, j, c, carry);
}

// ---- the lane-interleaved workspace: NW words (a multiple of 4) of slot e of one lane, through a local buffer so that the field's own
// load / store (and fb_store_entry's canonical form) stay the only definition of the word layout
template <int NW> HD void vb_put(uint4* base, size_t stride, uint32_t lane, uint32_t e, const uint32_t* buf) {
  const uint4* b = reinterpret_cast<const uint4*>(buf);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int q = 0; q < NW / 4; q++) base[((size_t)e * (NW / 4) + q) * stride + lane] = b[q];
}
template <int NW> HD void vb_get(const uint4* base, size_t stride, uint32_t lane, uint32_t e, uint32_t* buf) {
  uint4* b = reinterpret_cast<uint4*>(buf);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int q = 0; q < NW / 4; q++) b[q] = base[((size_t)e * (NW / 4) + q) * stride + lane];
}
template <class F> HD void vb_store_entry(uint4* table, size_t stride, uint32_t lane, uint32_t e, const Affine<F>& a) {
  alignas(16) uint32_t buf[2 * F::WORDS];
  fb_store_entry(buf, a);
  vb_put<2 * F::WORDS>(table, stride, lane, e, buf);
}
template <class F> HD Affine<F> vb_load_entry(const uint4* table, size_t stride, uint32_t lane, uint32_t e) {
  alignas(16) uint32_t buf[2 * F::WORDS];
  vb_get<2 * F::WORDS>(table, stride, lane, e, buf);
  return fb_load_entry<F>(buf);
}
template <class F> HD void vb_store_xyzz(uint4* chain, size_t stride, uint32_t lane, uint32_t e, const Xyzz<F>& a) {
  constexpr int FW = F::WORDS;
  alignas(16) uint32_t buf[4 * FW];
  a.X.store(buf); a.Y.store(buf + FW); a.ZZ.store(buf + 2 * FW); a.ZZZ.store(buf + 3 * FW);
  vb_put<4 * FW>(chain, stride, lane, e, buf);
}
template <class F> HD Xyzz<F> vb_load_xyzz(const uint4* chain, size_t stride, uint32_t lane, uint32_t e) {
  constexpr int FW = F::WORDS;
  alignas(16) uint32_t buf[4 * FW];
  vb_get<4 * FW>(chain, stride, lane, e, buf);
  return {F::load(buf), F::load(buf + FW), F::load(buf + 2 * FW), F::load(buf + 3 * FW)};
}

// ---- the table of one point, three passes over the lane's workspace (memory is the spill space: a pass keeps no more than the accumulator
// and one operand in registers).  Pass 1 writes P itself, canonical, as entry 0 and chains T[e] = T[e-1] + P in XYZZ (chain: H slots of 4 FW
// words), reading P back from entry 0.  Pass 2 leaves the running product of the denominators ZZ ZZZ BEFORE entry e in the x half of table
// slot e.  Pass 3 inverts the whole product once and walks back, as k_normalize does inside a lane.  An identity entry (P the identity, or
// e + 1 a multiple of P's order) takes no part in the product: flag 1, zero words.
template <class F> HD void vb_build_table(const Affine<F>& p, bool p_inf, uint32_t H, uint4* chain, uint4* table, uint8_t* tinf, size_t stride, uint32_t lane) {
  {
    Xyzz<F> acc = p_inf ? Xyzz<F>::identity() : Xyzz<F>::from_affine(p);
    vb_store_entry<F>(table, stride, lane, 0, p_inf ? Affine<F>{F::zero(), F::zero()} : p);
    tinf[lane] = p_inf ? 1 : 0;
    for (uint32_t e = 1; e < H; e++) {
      if (!p_inf) xyzz_madd(acc, vb_load_entry<F>(table, stride, lane, 0));
      vb_store_xyzz<F>(chain, stride, lane, e, acc);
    }
  }
  F run = F::one();
  for (uint32_t e = 1; e < H; e++) {
    const Xyzz<F> a = vb_load_xyzz<F>(chain, stride, lane, e);
    vb_store_entry<F>(table, stride, lane, e, Affine<F>{run, F::zero()});
    bool id = a.is_identity();
    if (!id) {
      const F den = F::norm(F::mul(a.ZZ, a.ZZZ));
      id = den.is_zero_mod_p();
      if (!id) run = F::norm(F::mul(run, den));
    }
    tinf[(size_t)e * stride + lane] = id ? 1 : 0;
  }
  F iv = F::norm(F::inv(run));
  for (uint32_t e = H; e-- > 1;) {
    if (tinf[(size_t)e * stride + lane]) {
      vb_store_entry<F>(table, stride, lane, e, Affine<F>{F::zero(), F::zero()});
      continue;
    }
    const Xyzz<F> a = vb_load_xyzz<F>(chain, stride, lane, e);
    const F pre = vb_load_entry<F>(table, stride, lane, e).x;
    const F di = F::norm(F::mul(iv, pre));
    iv = F::norm(F::mul(iv, F::norm(F::mul(a.ZZ, a.ZZZ))));
    const Affine<F> r = {F::norm(F::mul(a.X, F::norm(F::mul(di, a.ZZZ)))), F::norm(F::mul(a.Y, F::norm(F::mul(di, a.ZZ))))};
    vb_store_entry<F>(table, stride, lane, e, r);
  }
}

// acc += sign(d) T[|d| - 1], or its image under I when IMG (BLS12-377 G1 only: (beta x, -y))
template <class F, bool GLV> HD void vb_add_digit(Xyzz<F>& acc, int32_t d, bool img, const uint4* table, const uint8_t* tinf, size_t stride, uint32_t lane) {
  if (d == 0) return;
  const uint32_t e = (uint32_t)(d < 0 ? -d : d) - 1u;
  if (tinf[(size_t)e * stride + lane]) return;
  Affine<F> p = vb_load_entry<F>(table, stride, lane, e);
  bool neg = d < 0;
  if constexpr (GLV) {
    if (img) {
      p.x = F::norm(F::mul(p.x, F::from_limbs(T377::BETA_GLV)));
      neg = !neg;
    }
  }
  if (neg) p = affine_neg(p);
  xyzz_madd(acc, p);
}

// ---- the plain ladder: [k] P from P's table, k canonical in N64 limbs below 2^bits
template <class F, int N64> HD Xyzz<F> vb_ladder(const uint64_t* s, int bits, int c, const uint4* table, const uint8_t* tinf, size_t stride, uint32_t lane) {
  const int W = fb_windows(bits, c);
  const VbCarries cy = vb_carries<N64>(s, c, W);
  Xyzz<F> acc = Xyzz<F>::identity();
  for (int j = W - 1; j >= 0; j--) {
    for (int k = 0; k < c; k++) xyzz_dbl_fn(acc);
    vb_add_digit<F, false>(acc, vb_digit<N64>(s, cy, j, c), false, table, tinf, stride, lane);
  }
  return acc;
}

// ---- the subgroup ladder of BLS12-377 G1: k (4 limbs, below r) = k0 + k1 x^2, the halves' digits added window by window between shared
// doublings; the k1 half reads the same table through the image
template <class F> HD Xyzz<F> vb_ladder_glv(const uint64_t* s, int c, const uint4* table, const uint8_t* tinf, size_t stride, uint32_t lane) {
  uint32_t k[8], k0[4], k1[4];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < 4; i++) { k[2 * i] = (uint32_t)s[i]; k[2 * i + 1] = (uint32_t)(s[i] >> 32); }
  glv_split_x2<8>(k, k0, k1);
  const uint64_t h0[2] = {(uint64_t)k0[0] | ((uint64_t)k0[1] << 32), (uint64_t)k0[2] | ((uint64_t)k0[3] << 32)};
  const uint64_t h1[2] = {(uint64_t)k1[0] | ((uint64_t)k1[1] << 32), (uint64_t)k1[2] | ((uint64_t)k1[3] << 32)};
  const int W = fb_windows(VB_GLV_BITS, c);
  const VbCarries c0 = vb_carries<2>(h0, c, W), c1 = vb_carries<2>(h1, c, W);
  Xyzz<F> acc = Xyzz<F>::identity();
  for (int j = W - 1; j >= 0; j--) {
    for (int q = 0; q < c; q++) xyzz_dbl_fn(acc);
    // one addition site for both halves (the half is picked by value, not by index: the limbs stay registers)
    for (int half = 0; half < 2; half++) {
      const uint64_t hs[2] = {half ? h1[0] : h0[0], half ? h1[1] : h0[1]};
      const VbCarries cy = {half ? c1.m0 : c0.m0, half ? c1.m1 : c0.m1, half ? c1.m2 : c0.m2};
      vb_add_digit<F, true>(acc, vb_digit<2>(hs, cy, j, c), half != 0, table, tinf, stride, lane);
    }
  }
  return acc;
}

}  // namespace celo
