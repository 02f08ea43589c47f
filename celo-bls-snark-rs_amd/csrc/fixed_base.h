// Batched fixed-base scalar multiplication out[i] = k_i G (ark-ec FixedBaseMSM::multi_scalar_mul, the work of ark-groth16 0.1
// generate_parameters underneath crates/epoch-snark/src/api/setup.rs:22-46,63-105) and the Groth16 setup's scalar preparation.
//
// One generator, n scalars, n points.  The generator's table holds, for window w = 0 .. W-1 and digit d = 1 .. 2^(c-1),
//   T[w][d - 1] = d 2^(c w) G      (affine, device form)
// and a scalar's signed c-bit digits d_w in (-2^(c-1), 2^(c-1)] (W = ceil((BITS + 1) / c): the carry out of the top digit is always 0)
// select one entry per window:  k G = sum_w sign(d_w) T[w][|d_w| - 1]  - one mixed addition per nonzero digit, no doublings.
// Every routine here is HD: the kernels of unit_setup.hip and the host twins of host_test.cpp (-DCELO_FP_TRACK) run the same code.
#pragma once
#include "curve.h"
#include "fp2.h"
#if defined(__HIPCC__)
#include "runtime.h"
#endif

namespace celo {

// windows of c bits for scalars of BITS bits, signed digits
HD constexpr int fb_windows(int bits, int c) { return (bits + 1 + c - 1) / c; }

// the signed c-bit digit of window j of a canonical scalar s (N64 little-endian u64 limbs), carry in / out.  The limbs are selected by
// comparison, not by index: a run-time index into a register array is a private-memory access on the device.
template <int N64> HD int32_t fb_digit(const uint64_t* s, int j, int c, uint32_t& carry) {
  const int bit = j * c, wi = bit >> 6, off = bit & 63;
  uint64_t w0 = 0, w1 = 0;
#pragma unroll
  for (int k = 0; k < N64; k++) {
    if (k == wi) w0 = s[k];
    if (k == wi + 1) w1 = s[k];
  }
  uint64_t v = w0 >> off;
  if (off + c > 64) v |= w1 << (64 - off);
  const uint32_t raw = (uint32_t)v & ((1u << c) - 1u);
  const uint32_t d = raw + carry;
  if (d > (1u << (c - 1))) { carry = 1; return (int32_t)d - (int32_t)(1u << c); }
  carry = 0;
  return (int32_t)d;
}

// s < modulus (both N64 limbs)
template <int N64> HD bool fb_below(const uint64_t* s, const uint64_t* m) {
  for (int k = N64 - 1; k >= 0; k--) {
    if (s[k] != m[k]) return s[k] < m[k];
  }
  return false;
}

#if defined(__HIPCC__)
// N u64 handed to a kernel by value (a group order, a generator's limbs)
template <int N> struct ArkWords { uint64_t v[N]; };
// flag |= 1 for a scalar >= the group order
template <int N64>
__global__ void __launch_bounds__(256) k_scalars_below(const uint64_t* __restrict__ sc, uint32_t n, ArkWords<N64> r, uint32_t* flag) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t s[N64];
#pragma unroll
  for (int k = 0; k < N64; k++) s[k] = sc[(size_t)i * N64 + k];
  if (!fb_below<N64>(s, r.v)) atomicOr(flag, 1u);
}
// The range check of the device-pointer entries: n scalars on the device (N64 u64 each) against `order`, on cs's stream, which it
// synchronises.  0: all below; 2: one is not; else 10 (a HIP call failed).
template <int N64> int scalars_below_order(const uint64_t* d_sc, size_t n, const uint64_t* order, CallScope& cs) {
  ArkWords<N64> r;
  for (int k = 0; k < N64; k++) r.v[k] = order[k];
  uint32_t flag = 0;
  uint32_t* d_flag;
  HIP_TRY(cs.alloc(&d_flag, 4), 10);
  HIP_TRY(hipMemsetAsync(d_flag, 0, 4, cs.stream()), 10);
  hipLaunchKernelGGL((k_scalars_below<N64>), dim3(((uint32_t)n + 255) / 256), dim3(256), 0, cs.stream(), d_sc, (uint32_t)n, r, d_flag);
  HIP_TRY(hipGetLastError(), 10);
  HIP_TRY(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, cs.stream()), 10);
  HIP_TRY(hipStreamSynchronize(cs.stream()), 10);
  return flag ? 2 : 0;
}
#endif

// XYZZ -> affine with one inversion (x = X / ZZ, y = Y / ZZZ); false for the identity
template <class F> HD bool fb_to_affine(const Xyzz<F>& a, Affine<F>& out) {
  if (a.is_identity() || a.ZZ.is_zero_mod_p()) return false;
  const F t = F::inv(F::mul(a.ZZ, a.ZZZ));
  out = {F::norm(F::mul(a.X, F::mul(t, a.ZZZ))), F::norm(F::mul(a.Y, F::mul(t, a.ZZ)))};
  return true;
}

// Table entries are stored canonical (each coordinate below p) and loaded with that bound: F::load alone declares the loosest bound of
// the contract (vb 64), under which the negation of a negative digit's entry (sub<4, 1>) would not be admitted by the bounds tracker.
template <class P> HD Fp<P> fb_canon(const Fp<P>& a) { return Fp<P>::reduce(a); }
template <class P> HD Fp2<P> fb_canon(const Fp2<P>& a) { return {Fp<P>::reduce(a.c0), Fp<P>::reduce(a.c1)}; }
template <class P> HD Fp<P> fb_load_canon(const Fp<P>*, const uint32_t* p) { Fp<P> r = Fp<P>::load(p); TRK(r.vb = 1;) return r; }
template <class P> HD Fp2<P> fb_load_canon(const Fp2<P>*, const uint32_t* p) {
  Fp2<P> r = Fp2<P>::load(p);
  TRK(r.c0.vb = 1; r.c1.vb = 1;)
  return r;
}
template <class F> HD void fb_store_entry(uint32_t* p, const Affine<F>& a) { fb_canon(a.x).store(p); fb_canon(a.y).store(p + F::WORDS); }
template <class F> HD Affine<F> fb_load_entry(const uint32_t* p) {
  return {fb_load_canon((const F*)nullptr, p), fb_load_canon((const F*)nullptr, p + F::WORDS)};
}

// ---- table build, two steps.  Step 1 (one lane per window): 2^(c w) G by c w doublings.  Step 2 (one lane per entry): d times that base
// by the short double-and-add of curve.h (d <= 2^(c-1)), then the affine form.
template <class F> HD Xyzz<F> fb_window_base(const Affine<F>& g, int w, int c) {
  Xyzz<F> a = Xyzz<F>::from_affine(g);
  for (int k = 0; k < w * c; k++) xyzz_dbl_fn(a);
  return a;
}
template <class F> HD Xyzz<F> fb_table_entry(const Affine<F>& base, uint32_t d) {
  return xyzz_mul_small(Xyzz<F>::from_affine(base), d);
}

// ---- one scalar: recoding, table lookup and accumulation.  table: W 2^(c-1) affine entries of 2 F::WORDS words, window-major; tinf: the
// entries that are the identity (only a generator outside the prime-order group can produce one).  A scalar of zero returns the identity.
template <class F, int N64> HD Xyzz<F> fb_scalar_mul(const uint64_t* s, const uint32_t* table, const uint8_t* tinf, int c, int W) {
  constexpr int FW = F::WORDS;
  const uint32_t H = 1u << (c - 1);
  Xyzz<F> acc = Xyzz<F>::identity();
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
  return acc;
}

// ---- the Groth16 setup's scalars (ark-groth16 0.1 generate_parameters after the QAP evaluation at tau), arkworks Montgomery limbs in,
// canonical integers out (what fb_scalar_mul takes).  FR: the scalar field (Fp<P377> for BW6-761, Fp<P253> for BLS12-377).
//   (beta a_i + alpha b_i + c_i) inv     inv = gamma^-1 (gamma_abc, i < n_inputs) or delta^-1 (l_query)
template <class FR> HD void setup_lc(const uint64_t* a, const uint64_t* b, const uint64_t* c, const FR& alpha, const FR& beta, const FR& inv,
                                     uint64_t* out) {
  const FR x = FR::from_ark(a), y = FR::from_ark(b), z = FR::from_ark(c);
  const FR s = FR::norm(FR::add(FR::add(FR::mul(beta, x), FR::mul(alpha, y)), FR::norm(z)));
  FR::mul(s, inv).to_canonical(out);
}
// ark Montgomery -> canonical
template <class FR> HD void setup_canon(const uint64_t* a, uint64_t* out) { FR::from_ark(a).to_canonical(out); }
// rows of h per lane of the setup's power kernel (each block starts at tau^(block start))
constexpr uint32_t SETUP_H_BLOCK = 32;
// h_i = zt delta^-1 tau^i for i = i0 .. i0 + cnt - 1: one power tau^i0 (square-and-multiply on the 64-bit index), then one product per row
template <class FR> HD void setup_h_block(const FR& zt_dinv, const FR& tau, uint64_t i0, uint32_t cnt, uint64_t* out) {
  FR cur = FR::norm(FR::mul(zt_dinv, FR::pow64(FR::norm(tau), &i0, 1)));
  for (uint32_t k = 0; k < cnt; k++) {
    cur.to_canonical(out + (size_t)k * FR::ARK64);
    cur = FR::norm(FR::mul(cur, tau));
  }
}

}  // namespace celo
