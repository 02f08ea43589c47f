// Batch normalisation to affine (ProjectiveCurve::batch_normalization_into_affine, called at crates/bls-crypto/src/bls/signature.rs:82 and
// public.rs:58 before every MSM): Montgomery's trick inside a lane over K consecutive rows - one field inversion per K rows, 3 products per
// row for the prefix / suffix products, then the affine coordinates.  The one kernel every normalisation runs (unit_wire.hip wire_normalize,
// unit_setup.hip's fixed-base rows); the row source is a template parameter:
//   JAC = true   Jacobian rows in arkworks Montgomery limbs (identity = Z == 0):  x = X / Z^2, y = Y / Z^3.  Rows that are already affine
//                (Z == 1: everything that came off the wire) take part with z = 1; their x, y come out unchanged.
//   JAC = false  XYZZ rows in device form (4 FW words), the denominator ZZ ZZZ:  x = X ZZZ / (ZZ ZZZ), y = Y ZZ / (ZZ ZZZ).
// out: n x (x, y) in arkworks limbs; the identity row is written as zeros, or as arkworks' GroupAffine::zero() coordinates (0, 1) with
// ZERO_Y and ark_zero_y; inf[i] = 1 either way.
// WAVES: the amdgpu_waves_per_eu bound (0: none).  WAVES and ZERO_Y keep each instance the code it had before the units shared this kernel:
// the BLS12-377 Jacobian instances (unit_wire.hip) run at two waves per SIMD and never write (0, 1), the others have no bound and read the
// flag.  The body is the kernel's own: moved into a __forceinline__ function behind thin kernels, the same source compiles to other
// register counts.
#pragma once
#include <cstdint>
#include <type_traits>
#include "fp.h"

namespace celo {

// f(integral_constant<j>) for j = 0 .. N-1 (or N-1 .. 0)
template <int N, bool REVERSE, class Fn> __device__ __forceinline__ void static_for(Fn&& f) {
  if constexpr (N > 0) {
    if constexpr (REVERSE) { f(std::integral_constant<int, N - 1>{}); static_for<N - 1, true>(f); }
    else { static_for<N - 1, false>(f); f(std::integral_constant<int, N - 1>{}); }
  }
}

// Lane t normalises rows t K .. t K + K - 1.  Only the prefix products stay in registers (K x 14 / 28 words); a row's denominator is read
// again on the way back instead of being kept: with both arrays alive the BLS12-377 G1 instance (K = 8) held 224 words of state, the loops
// were not unrolled and the arrays went to private memory through run-time indices (912 B/lane).  The loops are unrolled by template
// recursion: `#pragma unroll` over bodies of this size is refused by the optimizer, and a rolled loop indexes pre[] at run time.
template <class F, int K, bool JAC, int WAVES, bool ZERO_Y>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES)))
k_normalize(const void* __restrict__ in_, uint64_t* __restrict__ out, uint8_t* __restrict__ inf, uint32_t n, int ark_zero_y) {
  constexpr int A = F::ARK64, FW = F::WORDS;
  const uint32_t lo = (blockIdx.x * blockDim.x + threadIdx.x) * K;
  if (lo >= n) return;
  const uint32_t cnt = n - lo < (uint32_t)K ? n - lo : (uint32_t)K;
  const uint64_t* jac = (const uint64_t*)in_;
  const uint32_t* xyzz = (const uint32_t*)in_;
  auto den = [&](int j) -> F {
    if constexpr (JAC) return F::norm(F::from_ark(jac + ((size_t)lo + j) * 3 * A + 2 * A));
    else {
      const uint32_t* p = xyzz + ((size_t)lo + j) * 4 * FW;
      const F zz = F::load(p + 2 * FW);
      if (zz.limbs_all_zero()) return F::zero();
      return F::norm(F::mul(zz, F::load(p + 3 * FW)));
    }
  };
  F pre[K];
  uint32_t idmask = 0;
  F acc = F::one();
  static_for<K, false>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    pre[j] = acc;
    if ((uint32_t)j < cnt) {
      const F dj = den(j);
      if (dj.is_zero_mod_p()) idmask |= 1u << j;
      else acc = F::norm(F::mul(acc, dj));
    }
  });
  F iv = F::norm(F::inv(acc));
  static_for<K, true>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    if ((uint32_t)j < cnt) {
      uint64_t* o = out + ((size_t)lo + j) * 2 * A;
      const bool id = (idmask >> j) & 1u;
      inf[lo + j] = id ? 1 : 0;
      if (id) {
        for (int q = 0; q < 2 * A; q++) o[q] = 0;
        if (ZERO_Y && ark_zero_y) F::one().to_ark(o + A);
      } else {
        const F di = F::norm(F::mul(iv, pre[j]));
        iv = F::norm(F::mul(iv, den(j)));
        if constexpr (JAC) {
          const uint64_t* src = jac + ((size_t)lo + j) * 3 * A;
          const F di2 = F::norm(F::sqr(di));
          F::mul(F::from_ark(src), di2).to_ark(o);
          F::mul(F::from_ark(src + A), F::norm(F::mul(di2, di))).to_ark(o + A);
        } else {
          const uint32_t* p = xyzz + ((size_t)lo + j) * 4 * FW;
          F::mul(F::load(p), F::norm(F::mul(di, F::load(p + 3 * FW)))).to_ark(o);
          F::mul(F::load(p + FW), F::norm(F::mul(di, F::load(p + 2 * FW)))).to_ark(o + A);
        }
      }
    }
  });
}

// The XYZZ form's launch: n device rows of 4 F::WORDS words -> n affine rows and flags, enqueued on s.  K rows per lane by the field's size
// (8 for the 14-limb field, 4 for the wider ones).  ZERO_Y: the instance that can write the identity as (0, 1), when ark_zero_y asks for it.
template <class F, bool ZERO_Y>
void normalize_xyzz(const uint32_t* d_xyzz, uint64_t* d_out, uint8_t* d_inf, uint32_t n, int ark_zero_y, hipStream_t s) {
  constexpr int K = sizeof(F) <= 64 ? 8 : 4;
  hipLaunchKernelGGL((k_normalize<F, K, false, 0, ZERO_Y>), dim3(((n + K - 1) / K + 63) / 64), dim3(64), 0, s, (const void*)d_xyzz, d_out, d_inf, n, ark_zero_y);
}

}  // namespace celo
