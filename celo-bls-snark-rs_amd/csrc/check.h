// Validation of affine rows in arkworks Montgomery limbs (what every MSM, pairing and key entry point takes and trusts): is the row a
// canonical point of the curve, and does it lie in the prime-order subgroup.  The membership test a caller of Seam B has for points it
// holds as limb rows rather than as wire bytes (check_points_*, include/celo_bls_amd.h); what ark-ec calls is_on_curve and
// is_in_correct_subgroup_assuming_on_curve.  Host and device templates, one row per call: k_check_rows (unit_check.hip) runs them one row
// per lane, tests/test_subgroup_host.py runs them on the host under bounds tracking.
//
// Group CG: 0 / 1 = BLS12-377 G1 (y^2 = x^3 + 1, 12 u64 per row) / G2 (y^2 = x^3 + 1/u over Fq2, 24 u64: c0 then c1 per coordinate),
//           2 / 3 = BW6-761 G1 (y^2 = x^3 - 1) / G2 (y^2 = x^3 + 4), 24 u64 per row.
// Status, the first that applies (wire.h WireStatus, the decoders' codes):
//   the row's flag is set                              -> WIRE_INFINITY (1); the coordinates are not looked at
//   a coordinate (an Fq2 component) is not below q     -> WIRE_INVALID (2)
//   (x, y) does not satisfy the curve equation         -> WIRE_INVALID (2)
//   level 2: r P != O                                  -> WIRE_NOT_IN_SUBGROUP (3)
//   otherwise                                          -> WIRE_OK (0)
// The subgroup tests are the decoders': wire_in_subgroup (wire.h) for BLS12-377, w761_in_subgroup_endo (wire761.h) for BW6-761.
#pragma once
#include <cstdint>
#include "wire.h"
#include "wire761.h"

namespace celo {

constexpr int check_row_words(int cg) { return cg == 0 ? 12 : 24; }

// BLS12-377: the row up to the curve equation; p is set when WIRE_OK
HD WireStatus check_curve_377_g1(const uint64_t* row, Affine<Fq>& p) {
  if (wire_cmp(row, P377::P64, 6) >= 0 || wire_cmp(row + 6, P377::P64, 6) >= 0) return WIRE_INVALID;
  const Fq x = Fq::norm(Fq::from_ark(row)), y = Fq::norm(Fq::from_ark(row + 6));
  if (!wire_eq(Fq::sqr(y), Fq::norm(Fq::add(Fq::mul(Fq::sqr(x), x), Fq::one())))) return WIRE_INVALID;
  p = {x, y};
  return WIRE_OK;
}
HD WireStatus check_curve_377_g2(const uint64_t* row, const WireConsts& k, Affine<Fq2>& p) {
  for (int c = 0; c < 4; c++) {
    if (wire_cmp(row + 6 * c, P377::P64, 6) >= 0) return WIRE_INVALID;
  }
  const Fq2 x = Fq2::norm({Fq::from_ark(row), Fq::from_ark(row + 6)}), y = Fq2::norm({Fq::from_ark(row + 12), Fq::from_ark(row + 18)});
  const Fq2 tb = {Fq::zero(), wire_neg(k.inv5)};                      // B' = 1/u = -u/5, as in wire_decode_g2
  const Fq2 rhs = Fq2::norm(Fq2::add(Fq2::mul(Fq2::sqr(x), x), tb)), yy = Fq2::sqr(y);
  if (!wire_eq(yy.c0, rhs.c0) || !wire_eq(yy.c1, rhs.c1)) return WIRE_INVALID;
  p = {x, y};
  return WIRE_OK;
}
// BW6-761, b = B: the same
template <int B> HD WireStatus check_curve_761(const uint64_t* row, Affine<Fw761>& p) {
  if (wire_cmp(row, P761::P64, 12) >= 0 || wire_cmp(row + 12, P761::P64, 12) >= 0) return WIRE_INVALID;
  const Fw761 x = Fw761::norm(Fw761::from_ark(row)), y = Fw761::norm(Fw761::from_ark(row + 12));
  if (!w761_eq(Fw761::sqr(y), w761_rhs<B>(x))) return WIRE_INVALID;
  p = {x, y};
  return WIRE_OK;
}

// one row of group CG at level 1 (the curve equation) or 2 (and the subgroup).  ladder761: BW6-761 runs the r P ladder in place of the
// endomorphism form (the twin; the verdicts are the same)
template <int CG> HD WireStatus check_row(const uint64_t* row, bool flagged, int level, const WireConsts& k, bool ladder761 = false) {
  static_assert(CG >= 0 && CG <= 3, "0 / 1: BLS12-377 G1 / G2, 2 / 3: BW6-761 G1 / G2");
  if (flagged) return WIRE_INFINITY;
  if constexpr (CG == 0) {
    Affine<Fq> p = {Fq::zero(), Fq::zero()};
    const WireStatus st = check_curve_377_g1(row, p);
    if (st != WIRE_OK || level < 2) return st;
    return wire_in_subgroup(p, k) ? WIRE_OK : WIRE_NOT_IN_SUBGROUP;
  } else if constexpr (CG == 1) {
    Affine<Fq2> p = {Fq2::zero(), Fq2::zero()};
    const WireStatus st = check_curve_377_g2(row, k, p);
    if (st != WIRE_OK || level < 2) return st;
    return wire_in_subgroup(p, k) ? WIRE_OK : WIRE_NOT_IN_SUBGROUP;
  } else {
    constexpr int B = CG == 2 ? -1 : 4;
    Affine<Fw761> p = {Fw761::zero(), Fw761::zero()};
    const WireStatus st = check_curve_761<B>(row, p);
    if (st != WIRE_OK || level < 2) return st;
    return (ladder761 ? w761_in_subgroup(p) : w761_in_subgroup_endo<B>(p)) ? WIRE_OK : WIRE_NOT_IN_SUBGROUP;
  }
}

}  // namespace celo
