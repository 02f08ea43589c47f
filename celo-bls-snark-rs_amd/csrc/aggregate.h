// Masked, segmented point sums: out_i = sum { P_j : bits_i[j] != 0 } for many bitmaps at once - the aggregated public key of a seal
// (PublicKeyCache::aggregate, crates/bls-crypto/src/bls/cache.rs:65-87; BlsGadget::enforce_bitmap's native twin,
// crates/epoch-snark/src/gadgets/single_update.rs:71-117) and Signature::aggregate over a bitmap.
//
// Two forms.  Per-seal sets: seal i owns rows [offsets[i], offsets[i+1]) and the bytes of `bits` at the same indices.  Shared set: every
// seal reads rows [offsets[0], offsets[1]), n of them, and its own n bytes bits[i n ..].  A row flagged as the identity adds nothing.
//
// The complement (shared set only): with T the sum of the whole set, sum of the ones = T + sum of the NEGATED keys at the zero bytes.  A seal
// takes that side when it has strictly fewer zeros than ones (a tie sums the ones) - the reference's cache trick: with 2/3 signing it is
// 3 x fewer additions.  The group element, and so the normalised row, is the same either way.
//
// One sum is the work of L lanes, L a power of two from 1 to 64 (AGG_MAX_LANES):
//   phase 1   lane l walks the rows j = l, l + L, l + 2 L, ... of its seal and adds the selected ones with xyzz_madd (mixed additions);
//   phase 2   the L partials are folded pairwise through a buffer (LDS on the device): in the round of stride s = L/2, L/4, .. 1 lane
//             l < s adds the partial stored in slot l + s to its own with a full addition (xyzz_add_mem, which reads the partner where it
//             is used: two Fq2 XYZZ points and the addition's temporaries do not fit the register file) and stores the result in slot l;
//   lane 0 then adds T when the seal took the complement.
// Every branch of both formulas is live in both phases: duplicate keys meet in the doubling branch, a key and its negative in the
// cancelling branch, and a lane without selected rows carries the identity into the fold.
//
// The lane width of a call (agg_pick_lanes): a = the largest number of rows any seal adds after the side choice, m the number of seals.
//   L = min( smallest power of two >= a / AGG_ROWS_PER_LANE,  largest power of two <= AGG_FILL_LANES / m ),  at least 1, at most 64
// A lane should have AGG_ROWS_PER_LANE mixed additions before the fold's log2 L full additions are worth paying, and past AGG_FILL_LANES
// lanes in flight (2^16: one wave on every SIMD of the device, which is all the G2 kernel's 256 registers admit) more lanes per sum only
// add fold work to a device that is already full.  The constants come from a same-run A/B over all seven widths (tools/bench_seals.py,
// profiles/bench_seals.json; G2, kernel ms, best width / the rule's): 17 280 seals x 110 shared, complement 1.72 at L = 2 /
// 2; the same without the complement 2.16 at 8 / 2.33 at 2; 4 096 sets of 256: 1.31 at 16 / 16; 64 seals x 110: 1.06 - 1.08 from 16 to 64 /
// 16, without the complement 0.69 at 64 / 0.73 at 32.
// Every routine is HD: the kernels of unit_seals.hip and the host twins of host_test.cpp (-DCELO_FP_TRACK) run the same code.
#pragma once
#include "curve.h"
#include "fp2.h"

namespace celo {

constexpr uint32_t AGG_MAX_LANES = 64;
constexpr uint32_t AGG_MAX_SEALS = 1u << 24;
constexpr uint32_t AGG_ROWS_PER_LANE = 4;
constexpr uint32_t AGG_FILL_LANES = 1u << 16;
// words between two partials in the fold buffer: a point and one 16-byte pad, which keeps vector accesses aligned and takes the stride
// off the power of two
template <class F> constexpr uint32_t agg_slot_words() { return 4 * F::WORDS + 4; }

HD bool agg_lanes_ok(int L) { return L >= 1 && L <= (int)AGG_MAX_LANES && (L & (L - 1)) == 0; }
inline uint32_t agg_pick_lanes(uint32_t max_adds, size_t m) {
  uint32_t work = 1, fill = AGG_MAX_LANES;
  while (work < AGG_MAX_LANES && (uint64_t)work * AGG_ROWS_PER_LANE < max_adds) work <<= 1;
  while (fill > 1 && (uint64_t)fill * m > AGG_FILL_LANES) fill >>= 1;
  return work < fill ? work : fill;
}

// the number of set bytes of one bitmap
HD uint32_t agg_count(const uint8_t* bits, uint32_t n) {
  uint32_t c = 0;
  for (uint32_t j = 0; j < n; j++) c += bits[j] != 0 ? 1u : 0u;
  return c;
}
// the side of one seal: true = sum the negated keys at the zero bytes and add the set's total.  mode: -1 the rule, 0 never, 1 always
HD bool agg_side(uint32_t count, uint32_t n, int mode, bool shared_set) {
  if (!shared_set || mode == 0) return false;
  if (mode == 1) return true;
  return n - count < count;
}

// A stored partial keeps the bounds of curve.h's Xyzz contract (vb(X) <= 19, vb(Y) <= 7, vb(ZZ), vb(ZZZ) <= 3): checked where it is stored
// and declared where a whole point is loaded (F::load alone declares the loosest bound, vb 64, under which the doubling of a loaded point
// is not admitted by the bounds tracker).
template <class P> HD void agg_bound(Fp<P>& a, double vb, bool check) { TRK(if (check) assert(a.lb <= 1 && a.vb <= vb); else a.vb = vb;) (void)a; (void)vb; (void)check; }
template <class P> HD void agg_bound(Fp2<P>& a, double vb, bool check) { agg_bound(a.c0, vb, check); agg_bound(a.c1, vb, check); }
template <class F> HD void agg_bounds(Xyzz<F>& a, bool check) { agg_bound(a.X, 19, check); agg_bound(a.Y, 7, check); agg_bound(a.ZZ, 3, check); agg_bound(a.ZZZ, 3, check); }
template <class F> HD void agg_store(uint32_t* slot, const Xyzz<F>& a) {
  constexpr int FW = F::WORDS;
  TRK(Xyzz<F> c = a; agg_bounds(c, true);)
  a.X.store(slot); a.Y.store(slot + FW); a.ZZ.store(slot + 2 * FW); a.ZZZ.store(slot + 3 * FW);
}
// a += the stored point at src: xyzz_add_mem of curve.h, which reads the point where it is used; into an identity accumulator the whole
// point is loaded, with its bounds
template <class F> HD void agg_add_stored(Xyzz<F>& a, const uint32_t* src) {
  constexpr int FW = F::WORDS;
  if (a.is_identity()) {
    a = {F::load(src), F::load(src + FW), F::load(src + 2 * FW), F::load(src + 3 * FW)};
    agg_bounds(a, false);
    return;
  }
  xyzz_add_mem<F>(a, src);
}

// phase 1 of lane `lane` of `L`: rows xy / inf (n of them, inf may be null) under the n bytes of bits; bits == null selects every row (the
// set's total).  neg: the complement's side - the rows at the ZERO bytes, negated.
template <class F> HD Xyzz<F> agg_lane_sum(const uint64_t* xy, const uint8_t* inf, const uint8_t* bits, uint32_t n, uint32_t lane, uint32_t L, bool neg) {
  constexpr int A = F::ARK64;
  Xyzz<F> acc = Xyzz<F>::identity();
  // The lane steps from one of ITS rows to the next (the scan is a few byte loads), so that the k-th addition of every lane of a wave runs
  // at the same time: a wave takes as many additions as its busiest lane has rows.  One loop over j with the addition under the test takes
  // an addition's time for every j that ANY lane of the wave selects - with 64 bitmaps in a wave, nearly every j, whichever side was chosen.
  for (uint64_t j = lane;; j += L) {              // (64 bits: j + L passes n, which may be near 2^32)
    while (j < n && (((bits ? bits[j] != 0 : true) == neg) || (inf && inf[j]))) j += L;
    if (j >= n) break;
    const uint64_t* row = xy + (size_t)j * 2 * A;
    Affine<F> p = {F::norm(F::from_ark(row)), F::norm(F::from_ark(row + A))};
    if (neg) p = affine_neg(p);
    xyzz_madd(acc, p);
  }
  return acc;
}

// phase 2, the round of stride s seen from lane l < s: acc += the partial in slot l + s.  The rounds run s = L/2, L/4, .. 1; after each but
// the last, lane l < s stores acc to slot l, and the next round starts when those stores have landed.
template <class F> HD void agg_fold_step(Xyzz<F>& acc, const uint32_t* slots, uint32_t lane, uint32_t s) {
  agg_add_stored<F>(acc, slots + (size_t)(lane + s) * agg_slot_words<F>());
}
// lane 0 after the fold: the complement's side adds the set's total (an XYZZ point of 4 F::WORDS words)
template <class F> HD void agg_finish(Xyzz<F>& acc, bool neg, const uint32_t* total) {
  if (neg) agg_add_stored<F>(acc, total);
}

}  // namespace celo
