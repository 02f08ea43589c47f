// Bowe-Hopwood-Pedersen CRH evaluation over the twisted Edwards curve ed-on-BW6-761 (-x^2 + y^2 = 1 + 79743 x^2 y^2 over Fq of
// BLS12-377) - the composite hasher's CRH (crates/bls-crypto/src/hashers/composite.rs:79-86: bowe_hopwood::CRH::evaluate with
// WINDOW_SIZE = 93, NUM_WINDOWS = 560), host+device templates.  The message is cut into 3-bit chunks (LSB-first, zero
// padded); chunk ch uses generator ch of the window-major table (generator j of a window = 16^j * its base) and contributes
// (1 + b0 + 2 b1) * g, negated when b2 is set; the hash is the affine x coordinate of the sum, 48 bytes little-endian.
// The generator table itself is built on the host (seam_hash.hip: ChaCha20 stream exactly as the reference consumes it) and
// handed to the device once.  It holds FOUR entries per chunk - g, 2g, 3g, 4g (PEDERSEN_MULTIPLES) - so that a chunk's contribution
// (1 + b0 + 2 b1) g is one table entry and costs ONE point addition; round 2 kept g alone and formed the multiple per chunk (up to two
// additions and a doubling before the one that counts: 2.5 point operations per chunk on average).  Same group element, same hash.  One source for Seam A's host path (hash_crh, the composite hashers) and the bulk GPU
// kernels (unit_hash.hip: k_pedersen_crh, one message per lane; unit_hash_lanes.hip: k_pedersen_crh_lanes, several lanes per message, below).
#pragma once
#include "wire.h"

namespace celo {

struct SF {  // "safe" field element: every result weak-reduced and normalised (the sums dominate; no lazy-bound bookkeeping)
  Fq v;
  HD static SF from(const Fq& x) { return {Fq::wred(Fq::norm(x))}; }
  HD SF operator+(const SF& o) const { return from(Fq::add(v, o.v)); }
  HD SF operator-(const SF& o) const { return from(Fq::sub<4, 1>(v, o.v)); }
  HD SF operator*(const SF& o) const { return from(Fq::mul(v, o.v)); }
  HD SF neg() const { return from(Fq::neg<4, 1>(v)); }
  HD SF dbl() const { return from(Fq::add(v, v)); }
};
struct EdPoint { SF X, Y, Z, T; };  // extended twisted Edwards, a = -1
HD SF sf_small(uint64_t k) { uint64_t w[6] = {k, 0, 0, 0, 0, 0}; return SF::from(Fq::from_canonical(w)); }
WIRE_FN EdPoint ed_add(const EdPoint& p, const EdPoint& q) {  // add-2008-hwcd-3 (a = -1)
  const SF d2 = sf_small(2 * 79743);
  SF A = (p.Y - p.X) * (q.Y - q.X), B = (p.Y + p.X) * (q.Y + q.X), C = p.T * d2 * q.T, D = (p.Z * q.Z).dbl();
  SF E = B - A, F = D - C, G = D + C, H = B + A;
  return {E * F, G * H, F * G, E * H};
}
WIRE_FN EdPoint ed_dbl(const EdPoint& p) {  // dbl-2008-hwcd (a = -1)
  SF A = p.X * p.X, B = p.Y * p.Y, C = (p.Z * p.Z).dbl(), D = A.neg();
  SF E = (p.X + p.Y) * (p.X + p.Y) - A - B, G = D + B, F = G - C, H = D - B;
  return {E * F, G * H, F * G, E * H};
}
HD EdPoint ed_neg(const EdPoint& p) { return {p.X.neg(), p.Y, p.Z, p.T.neg()}; }
HD EdPoint ed_zero() { return {sf_small(0), sf_small(1), sf_small(1), sf_small(0)}; }

constexpr int PEDERSEN_WINDOW_SIZE = 93, PEDERSEN_NUM_WINDOWS = 560, PEDERSEN_MULTIPLES = 4;
constexpr size_t PEDERSEN_MAX_BITS = (size_t)PEDERSEN_WINDOW_SIZE * PEDERSEN_NUM_WINDOWS * 3;

// out48 = x coordinate of sum_ch enc_ch over the bytes src(0 .. src.size()); the caller has checked size * 8 <= PEDERSEN_MAX_BITS
// (the reference panics beyond).  Src: any byte source with size() and operator()(j) (a plain buffer, or the counter || extra ||
// message string of a try-and-increment attempt).
struct PtrBytes {
  const uint8_t* p;
  size_t n;
  HD size_t size() const { return n; }
  HD uint8_t operator()(size_t j) const { return p[j]; }
};
// the contribution of chunk ch: three message bits, LSB-first within a byte, zero beyond the end, pick (1 + b0 + 2 b1) * generator ch, negated under b2.
// pedersen_crh_src below holds the SAME lines written out (see there): change both or neither; tests/test_crh_lanes_host.py compares the two forms.
template <class Src> HD EdPoint pedersen_chunk(const EdPoint* gens, const Src& src, size_t len, size_t ch) {
  const size_t b = 3 * ch;
  uint32_t two = src(b >> 3);
  if ((b >> 3) + 1 < len) two |= (uint32_t)src((b >> 3) + 1) << 8;
  const uint32_t bits = (two >> (b & 7)) & 7u;
  EdPoint enc = gens[(size_t)PEDERSEN_MULTIPLES * ch + (bits & 3u)];
  if (bits & 4) enc = ed_neg(enc);
  return enc;
}
// the hash of a sum: its affine x, 48 canonical bytes little-endian
HD void pedersen_crh_finish(const EdPoint& total, uint8_t out48[48]) {
  const SF x = total.X * SF::from(wire_inv(total.Z.v));
  uint64_t w[6];
  x.v.to_canonical(w);
#pragma unroll   // in a function of its own the loop is otherwise left rolled and w[] indexed at run time; unrolled, k_pedersen_crh is the code it was
  for (int i = 0; i < 48; i++) out48[i] = (uint8_t)(w[i >> 3] >> (8 * (i & 7)));
}
template <class Src> HD void pedersen_crh_src(const EdPoint* gens, const Src& src, uint8_t out48[48]) {
  const size_t len = src.size(), nbits = len * 8, nchunks = (nbits + 2) / 3;
  EdPoint total = ed_zero();
  for (size_t ch = 0; ch < nchunks; ch++) {   // pedersen_chunk above, written out - keep the two in step: through the helper k_pedersen_crh's frame is laid out the other way round
    const size_t b = 3 * ch;
    // three message bits, LSB-first within a byte, zero beyond the end
    uint32_t two = src(b >> 3);
    if ((b >> 3) + 1 < len) two |= (uint32_t)src((b >> 3) + 1) << 8;
    const uint32_t bits = (two >> (b & 7)) & 7u;
    EdPoint enc = gens[(size_t)PEDERSEN_MULTIPLES * ch + (bits & 3u)];     // (1 + b0 + 2 b1) * generator ch
    if (bits & 4) enc = ed_neg(enc);
    total = ed_add(total, enc);
  }
  pedersen_crh_finish(total, out48);
}
HD void pedersen_crh(const EdPoint* gens, const uint8_t* msg, size_t len, uint8_t out48[48]) { pedersen_crh_src(gens, PtrBytes{msg, len}, out48); }

// ---- several lanes per message (unit_hash_lanes.hip: k_pedersen_crh_lanes; host_test.cpp: ht_pedersen_crh_lanes).  The hash is the x of a sum in
// a group and ed_add is complete on this curve (a = -1 is a square, q = 1 mod 4; d = 79743 is not), so the chunks may be summed in any order
// and partial sums that are the identity, equal or opposite need no special case.  Lane `lane` of L sums the chunks ch = lane (mod L):
// strided, so that lanes differ by at most one chunk and neighbouring lanes read neighbouring message bytes and table rows.  The L partials
// are folded pairwise through a buffer of slots (LDS on the device): in the round of stride s = L/2, L/4, .. 1 lane l < s adds the partial in
// slot l + s to its own and stores the result in slot l; lane 0 finishes.  A lane without a chunk carries ed_zero() into the fold.
template <class Src> HD EdPoint pedersen_crh_lane_sum(const EdPoint* gens, const Src& src, uint32_t lane, uint32_t L) {
  const size_t len = src.size(), nchunks = (len * 8 + 2) / 3;
  EdPoint total = ed_zero();
  for (size_t ch = lane; ch < nchunks; ch += L) total = ed_add(total, pedersen_chunk(gens, src, len, ch));
  return total;
}
// a slot of the fold buffer: four normalised Fq, Fq::WORDS words each
constexpr uint32_t CRH_SLOT_WORDS = 4 * Fq::WORDS;
HD void ed_store(uint32_t* slot, const EdPoint& p) {
  constexpr int FW = Fq::WORDS;
  p.X.v.store(slot); p.Y.v.store(slot + FW); p.Z.v.store(slot + 2 * FW); p.T.v.store(slot + 3 * FW);
}
HD EdPoint ed_load(const uint32_t* slot) {
  constexpr int FW = Fq::WORDS;
  return {SF::from(Fq::load(slot)), SF::from(Fq::load(slot + FW)), SF::from(Fq::load(slot + 2 * FW)), SF::from(Fq::load(slot + 3 * FW))};
}

// The lane width of a call: c = the chunk count of its longest message, n the number of messages.
//   L = min( smallest power of two >= c / CRH_CHUNKS_PER_LANE,  largest power of two <= CRH_FILL_LANES / n ),  at least 1, at most 256
// A lane should have CRH_CHUNKS_PER_LANE additions of its own before the fold's log2 L additions and barriers are worth paying, and past
// CRH_FILL_LANES lanes in flight more lanes per message only add fold work to a device that is already full; a call of CRH_FILL_LANES
// messages or more runs one lane per message, the kernel it always ran.  request != 0 (celo_amd_crh_set_lanes) is taken as the width.
// Either way the width is halved while n L lanes need more workgroups of CRH_BLOCK lanes than a 31-bit grid holds.
// The constants against a same-run A/B over all nine widths (tools/bench_crh_lanes.py, profiles/bench_crh_lanes.json; kernel
// ms, best width / the rule's): 1 x 14 200 B 2.95 at 256 / 256; 64 x 10 400 B 2.35 at 256 / 256 (one lane: 458); 143 x 14 200 B 3.30 at 256 /
// 256; 2 048 x 10 400 B 16.8 at 256 (16.8 - 17.2 from 64 up) / 18.4 at 32, 1.09 x: CRH_FILL_LANES = 2^17 would pick 64 there, but two lanes at
// 65 536 x 127 B, and the bulk short-message calls keep the one-lane kernel; 65 536 x 127 B 6.6 at 2 / 7.6 at 1, 1.15 x, for that reason;
// 65 537 x 12 B 1.11 at 1 / 1.  The work term alone, on an empty device: 64 x 400 B (1 067 chunks) 0.44 at 256 / 1.01 at 64, 2.3 x; 64 x 100 B
// (267 chunks) 0.38 at 256 / 0.90 at 16, 2.4 x - there every doubling still pays down to ONE chunk per lane, so a smaller
// CRH_CHUNKS_PER_LANE would be faster by 0.5 ms on such calls.  32 is the smallest value under which a call of 12-byte messages (32 chunks,
// the bulk shape below CRH_FILL_LANES messages too) keeps the one-lane kernel, which is asked of the rule; it is a floor, not an optimum.
constexpr uint32_t CRH_MAX_LANES = 256;
constexpr uint32_t CRH_BLOCK = 256;              // lanes of a workgroup of the lanes kernel: CRH_BLOCK / L messages each
constexpr uint32_t CRH_CHUNKS_PER_LANE = 32;
constexpr uint32_t CRH_FILL_LANES = 1u << 16;
HD bool crh_lanes_ok(int L) { return L >= 1 && L <= (int)CRH_MAX_LANES && (L & (L - 1)) == 0; }
inline uint32_t crh_pick_lanes(uint32_t request, size_t max_chunks, size_t n) {
  uint32_t L = request;
  if (!L) {
    uint32_t work = 1, fill = CRH_MAX_LANES;
    while (work < CRH_MAX_LANES && (uint64_t)work * CRH_CHUNKS_PER_LANE < max_chunks) work <<= 1;
    while (fill > 1 && (uint64_t)fill * n > CRH_FILL_LANES) fill >>= 1;
    L = work < fill ? work : fill;
  }
  while (L > 1 && (uint64_t)n * L > (uint64_t)0x7fffffffu * CRH_BLOCK) L >>= 1;
  return L;
}

}  // namespace celo
