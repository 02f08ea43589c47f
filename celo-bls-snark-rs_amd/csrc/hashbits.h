// The HashToBits circuit of the hash-helper proof (crates/epoch-snark/src/gadgets/hash_to_bits.rs, generate_hash_helper in
// api/prover.rs:85-118) over Fr(BLS12-377): its R1CS, its assignment from the CRH rows and its public inputs, as host+device templates.
// DESIGN.md section 6m holds the layout, the counts and the soundness argument.
//
// The statement is the reference's.  Per epoch 384 message bits (bit j of a message = bit j % 8 of byte j / 8 of its 48-byte row with
// bit_order 0, the 384-bit reversal of that with bit_order 1: bytes_le_to_bits_be, what prover.rs:101 feeds) go through the two
// single-block Blake2s compressions of the Blake2Xs XOF under SIG_DOMAIN (bls-gadgets hash_to_group.rs:192-250) to 512 bits; the instance is
// [1] ++ pack(all message bits, 252) ++ pack(all XOF bits, 252), the first bit of a chunk the most significant (gadgets/pack.rs).
// The LAYOUT is this library's: the reference's order of variables and constraints comes from the arkworks gadgets, which cannot be
// reproduced here, so a key made for this system is no ceremony key of the reference and the other way round.
//
// One generic routine, hb_compress, walks the compression once per "ops" policy: HbTraceOps computes on u32 words and stores every
// word-valued intermediate (k_hashbits_trace and the host twin), HbSymOps (host) walks the same steps over bits as linear forms and emits the
// rows and the variables' descriptors.  A slot of the trace is the index of the step that made it in both, which is what ties a variable to
// its value.  The assignment is then a pure expansion: variable -> (trace word, bit) -> the Montgomery 0 or 1.
#pragma once
#include <cstring>
#include <map>
#include <vector>
#include "epoch.h"

namespace celo {

constexpr uint32_t HB_MSG_BITS = 384, HB_MSG_WORDS = 12, HB_ROW_BYTES = 48, HB_XOF_BITS = 512, HB_CAP = 252;
constexpr uint32_t HB_STEP_SLOTS = 80 * 12 + 8;            // per compression: 80 G of 4 additions (sum, carry) and 4 XORs, then v[i] ^ v[i + 8]
constexpr uint32_t HB_COMP_WORDS = HB_STEP_SLOTS + 8;      // ... and the final h
constexpr uint32_t HB_TRACE_WORDS = HB_MSG_WORDS + 2 * HB_COMP_WORDS;   // per epoch: the message words, compression 0, compression 1
constexpr size_t HB_MAX_EPOCHS = 1u << 16;                 // far above what log_n <= 28 admits; keeps every count below 2^63

HD uint32_t hb_final_word(uint32_t comp, uint32_t j) { return HB_MSG_WORDS + comp * HB_COMP_WORDS + HB_STEP_SLOTS + j; }
HD uint32_t hb_msg_chunks(uint64_t m) { return (uint32_t)((HB_MSG_BITS * m + HB_CAP - 1) / HB_CAP); }
HD uint32_t hb_xof_chunks(uint64_t m) { return (uint32_t)((HB_XOF_BITS * m + HB_CAP - 1) / HB_CAP); }
HD uint32_t hb_n_inputs(uint64_t m) { return 1 + hb_msg_chunks(m) + hb_xof_chunks(m); }

// ---- Fr(BLS12-377) on four u64: only what a 0 / 1 expansion and a 252-bit pack need
struct HbFr {
  static constexpr uint64_t P[4] = {0x0a11800000000001ULL, 0x59aa76fed0000001ULL, 0x60b44d1e5c37b001ULL, 0x12ab655e9a2ca556ULL};
  static constexpr uint64_t R[4] = {0x7d1c7ffffffffff3ULL, 0x7257f50f6ffffff2ULL, 0x16d81575512c0feeULL, 0x0d4bda322bbb9a9dULL};    // 2^256 mod r
  static constexpr uint64_t R2[4] = {0x25d577bab861857bULL, 0xcc2c27b58860591fULL, 0xa7cc008fe5dc8593ULL, 0x011fdae7eff1c939ULL};   // 2^512 mod r
  static constexpr uint64_t INV = 0x0a117fffffffffffULL;   // -r^-1 mod 2^64
};
HD uint64_t hb_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}
// t += a * b + c -> the low word in t, the high word returned
HD uint64_t hb_mac(uint64_t& t, uint64_t a, uint64_t b, uint64_t c) {
  const uint64_t lo = a * b;
  uint64_t hi = hb_mulhi(a, b);
  uint64_t s = t + lo;
  hi += s < lo;
  const uint64_t s2 = s + c;
  hi += s2 < s;
  t = s2;
  return hi;
}
// a b / 2^256 mod r (CIOS); a, b < r -> out < r
HD void hb_montmul(const uint64_t a[4], const uint64_t b[4], uint64_t out[4]) {
  uint64_t t[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 4; i++) {
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) c = hb_mac(t[j], a[j], b[i], c);
    uint64_t s = t[4] + c;
    t[5] = s < c;
    t[4] = s;
    const uint64_t q = t[0] * HbFr::INV;
    uint64_t z = t[0];
    c = hb_mac(z, q, HbFr::P[0], 0);
#pragma unroll
    for (int j = 1; j < 4; j++) { c = hb_mac(t[j], q, HbFr::P[j], c); t[j - 1] = t[j]; }
    s = t[4] + c;
    t[3] = s;
    t[4] = t[5] + (s < c);
  }
  uint64_t d[4], borrow = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const uint64_t x = t[j] - HbFr::P[j], y = x - borrow;
    borrow = (t[j] < HbFr::P[j]) | (x < borrow);
    d[j] = y;
  }
  const bool ge = t[4] != 0 || borrow == 0;
#pragma unroll
  for (int j = 0; j < 4; j++) out[j] = ge ? d[j] : t[j];
}
HD void hb_to_mont(const uint64_t canonical[4], uint64_t out[4]) { hb_montmul(canonical, HbFr::R2, out); }

// ---- the message words of one 48-byte row: bit k of word w is message bit 32 w + k
HD void hb_message_words(const uint8_t* row, int bit_order, uint32_t m[16]) {
#pragma unroll
  for (int w = 0; w < 16; w++) m[w] = 0;
  for (int w = 0; w < (int)HB_MSG_WORDS; w++) {
    uint32_t v = 0;
    for (int b = 3; b >= 0; b--) v = (v << 8) | row[4 * w + b];
    if (bit_order == 0) m[w] = v;
    else m[HB_MSG_WORDS - 1 - w] = epoch_rev32(v);
  }
}

// ---- the compression, once for every policy O.  O::W is a word; o.add3 / o.add2 / o.xr take one trace slot pair / one slot each, in the
// order they are called; konst, rotr and xork take none.  h0 = IV ^ parameter block of the compression, t = 48 bytes, the last block.
template <class O> HD void hb_compress(O& o, const uint32_t h0[8], const typename O::W m[16], typename O::W out[8]) {
  typedef typename O::W W;
  W v[16];
#pragma unroll
  for (int i = 0; i < 8; i++) { v[i] = O::konst(h0[i]); v[i + 8] = O::konst(B2sTab::IV[i]); }
  v[12] = O::konst(B2sTab::IV[4] ^ HB_ROW_BYTES);
  v[14] = O::konst(~B2sTab::IV[6]);
#define CELO_HB_G(a, b, c, d, x, y)                                      \
  v[a] = o.add3(v[a], v[b], (x)); v[d] = O::rotr(o.xr(v[d], v[a]), 16);  \
  v[c] = o.add2(v[c], v[d]);      v[b] = O::rotr(o.xr(v[b], v[c]), 12);  \
  v[a] = o.add3(v[a], v[b], (y)); v[d] = O::rotr(o.xr(v[d], v[a]), 8);   \
  v[c] = o.add2(v[c], v[d]);      v[b] = O::rotr(o.xr(v[b], v[c]), 7);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int r = 0; r < 10; r++) {
    CELO_HB_G(0, 4, 8, 12, m[B2sTab::SIGMA[r][0]], m[B2sTab::SIGMA[r][1]])
    CELO_HB_G(1, 5, 9, 13, m[B2sTab::SIGMA[r][2]], m[B2sTab::SIGMA[r][3]])
    CELO_HB_G(2, 6, 10, 14, m[B2sTab::SIGMA[r][4]], m[B2sTab::SIGMA[r][5]])
    CELO_HB_G(3, 7, 11, 15, m[B2sTab::SIGMA[r][6]], m[B2sTab::SIGMA[r][7]])
    CELO_HB_G(0, 5, 10, 15, m[B2sTab::SIGMA[r][8]], m[B2sTab::SIGMA[r][9]])
    CELO_HB_G(1, 6, 11, 12, m[B2sTab::SIGMA[r][10]], m[B2sTab::SIGMA[r][11]])
    CELO_HB_G(2, 7, 8, 13, m[B2sTab::SIGMA[r][12]], m[B2sTab::SIGMA[r][13]])
    CELO_HB_G(3, 4, 9, 14, m[B2sTab::SIGMA[r][14]], m[B2sTab::SIGMA[r][15]])
  }
#undef CELO_HB_G
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = O::xork(o.xr(v[i], v[i + 8]), h0[i]);
}
// h0 of compression `comp` (0 / 1) of the 64-byte XOF under SIG_DOMAIN: DirectHasher::xof's parameter block (hash_direct.h tai_candidate)
HD void hb_h0(uint32_t comp, uint32_t h0[8]) {
  const uint8_t dom[8] = {'U', 'L', 'f', 'o', 'r', 'x', 'o', 'f'};
  b2s_init(h0, 32, 0, 0, 32, b2x_node_offset(comp, 64), 0, 32, dom);
}

// the policy that computes: slot n of tr = the n-th intermediate (a sum's low word, then its carry; an XOR's result before the rotation)
struct HbTraceOps {
  typedef uint32_t W;
  uint32_t* tr;
  uint32_t n;
  HD static W konst(uint32_t c) { return c; }
  HD static W rotr(W w, int k) { return b2s_rotr(w, k); }
  HD static W xork(W w, uint32_t c) { return w ^ c; }
  HD W add3(W a, W b, W x) {
    const uint64_t s = (uint64_t)a + b + x;
    tr[n++] = (uint32_t)s; tr[n++] = (uint32_t)(s >> 32);
    return (uint32_t)s;
  }
  HD W add2(W a, W b) {
    const uint64_t s = (uint64_t)a + b;
    tr[n++] = (uint32_t)s; tr[n++] = (uint32_t)(s >> 32);
    return (uint32_t)s;
  }
  HD W xr(W a, W b) { const W r = a ^ b; tr[n++] = r; return r; }
};
// One lane of the trace: compression `comp` of the message in `row` into the epoch's trace (HB_TRACE_WORDS words); comp 0 also stores the
// message words.
HD void hb_trace_lane(const uint8_t* row, int bit_order, uint32_t comp, uint32_t* epoch_trace) {
  uint32_t m[16], h0[8], out[8];
  hb_message_words(row, bit_order, m);
  if (comp == 0) for (int w = 0; w < (int)HB_MSG_WORDS; w++) epoch_trace[w] = m[w];
  hb_h0(comp, h0);
  HbTraceOps o = {epoch_trace + HB_MSG_WORDS + comp * HB_COMP_WORDS, 0};
  hb_compress(o, h0, m, out);
#pragma unroll
  for (int j = 0; j < 8; j++) epoch_trace[hb_final_word(comp, j)] = out[j];
}

// ---- expansion: descriptor = trace word << 5 | bit.  Variable i of the call: 0 the constant, [1, n_inputs) the instance (hb_pack_input),
// then epoch-major with `stride` variables per epoch.  `half` selects limbs 0..1 or 2..3 of the row, so that two neighbouring lanes write one.
HD bool hb_var_bit(const uint32_t* __restrict__ desc, const uint32_t* __restrict__ trace, uint32_t stride, uint32_t n_inputs, uint32_t i) {
  const uint32_t j = i - n_inputs, e = j / stride, d = desc[j - e * stride];
  return (trace[(size_t)e * HB_TRACE_WORDS + (d >> 5)] >> (d & 31)) & 1u;
}

// ---- packing.  Bit g of the message stream / the XOF stream of the call (epochs in order) from the trace
HD uint32_t hb_msg_bit(const uint32_t* trace, uint64_t g) {
  const uint64_t e = g / HB_MSG_BITS;
  const uint32_t j = (uint32_t)(g - e * HB_MSG_BITS);
  return (trace[e * HB_TRACE_WORDS + (j >> 5)] >> (j & 31)) & 1u;
}
HD uint32_t hb_xof_bit(const uint32_t* trace, uint64_t g) {
  const uint64_t e = g / HB_XOF_BITS;
  const uint32_t j = (uint32_t)(g - e * HB_XOF_BITS);
  return (trace[e * HB_TRACE_WORDS + hb_final_word(j >> 8, (j >> 5) & 7)] >> (j & 31)) & 1u;
}
// instance variable c + 1 (c < msg chunks + xof chunks) of m epochs as a canonical integer: the first bit of the chunk on top
HD void hb_pack_chunk(const uint32_t* trace, uint64_t m, uint32_t c, uint64_t out[4]) {
  const uint32_t mc = hb_msg_chunks(m);
  const bool xof = c >= mc;
  const uint64_t total = (xof ? HB_XOF_BITS : HB_MSG_BITS) * m, lo = (uint64_t)(xof ? c - mc : c) * HB_CAP;
  const uint32_t len = total - lo < HB_CAP ? (uint32_t)(total - lo) : HB_CAP;
  out[0] = out[1] = out[2] = out[3] = 0;
  for (uint32_t t = 0; t < len; t++) {
    const uint32_t bit = xof ? hb_xof_bit(trace, lo + t) : hb_msg_bit(trace, lo + t), q = len - 1 - t;
    out[q >> 6] |= (uint64_t)bit << (q & 63);
  }
}

// ================================================================ host: the template of one epoch and the matrices of m

// a bit as a linear form: a constant (var < 0, value neg), a variable x (neg = 0) or 1 - x (neg = 1).  var is local to the epoch.
struct HbBit { int32_t var; uint8_t neg; };
struct HbSymWord { HbBit b[32]; };
// one matrix of the template: entries (local column, coefficient); local column 0 = the constant one, 1 + v = variable v of the epoch
struct HbTplMat {
  std::vector<uint64_t> row_ptr{0};
  std::vector<uint32_t> col;
  std::vector<int64_t> coef;
  void end_row() { row_ptr.push_back(col.size()); }
  void put(const std::map<uint32_t, int64_t>& lc) { for (auto& kv : lc) if (kv.second) { col.push_back(kv.first); coef.push_back(kv.second); } }
};
struct HbTemplate {
  HbTplMat mat[3];
  std::vector<uint32_t> desc;          // per variable: trace word << 5 | bit
  HbBit xof[HB_XOF_BITS];              // the 512 output bits as forms over the epoch's variables
  uint32_t rows = 0;
  uint32_t stride() const { return (uint32_t)desc.size(); }
};

struct HbSymOps {
  typedef HbSymWord W;
  typedef std::map<uint32_t, int64_t> Lc;
  HbTemplate& T;
  uint32_t base;       // the trace word of slot 0 of this compression
  uint32_t n = 0;
  static W konst(uint32_t c) { W w; for (int k = 0; k < 32; k++) w.b[k] = {-1, (uint8_t)((c >> k) & 1)}; return w; }
  static W rotr(const W& w, int r) { W o; for (int k = 0; k < 32; k++) o.b[k] = w.b[(k + r) & 31]; return o; }
  static W xork(const W& w, uint32_t c) { W o = w; for (int k = 0; k < 32; k++) o.b[k].neg ^= (c >> k) & 1; return o; }
  int32_t new_var(uint32_t word, uint32_t bit) { T.desc.push_back(word << 5 | bit); return (int32_t)T.desc.size() - 1; }
  static void add_form(Lc& lc, const HbBit& b, int64_t coef) {
    if (b.var < 0) { if (b.neg) lc[0] += coef; return; }
    if (b.neg) { lc[0] += coef; lc[1 + b.var] -= coef; } else lc[1 + b.var] += coef;
  }
  void row(const Lc& a, const Lc& b, const Lc& c) {
    T.mat[0].put(a); T.mat[1].put(b); T.mat[2].put(c);
    for (int k = 0; k < 3; k++) T.mat[k].end_row();
    T.rows++;
  }
  void boolean_row(int32_t v) { row(Lc{{1u + v, 1}}, Lc{{0u, 1}, {1u + v, -1}}, Lc{}); }     // x (1 - x) = 0
  // sum of the operands = result + 2^32 carry: one linear row, a booleanity row per result bit and carry bit.  The carry takes as many bits
  // as the largest sum needs; all-constant operands make a constant.
  W add(const W* ops, int nops) {
    const uint32_t slot = base + n;
    n += 2;
    Lc lc;
    uint64_t max = 0;
    bool any = false;
    for (int q = 0; q < nops; q++)
      for (int k = 0; k < 32; k++) {
        const HbBit& b = ops[q].b[k];
        add_form(lc, b, int64_t(1) << k);
        if (b.var >= 0) { any = true; max += uint64_t(1) << k; } else if (b.neg) max += uint64_t(1) << k;
      }
    if (!any) return konst((uint32_t)max);
    W res;
    for (int k = 0; k < 32; k++) { res.b[k] = {new_var(slot, k), 0}; lc[1 + res.b[k].var] -= int64_t(1) << k; }
    int32_t cv[2];
    int nc = 0;
    for (uint64_t c = max >> 32; c; c >>= 1) { cv[nc] = new_var(slot + 1, nc); lc[1 + cv[nc]] -= int64_t(1) << (32 + nc); nc++; }
    row(lc, Lc{{0u, 1}}, Lc{});
    for (int k = 0; k < 32; k++) boolean_row(res.b[k].var);
    for (int k = 0; k < nc; k++) boolean_row(cv[k]);
    return res;
  }
  W add3(const W& a, const W& b, const W& x) { const W ops[3] = {a, b, x}; return add(ops, 3); }
  W add2(const W& a, const W& b) { const W ops[2] = {a, b}; return add(ops, 2); }
  // c = a ^ b per bit: free when either is a constant, else (2 a) b = a + b - c with a new variable c
  W xr(const W& a, const W& b) {
    const uint32_t slot = base + n;
    n += 1;
    W res;
    for (int k = 0; k < 32; k++) {
      const HbBit &x = a.b[k], &y = b.b[k];
      if (x.var < 0) { res.b[k] = {y.var, (uint8_t)(y.neg ^ x.neg)}; continue; }
      if (y.var < 0) { res.b[k] = {x.var, (uint8_t)(x.neg ^ y.neg)}; continue; }
      res.b[k] = {new_var(slot, k), 0};
      Lc la, lb, lc;
      add_form(la, x, 2); add_form(lb, y, 1); add_form(lc, x, 1); add_form(lc, y, 1);
      lc[1 + res.b[k].var] -= 1;
      row(la, lb, lc);
    }
    return res;
  }
};

// built once per process (the circuit is the same for every epoch)
inline const HbTemplate& hb_template() {
  static const HbTemplate* tpl = [] {
    HbTemplate* T = new HbTemplate();
    HbSymWord m[16];
    HbSymOps boot{*T, 0};
    for (int w = 0; w < 16; w++) m[w] = HbSymOps::konst(0);
    for (uint32_t j = 0; j < HB_MSG_BITS; j++) m[j >> 5].b[j & 31] = {boot.new_var(j >> 5, j & 31), 0};
    for (uint32_t j = 0; j < HB_MSG_BITS; j++) boot.boolean_row((int32_t)j);
    for (uint32_t comp = 0; comp < 2; comp++) {
      uint32_t h0[8];
      hb_h0(comp, h0);
      HbSymOps o{*T, HB_MSG_WORDS + comp * HB_COMP_WORDS};
      HbSymWord out[8];
      hb_compress(o, h0, m, out);
      for (int j = 0; j < 8; j++) for (int k = 0; k < 32; k++) T->xof[256 * comp + 32 * j + k] = out[j].b[k];
    }
    return T;
  }();
  return *tpl;
}

// a signed coefficient, or +-2^k, in arkworks Montgomery limbs
inline void hb_coef_mont(int64_t c, uint64_t out[4]) {
  uint64_t v[4] = {c < 0 ? (uint64_t)(-c) : (uint64_t)c, 0, 0, 0};
  if (c < 0) {
    uint64_t borrow = 0;
    for (int j = 0; j < 4; j++) {
      const uint64_t x = HbFr::P[j] - v[j], y = x - borrow;
      borrow = (HbFr::P[j] < v[j]) | (x < borrow);
      v[j] = y;
    }
  }
  hb_to_mont(v, out);
}
inline void hb_pow2_mont(uint32_t k, bool negative, uint64_t out[4]) {
  uint64_t v[4] = {0, 0, 0, 0};
  v[k >> 6] = uint64_t(1) << (k & 63);
  if (negative) {
    uint64_t borrow = 0;
    for (int j = 0; j < 4; j++) {
      const uint64_t x = HbFr::P[j] - v[j], y = x - borrow;
      borrow = (HbFr::P[j] < v[j]) | (x < borrow);
      v[j] = y;
    }
  }
  hb_to_mont(v, out);
}

// the pack row of chunk c as (column, +-2^k or the constant) entries: sum 2^(len-1-t) bit_t - input = 0.  emit(col, pow, negative) for a
// power of two, constant(canonical limbs) for the row's constant term (only called when it is not zero).
template <class Emit, class Const> inline void hb_pack_row(const HbTemplate& T, uint64_t m, uint32_t c, Emit emit, Const constant) {
  const uint32_t mc = hb_msg_chunks(m), n_inputs = hb_n_inputs(m), stride = T.stride();
  const bool xof = c >= mc;
  const uint64_t per = xof ? HB_XOF_BITS : HB_MSG_BITS, total = per * m, lo = (uint64_t)(xof ? c - mc : c) * HB_CAP;
  const uint32_t len = total - lo < HB_CAP ? (uint32_t)(total - lo) : HB_CAP;
  uint64_t k0[4] = {0, 0, 0, 0};
  for (uint32_t t = 0; t < len; t++) if (xof && T.xof[(lo + t) % per].neg) { const uint32_t q = len - 1 - t; k0[q >> 6] |= uint64_t(1) << (q & 63); }
  if (k0[0] | k0[1] | k0[2] | k0[3]) constant(k0);
  emit(1 + c, 0u, true);
  for (uint32_t t = 0; t < len; t++) {
    const uint64_t g = lo + t, e = g / per;
    const uint32_t j = (uint32_t)(g - e * per);
    const HbBit b = xof ? T.xof[j] : HbBit{(int32_t)j, 0};
    emit((uint32_t)(n_inputs + e * stride + b.var), len - 1 - t, b.neg != 0);
  }
}

struct HbSizes { uint64_t n_constraints, n_vars, n_inputs, nnz[3], log_n, stride; };
// 0, or 2: m == 0, or the circuit exceeds the R1CS limits (n_vars or an nnz >= 2^32, log_n > 28)
inline int hb_sizes(size_t m, HbSizes* s) {
  if (m == 0 || m > HB_MAX_EPOCHS || !s) return 2;
  const HbTemplate& T = hb_template();
  s->n_inputs = hb_n_inputs(m);
  s->stride = T.stride();
  s->n_vars = s->n_inputs + (uint64_t)m * T.stride();
  s->n_constraints = (uint64_t)m * T.rows + s->n_inputs - 1;
  for (int k = 0; k < 3; k++) s->nnz[k] = (uint64_t)m * T.mat[k].col.size();
  s->nnz[1] += s->n_inputs - 1;
  for (uint32_t c = 0; c + 1 < s->n_inputs; c++) hb_pack_row(T, m, c, [&](uint32_t, uint32_t, bool) { s->nnz[0]++; }, [&](const uint64_t*) { s->nnz[0]++; });
  s->log_n = 0;
  while ((uint64_t(1) << s->log_n) < s->n_constraints + s->n_inputs) s->log_n++;
  if (s->n_vars >> 32 || s->nnz[0] >> 32 || s->nnz[1] >> 32 || s->nnz[2] >> 32 || s->log_n > 28) return 2;
  return 0;
}
// the three matrices into caller-owned arrays of hb_sizes' sizes: row_ptr[k] n_constraints + 1, col[k] nnz[k], val[k] 4 nnz[k].
// Rows: epoch 0's, epoch 1's, ..., then one pack row per instance variable.
inline int hb_write_csr(size_t m, uint64_t* const row_ptr[3], uint32_t* const col[3], uint64_t* const val[3]) {
  HbSizes s;
  if (int rc = hb_sizes(m, &s)) return rc;
  for (int k = 0; k < 3; k++) if (!row_ptr[k] || !col[k] || !val[k]) return 2;
  const HbTemplate& T = hb_template();
  const uint32_t n_inputs = (uint32_t)s.n_inputs, stride = T.stride();
  for (int k = 0; k < 3; k++) {
    const HbTplMat& M = T.mat[k];
    const size_t tn = M.col.size();
    std::vector<uint64_t> tv(tn * 4);
    for (size_t i = 0; i < tn; i++) hb_coef_mont(M.coef[i], &tv[4 * i]);
    for (size_t e = 0; e < m; e++) {
      const uint64_t r0 = (uint64_t)e * T.rows, z0 = (uint64_t)e * tn;
      for (uint32_t j = 0; j < T.rows; j++) row_ptr[k][r0 + j] = z0 + M.row_ptr[j];
      for (size_t i = 0; i < tn; i++) col[k][z0 + i] = M.col[i] ? (uint32_t)(n_inputs + e * stride + M.col[i] - 1) : 0u;
      memcpy(val[k] + 4 * z0, tv.data(), tn * 32);
    }
    uint64_t at = (uint64_t)m * tn;
    const uint64_t r0 = (uint64_t)m * T.rows;
    for (uint32_t c = 0; c + 1 < n_inputs; c++) {
      row_ptr[k][r0 + c] = at;
      if (k == 0) {
        hb_pack_row(T, m, c, [&](uint32_t cc, uint32_t pow, bool neg) { col[0][at] = cc; hb_pow2_mont(pow, neg, val[0] + 4 * at); at++; },
                    [&](const uint64_t* k0) { col[0][at] = 0; hb_to_mont(k0, val[0] + 4 * at); at++; });
      } else if (k == 1) {
        col[1][at] = 0;
        memcpy(val[1] + 4 * at, HbFr::R, 32);
        at++;
      }
    }
    row_ptr[k][s.n_constraints] = at;
    if (at != s.nnz[k]) return 2;
  }
  return 0;
}

// ---- the host twin of the three kernels: trace (n_epochs x HB_TRACE_WORDS), the full assignment, the canonical instance rows
inline void hb_trace_host(const uint8_t* rows48, size_t n_epochs, int bit_order, uint32_t* trace) {
  for (size_t e = 0; e < n_epochs; e++)
    for (uint32_t comp = 0; comp < 2; comp++) hb_trace_lane(rows48 + e * HB_ROW_BYTES, bit_order, comp, trace + e * HB_TRACE_WORDS);
}
inline int hb_assignment_host(const uint8_t* rows48, size_t m, int bit_order, uint64_t* z) {
  HbSizes s;
  if (!rows48 || !z || bit_order < 0 || bit_order > 1) return 2;
  if (int rc = hb_sizes(m, &s)) return rc;
  const HbTemplate& T = hb_template();
  std::vector<uint32_t> trace(m * HB_TRACE_WORDS);
  hb_trace_host(rows48, m, bit_order, trace.data());
  memcpy(z, HbFr::R, 32);
  for (uint32_t c = 0; c + 1 < s.n_inputs; c++) {
    uint64_t v[4];
    hb_pack_chunk(trace.data(), m, c, v);
    hb_to_mont(v, z + 4 * (1 + c));
  }
  for (uint64_t i = s.n_inputs; i < s.n_vars; i++) {
    const bool bit = hb_var_bit(T.desc.data(), trace.data(), T.stride(), (uint32_t)s.n_inputs, (uint32_t)i);
    for (int j = 0; j < 4; j++) z[4 * i + j] = bit ? HbFr::R[j] : 0;
  }
  return 0;
}
// n_proofs x (n_inputs - 1) x 4 canonical limbs: proof p takes rows [p m, (p + 1) m)
inline int hb_public_inputs_host(const uint8_t* rows48, size_t n_proofs, size_t m, int bit_order, uint64_t* out) {
  HbSizes s;
  if (!rows48 || !out || bit_order < 0 || bit_order > 1) return 2;
  if (int rc = hb_sizes(m, &s)) return rc;
  std::vector<uint32_t> trace(m * HB_TRACE_WORDS);
  for (size_t p = 0; p < n_proofs; p++) {
    hb_trace_host(rows48 + p * m * HB_ROW_BYTES, m, bit_order, trace.data());
    for (uint32_t c = 0; c + 1 < s.n_inputs; c++) hb_pack_chunk(trace.data(), m, c, out + 4 * (p * (s.n_inputs - 1) + c));
  }
  return 0;
}

}  // namespace celo
