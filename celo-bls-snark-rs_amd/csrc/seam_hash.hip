// Seam A, the hashers (seam.h has the map of the units): Blake2s / Blake2Xs, the Bowe-Hopwood CRH and its generator table, hash-to-G1 for
// one message and for many, and the entry points built on one hash: hash_*, sign_*, verify_signature, verify_pop.
#include "hash_direct.h"
#include "pedersen.h"
#include "host64.h"
#include "seam.h"

using namespace celo;
using namespace celo::seam;

namespace {
// ---------------------------------------------------------------- DirectHasher (crates/bls-crypto/src/hashers/direct.rs:8-80)
// Blake2s (RFC 7693) with an explicit parameter block: the XOF uses fanout = depth = 0, leaf/inner length 32 and the
// BLAKE2X node-offset trick (xof length in bits 32..47 of the 48-bit node offset).  Host plumbing.
const uint32_t B2S_IV[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
const uint8_t B2S_SIGMA[10][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};
inline uint32_t rotr32(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
void b2s_compress(uint32_t h[8], const uint8_t block[64], uint64_t t, bool last) {
  uint32_t m[16], v[16];
  for (int i = 0; i < 16; i++) memcpy(&m[i], block + 4 * i, 4);
  for (int i = 0; i < 8; i++) { v[i] = h[i]; v[i + 8] = B2S_IV[i]; }
  v[12] ^= (uint32_t)t;
  v[13] ^= (uint32_t)(t >> 32);
  if (last) v[14] ^= 0xFFFFFFFFu;
#define B2S_G(a, b, c, d, x, y)                                   \
  v[a] = v[a] + v[b] + (x); v[d] = rotr32(v[d] ^ v[a], 16);       \
  v[c] = v[c] + v[d];       v[b] = rotr32(v[b] ^ v[c], 12);       \
  v[a] = v[a] + v[b] + (y); v[d] = rotr32(v[d] ^ v[a], 8);        \
  v[c] = v[c] + v[d];       v[b] = rotr32(v[b] ^ v[c], 7);
  for (int r = 0; r < 10; r++) {
    const uint8_t* s = B2S_SIGMA[r];
    B2S_G(0, 4, 8, 12, m[s[0]], m[s[1]]) B2S_G(1, 5, 9, 13, m[s[2]], m[s[3]])
    B2S_G(2, 6, 10, 14, m[s[4]], m[s[5]]) B2S_G(3, 7, 11, 15, m[s[6]], m[s[7]])
    B2S_G(0, 5, 10, 15, m[s[8]], m[s[9]]) B2S_G(1, 6, 11, 12, m[s[10]], m[s[11]])
    B2S_G(2, 7, 8, 13, m[s[12]], m[s[13]]) B2S_G(3, 4, 9, 14, m[s[14]], m[s[15]])
  }
#undef B2S_G
  for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[i + 8];
}
}  // namespace

namespace celo {
namespace seam {
std::vector<uint8_t> blake2s(const uint8_t* data, size_t len, const B2sParams& p, const uint8_t* personal, size_t plen) {
  uint8_t pb[32];
  memset(pb, 0, 32);
  pb[0] = p.digest_length; pb[1] = 0; pb[2] = p.fanout; pb[3] = p.depth;
  memcpy(pb + 4, &p.leaf_length, 4);
  for (int i = 0; i < 6; i++) pb[8 + i] = (uint8_t)(p.node_offset >> (8 * i));
  pb[14] = p.node_depth; pb[15] = p.inner_length;
  memcpy(pb + 24, personal, plen < 8 ? plen : 8);
  uint32_t h[8];
  for (int i = 0; i < 8; i++) { uint32_t w; memcpy(&w, pb + 4 * i, 4); h[i] = B2S_IV[i] ^ w; }
  uint64_t t = 0;
  size_t off = 0;
  // (::b2s_compress: the file-local function above - inside namespace celo the plain name finds hash_direct.h's celo::b2s_compress first)
  while (len - off > 64) { t += 64; ::b2s_compress(h, data + off, t, false); off += 64; }
  uint8_t lastb[64];
  memset(lastb, 0, 64);
  if (len - off) memcpy(lastb, data + off, len - off);
  t += len - off;
  ::b2s_compress(h, lastb, t, true);
  std::vector<uint8_t> out(p.digest_length);
  uint8_t full[32];
  memcpy(full, h, 32);
  memcpy(out.data(), full, p.digest_length);
  return out;
}
}  // namespace seam
}  // namespace celo

namespace {
uint64_t xof_node_offset(uint64_t i, size_t xof_len) { return i | ((uint64_t)(xof_len & 0xFF) << 32) | ((uint64_t)((xof_len >> 8) & 0xFF) << 40); }
std::vector<uint8_t> direct_crh(const uint8_t* dom, size_t dlen, const uint8_t* msg, size_t mlen, size_t xof_len) {
  B2sParams p;
  p.node_offset = xof_node_offset(0, xof_len);
  return blake2s(msg, mlen, p, dom, dlen);
}
std::vector<uint8_t> direct_xof(const uint8_t* dom, size_t dlen, const uint8_t* hashed, size_t hlen, size_t xof_len) {
  size_t n = (xof_len + 31) / 32;
  std::vector<uint8_t> out;
  for (size_t i = 0; i < n; i++) {
    B2sParams p;
    p.digest_length = (uint8_t)((i == n - 1 && (xof_len % 32)) ? xof_len % 32 : 32);
    p.fanout = 0; p.depth = 0; p.leaf_length = 32; p.inner_length = 32;
    p.node_offset = xof_node_offset(i, xof_len);
    std::vector<uint8_t> h = blake2s(hashed, hlen, p, dom, dlen);
    out.insert(out.end(), h.begin(), h.end());
  }
  return out;
}
std::vector<uint8_t> direct_hash(const uint8_t* dom, size_t dlen, const uint8_t* msg, size_t mlen, size_t n) {
  std::vector<uint8_t> c = direct_crh(dom, dlen, msg, mlen, n);
  return direct_xof(dom, dlen, c.data(), c.size(), n);
}
// TryAndIncrement<DirectHasher, G1>::hash_with_attempt with the deployed `compat` bit logic
// (crates/bls-crypto/src/hash_to_curve/try_and_increment.rs:87-139, mod.rs:146-158)
bool hash_to_g1_direct(const uint8_t* dom, const uint8_t* msg, size_t mlen, const uint8_t* extra, size_t elen, Affine<Fq_>& out, int& attempt) {
  return hash_to_g1_direct_tai(dom, msg, mlen, extra, elen, wire_consts(), out, attempt);   // hash_direct.h: the source the GPU kernels run
}

// ---------------------------------------------------------------- CompositeHasher (crates/bls-crypto/src/hashers/composite.rs)
// Bowe-Hopwood-Pedersen CRH over the twisted Edwards curve ed-on-BW6-761 (-x^2 + y^2 = 1 + 79743 x^2 y^2 over Fq of
// BLS12-377), WINDOW_SIZE = 93, NUM_WINDOWS = 560, generators drawn from ChaCha20 seeded with
// Blake2s("ULTRALIGHT PRNG SEED", personal "UL_prngs") exactly as rand 0.7 / rand_chacha 0.2 / ark-ff 0.1 consume it, then
// the Blake2Xs XOF.  Host plumbing; pinned on the reference's CRH vector and its 20 compat hash-to-G1
// vectors through the oracle restatement (tests/test_oracle_golden.py, tests/test_seam_a.py).
bool fq_sqrt(const Fq_& a, Fq_& out) { return wire_fq_sqrt(a, wire_consts(), out); }
struct CompositeParams {
  std::vector<EdPoint> gens;  // [NUM_WINDOWS * WINDOW_SIZE][PEDERSEN_MULTIPLES]: window-major, generator j = 16^j * base, then its multiples 1..4
  static constexpr int WINDOW_SIZE = PEDERSEN_WINDOW_SIZE, NUM_WINDOWS = PEDERSEN_NUM_WINDOWS;
  CompositeParams() {
    static const uint8_t PERS[8] = {'U', 'L', '_', 'p', 'r', 'n', 'g', 's'};
    static const char* SEED_MSG = "ULTRALIGHT PRNG SEED";
    B2sParams p;
    std::vector<uint8_t> seed = blake2s((const uint8_t*)SEED_MSG, strlen(SEED_MSG), p, PERS, 8);
    ChaCha20Rng rng;
    memcpy(rng.key, seed.data(), 32);
    const SF one = sf_small(1), dcoef = sf_small(79743);
    gens.reserve((size_t)WINDOW_SIZE * NUM_WINDOWS * PEDERSEN_MULTIPLES);
    for (int w = 0; w < NUM_WINDOWS; w++) {
      EdPoint base;
      for (;;) {  // TEProjective::rand: x = Fq::rand (raw Montgomery limbs, top 7 bits masked, rejection), greatest = rng.gen::<bool>()
        uint64_t raw[6];
        for (;;) {
          for (int i = 0; i < 6; i++) raw[i] = rng.next_u64();
          raw[5] &= (1ULL << 57) - 1;
          if (wire_cmp(raw, P377::P64, 6) < 0) break;
        }
        bool greatest = (rng.next_u32() >> 31) != 0;
        SF x = SF::from(Fq_::from_ark(raw));
        SF x2 = x * x;
        SF num = x2.neg() - one, den = dcoef * x2 - one;      // (a x^2 - 1) / (d x^2 - 1), a = -1
        if (den.v.is_zero_mod_p()) continue;
        SF y2 = num * SF::from(Fq_::inv(den.v));
        Fq_ yv;
        if (!fq_sqrt(y2.v, yv)) continue;
        if (wire_lex_largest(yv) != greatest) yv = wire_neg(yv);   // (y < -y) ^ greatest ? y : -y
        SF y = SF::from(yv);
        base = {x, y, one, x * y};
        for (int k = 0; k < 3; k++) base = ed_dbl(base);       // scale_by_cofactor (8)
        break;
      }
      for (int j = 0; j < WINDOW_SIZE; j++) {
        const EdPoint g2 = ed_dbl(base), g4 = ed_dbl(g2);
        gens.push_back(base); gens.push_back(g2); gens.push_back(ed_add(g2, base)); gens.push_back(g4);   // (1 + b0 + 2 b1) g for the chunk's two low bits
        base = ed_dbl(ed_dbl(g4));                                                                          // 16 g
      }
    }
  }
};
const CompositeParams& composite_params() { static CompositeParams p; return p; }
// The HOST evaluation of ONE message's CRH (round 6; VERDICT r5 item 5: the single-caller path - verify_signature, hash_composite*, hash_crh -
// spent more than half of a call here).  pedersen.h is one host+device source on the device's 28-bit limbs: right for the bulk GPU kernel, ~1.4 us
// per Edwards addition on a host core.  Here the same sum runs on 64-bit limbs (host64.h: arkworks' own Montgomery form, 6 x 6 CIOS) against a
// table of AFFINE entries precomputed for the mixed addition - (y - x, y + x, 2 d x y) per multiple, so an addition is 7 products (madd-2008-hwcd-3)
// and a negated entry is a swap and one negation: ~0.3 us per chunk.  Same group element, so the same 48 bytes (the reference's CRH vector and
// its 20 compat hash-to-G1 points pin both paths: tests/test_seam_a.py, tests/test_hash_gpu.py).  The table is derived from CompositeParams::gens
// (one batched inversion) window by window on first use: messages of the FFI's shapes touch the first two or three of the 560 windows.
struct CompositeHostTable {
  typedef HFp<P377> H;
  struct Entry { H ymx, ypx, t2d; };
  static constexpr size_t PER_WINDOW = (size_t)PEDERSEN_WINDOW_SIZE * PEDERSEN_MULTIPLES;
  std::vector<Entry> tab;
  std::vector<std::atomic<int>> ready;       // per window: 0 = not built, 2 = built (1 = being built: the builder holds `mu`)
  std::mutex mu;
  H two_d, raw_one;
  CompositeHostTable() : tab(PER_WINDOW * PEDERSEN_NUM_WINDOWS), ready(PEDERSEN_NUM_WINDOWS) {
    for (auto& r : ready) r.store(0);
    uint64_t w[6];
    sf_small(2 * 79743).v.to_ark(w);
    two_d = H::load(w);
    memset(raw_one.v, 0, sizeof raw_one.v);
    raw_one.v[0] = 1;                           // a * raw_one = a R^-1: Montgomery form -> the plain integer
  }
  static H from_sf(const SF& a) { uint64_t w[6]; a.v.to_ark(w); return H::load(w); }
  static H inv(const H& a) {                   // a^(p - 2), square-and-multiply from the top: one per built window and one per message
    uint64_t e[6];
    memcpy(e, P377::P64, sizeof e);
    e[0] -= 2;                                  // (p is odd and its low limb is far from 0: no borrow)
    H r = H::one();
    bool started = false;
    for (int i = 6 * 64 - 1; i >= 0; i--) {
      if (started) r = r.sqr();
      if ((e[i >> 6] >> (i & 63)) & 1) { r = started ? r * a : a; started = true; }
    }
    return r;
  }
  void build(int w) {
    std::lock_guard<std::mutex> lk(mu);
    if (ready[(size_t)w].load(std::memory_order_acquire) == 2) return;
    const EdPoint* g = composite_params().gens.data() + (size_t)w * PER_WINDOW;
    std::vector<H> z(PER_WINDOW), pre(PER_WINDOW);
    H acc = H::one();
    for (size_t i = 0; i < PER_WINDOW; i++) { z[i] = from_sf(g[i].Z); pre[i] = acc; acc = acc * z[i]; }
    H iv = inv(acc);
    for (size_t i = PER_WINDOW; i-- > 0;) {
      const H zi = iv * pre[i];
      iv = iv * z[i];
      const H x = from_sf(g[i].X) * zi, y = from_sf(g[i].Y) * zi;
      tab[(size_t)w * PER_WINDOW + i] = {y - x, y + x, x * y * two_d};
    }
    ready[(size_t)w].store(2, std::memory_order_release);
  }
  void eval(const uint8_t* msg, size_t len, uint8_t out48[48]) {
    const size_t nbits = len * 8, nchunks = (nbits + 2) / 3;
    for (size_t w = 0; w * PEDERSEN_WINDOW_SIZE < nchunks; w++)
      if (ready[w].load(std::memory_order_acquire) != 2) build((int)w);
    H X = H::zero(), Y = H::one(), Z = H::one(), T = H::zero();
    for (size_t ch = 0; ch < nchunks; ch++) {
      const size_t b = 3 * ch;
      uint32_t two = msg[b >> 3];
      if ((b >> 3) + 1 < len) two |= (uint32_t)msg[(b >> 3) + 1] << 8;
      const uint32_t bits = (two >> (b & 7)) & 7u;
      const Entry& e = tab[(size_t)PEDERSEN_MULTIPLES * ch + (bits & 3u)];
      const bool ng = (bits & 4) != 0;           // -(x, y) = (-x, y): the two sums swap, the T term changes sign
      const H A = (Y - X) * (ng ? e.ypx : e.ymx), B = (Y + X) * (ng ? e.ymx : e.ypx), Ct = T * e.t2d, D = Z.dbl();
      const H C = ng ? H::zero() - Ct : Ct;
      const H E = B - A, F = D - C, G = D + C, Hh = B + A;
      X = E * F; Y = G * Hh; Z = F * G; T = E * Hh;
    }
    // x = X / Z as a plain integer: Z out of Montgomery form, inverted by division steps (modinv.h works on plain 64-bit limbs: a few us on a
    // host core, where Fermat's 570 products were half of a 64-byte message's time), and X_mont * (1 / Z)_plain = (X / Z)_plain
    const H zc = Z * raw_one;
    H zi;
    SafeGcd<P377>::inv(zc.v, zi.v);
    const H x = X * zi;
    for (int i = 0; i < 48; i++) out48[i] = (uint8_t)(x.v[i >> 3] >> (8 * (i & 7)));
  }
  static CompositeHostTable& get() { static CompositeHostTable* t = new CompositeHostTable; return *t; }
};
bool composite_crh(const uint8_t* msg, size_t len, std::vector<uint8_t>& out) {  // bowe_hopwood::CRH::evaluate -> affine x, 48 bytes
  if (len * 8 > PEDERSEN_MAX_BITS) return false;  // the reference panics
  out.assign(48, 0);
  static const bool slow = getenv("CELO_CRH_DEVICE_LIMBS") != nullptr;      // A/B and cross-check switch: pedersen.h's source on the host, as rounds 2-5 ran it
  if (slow) pedersen_crh(composite_params().gens.data(), msg, len, out.data());
  else CompositeHostTable::get().eval(msg, len, out.data());
  return true;
}
// scale_by_cofactor + affine normalisation of hash_direct.h's tai_finish on the host's 64-bit limbs (host64.h): 124 doublings and 17 additions
// are ~1 700 products - 0.3 ms of every single hash on the device's 28-bit limbs, a third of that here.  Same group element.
static bool tai_finish_host64(const Affine<Fq_>& p, Affine<Fq_>& out) {
  typedef HFp<P377> H;
  const uint64_t cof[2] = {0x0000000000000000ULL, 0x170b5d4430000000ULL};   // (x - 1)^2 / 3, 125 bits, bit 124 set
  uint64_t w[6];
  HXyzz<H> base;
  p.x.to_ark(w); base.X = H::load(w);
  p.y.to_ark(w); base.Y = H::load(w);
  base.ZZ = H::one(); base.ZZZ = H::one();
  HXyzz<H> s = base;
  for (int i = 123; i >= 0; i--) {
    s = hxyzz_dbl(s);
    if ((cof[i >> 6] >> (i & 63)) & 1) hxyzz_add(s, base);
  }
  if (s.is_identity()) return false;
  H raw_one;
  memset(raw_one.v, 0, sizeof raw_one.v);
  raw_one.v[0] = 1;
  const H zc = (s.ZZ * s.ZZZ) * raw_one;     // plain integer
  H t;
  SafeGcd<P377>::inv(zc.v, t.v);             // 1 / (ZZ ZZZ) as a plain integer: (a_mont * b_plain) is a b plain, times c_mont is a b c plain
  const H x = (s.X * t) * s.ZZZ, y = (s.Y * t) * s.ZZ;
  out.x = Fq_::norm(Fq_::from_canonical(x.v));
  out.y = Fq_::norm(Fq_::from_canonical(y.v));
  return true;
}

}  // namespace

namespace celo {
namespace seam {
// generic try-and-increment over {direct, composite} x {plain, cip22} with the `compat` bit logic
// pre_cofactor (optional): the curve point BEFORE scale_by_cofactor (from_random_bytes' point), for the callers that restate arkworks' own multiple
bool hash_to_g1(bool composite, bool cip22, const uint8_t* dom, const uint8_t* msg, size_t mlen, const uint8_t* extra, size_t elen,
                Affine<Fq_>& out, int& attempt, Affine<Fq_>* pre_cofactor) {
  auto crh = [&](const uint8_t* m, size_t l, std::vector<uint8_t>& o) -> bool {
    if (composite) return composite_crh(m, l, o);
    o = direct_crh(dom, 8, m, l, 64);
    return true;
  };
  std::vector<uint8_t> inner, buf, pre;
  if (cip22 && !crh(msg, mlen, inner)) return false;
  const uint8_t* tail = cip22 ? inner.data() : msg;
  const size_t tlen = cip22 ? inner.size() : mlen;
  buf.resize(1 + elen + tlen);
  if (elen) memcpy(buf.data() + 1, extra, elen);
  if (tlen) memcpy(buf.data() + 1 + elen, tail, tlen);
  for (int c = 0; c < 255; c++) {
    buf[0] = (uint8_t)c;
    std::vector<uint8_t> cand;
    if (cip22) cand = direct_xof(dom, 8, buf.data(), buf.size(), 64);
    else { if (!crh(buf.data(), buf.size(), pre)) return false; cand = direct_xof(dom, 8, pre.data(), pre.size(), 64); }
    uint32_t w12[12];
    memcpy(w12, cand.data(), 48);
    Affine<Fq_> p = {Fq_::zero(), Fq_::zero()};
    if (!tai_point_from_xof(w12, wire_consts(), p)) continue;            // hash_direct.h: compat flags, get_point_from_x
    if (!tai_finish_host64(p, out)) continue;                            // scale_by_cofactor
    attempt = c;
    if (pre_cofactor) *pre_cofactor = p;
    return true;
  }
  return false;
}

// hash many messages on all host cores (hash-to-curve is host plumbing for now; one attempt costs a
// Blake2Xs call, a 377-bit square root and a 125-bit cofactor multiplication)
// failed (optional, one flag per job): a message that cannot be hashed marks its own job and the call goes on (the caller
// decides what one bad message means); without it the first failure fails the call.
bool hash_many(bool composite, bool cip22, const uint8_t* dom, std::vector<HashJob>& jobs, std::vector<uint8_t>* failed) {
  (void)wire_consts();
  if (failed) failed->assign(jobs.size(), 0);
  bool gpu_done = false;
  // many messages: hashing runs on the GPU (a lone wave of 64 needs ~4 ms, so the host cores keep the small calls), for
  // every hasher: hash_direct.h's try-and-increment rounds over the Blake2s CRH, over precomputed Pedersen CRHs (CIP22), or
  // with a Pedersen CRH per attempt (composite before CIP22)
  if (jobs.size() >= 256) {
    const size_t n = jobs.size();
    std::vector<uint64_t> moff(n + 1, 0), eoff(n + 1, 0);
    for (size_t i = 0; i < n; i++) { moff[i + 1] = moff[i] + jobs[i].mlen; eoff[i + 1] = eoff[i] + jobs[i].elen; }
    std::vector<uint8_t> mb(moff[n] + 1), eb(eoff[n] + 1), att(n);
    for (size_t i = 0; i < n; i++) {
      if (jobs[i].mlen) memcpy(&mb[moff[i]], jobs[i].msg, jobs[i].mlen);
      if (jobs[i].elen) memcpy(&eb[eoff[i]], jobs[i].extra, jobs[i].elen);
    }
    std::vector<uint64_t> xy(n * 12);
    const int rc = composite ? hash_to_g1_composite_bls12_377(dom, mb.data(), moff.data(), eb.data(), eoff.data(), n, cip22 ? 1 : 0, xy.data(), att.data())
                             : hash_to_g1_direct_bls12_377(dom, mb.data(), moff.data(), eb.data(), eoff.data(), n, xy.data(), att.data());
    if (rc != 0 && !failed) return false;
    if (rc == 0) {
      for (size_t i = 0; i < n; i++) {
        if (att[i] == 255) { if (!failed) return false; (*failed)[i] = 1; continue; }
        memcpy(jobs[i].out_xy, &xy[i * 12], 96);
      }
      gpu_done = true;
    }
    // rc != 0 with per-job flags wanted (e.g. ONE oversized composite message): the host loop below sorts out which
  }
  if (gpu_done) return true;
  if (composite) (void)composite_params();  // initialise shared constants before the threads start
  std::atomic<size_t> next(0);
  std::atomic<bool> ok(true);
  unsigned nt = std::thread::hardware_concurrency();
  if (nt == 0) nt = 1;
  if (nt > 64) nt = 64;
  if (nt > jobs.size() / 4 + 1) nt = (unsigned)(jobs.size() / 4 + 1);    // at least ~4 hashes (~1 ms) per thread
  run_on_threads(nt, [&](unsigned) {
    for (;;) {
      size_t i = next.fetch_add(1);
      if (i >= jobs.size()) break;
      Affine<Fq_> h; int c;
      if (!hash_to_g1(composite, cip22, dom, jobs[i].msg, jobs[i].mlen, jobs[i].extra, jobs[i].elen, h, c)) {
        if (failed) (*failed)[i] = 1; else ok = false;
        continue;
      }
      h.x.to_ark(jobs[i].out_xy); h.y.to_ark(jobs[i].out_xy + 6);
    }
  });
  return ok;
}
void neg_g2_generator(uint64_t out_xy[24]) {
  Fq_::from_limbs(T377::G2_GEN_X0).to_ark(out_xy);
  Fq_::from_limbs(T377::G2_GEN_X1).to_ark(out_xy + 6);
  wire_neg(Fq_::from_limbs(T377::G2_GEN_Y0)).to_ark(out_xy + 12);
  wire_neg(Fq_::from_limbs(T377::G2_GEN_Y1)).to_ark(out_xy + 18);
}
}  // namespace seam

// the composite hasher's generator table for the bulk GPU kernel (unit_hash.hip: k_pedersen_crh)
const EdPoint* celo_composite_gens(size_t* count) {
  const CompositeParams& cp = composite_params();
  *count = cp.gens.size();
  return cp.gens.data();
}
}  // namespace celo

extern "C" {

// ---------------------------------------------------------------- GPU verification cores (the part of verify_* after hashing)
// message_hash_xy: H(m) as an affine G1 point in arkworks limbs (12 u64) — what hash_to_g1.hash(..) returns in
// PublicKey::verify_sig (crates/bls-crypto/src/bls/public.rs:108) after into_affine().
bool celo_amd_g2_generator(uint64_t out_xy[24]) {
  Fq_::from_limbs(T377::G2_GEN_X0).to_ark(out_xy);
  Fq_::from_limbs(T377::G2_GEN_X1).to_ark(out_xy + 6);
  Fq_::from_limbs(T377::G2_GEN_Y0).to_ark(out_xy + 12);
  Fq_::from_limbs(T377::G2_GEN_Y1).to_ark(out_xy + 18);
  return true;
}
bool celo_amd_verify_hash(const PublicKey* pk, const uint64_t* message_hash_xy, const Signature* sig, bool* out_verified) {
  if (!pk || !message_hash_xy || !sig || !out_verified) return false;
  PhaseLog ph("verify_hash");
  Affine<Fq_> s;
  Affine<Fq2_> p;
  uint8_t inf1[2] = {0, 0}, inf2[2] = {0, 0};
  uint64_t g1[24], g2[48];
  memset(g1, 0, sizeof g1);
  memset(g2, 0, sizeof g2);
  if (jac_to_affine<Fq_>(sig->xyz, s)) { s.x.to_ark(g1); s.y.to_ark(g1 + 6); } else inf1[0] = 1;
  memcpy(g1 + 12, message_hash_xy, 96);
  neg_g2_generator(g2);
  if (jac_to_affine<Fq2_>(pk->xyz, p)) { p.x.to_ark(g2 + 24); p.y.to_ark(g2 + 36); } else inf2[1] = 1;
  ph.mark("handles -> affine pairs (host)");
  int one = 0;
  if (pairing_product_is_one_bls12_377(g1, inf1, g2, inf2, 2, &one) != 0) return false;
  ph.mark("2-pair product check (GPU, latency path)");
  *out_verified = one != 0;
  return true;
}

// ---------------------------------------------------------------- hashing / signing: the direct hasher, then the composite one
static bool emit_affine_tobytes(const Affine<Fq_>& p, uint8_t** out, int* out_len) {  // ToBytes: x || y || infinity byte
  std::vector<uint8_t> v(97, 0);
  fq_to_bytes(p.x, v.data());
  fq_to_bytes(p.y, v.data() + 48);
  return emit(v, out, out_len);
}
bool hash_direct(const uint8_t* msg, int len, uint8_t** out_hash, int* out_len, bool use_pop) {                /* signatures.rs:93 */
  if ((!msg && len) || !out_hash || !out_len || len < 0) return false;
  Affine<Fq_> h; int c;
  if (!hash_to_g1_direct(use_pop ? POP_DOMAIN : SIG_DOMAIN, msg, (size_t)len, nullptr, 0, h, c)) return false;
  return emit_affine_tobytes(h, out_hash, out_len);
}
bool hash_direct_with_attempt(const uint8_t* msg, int len, uint8_t** out_hash, int* out_len, int* out_attempt, bool use_pop) { /* :117 */
  if ((!msg && len) || !out_hash || !out_len || !out_attempt || len < 0) return false;
  Affine<Fq_> h; int c;
  if (!hash_to_g1_direct(use_pop ? POP_DOMAIN : SIG_DOMAIN, msg, (size_t)len, nullptr, 0, h, c)) return false;
  *out_attempt = c;
  return emit_affine_tobytes(h, out_hash, out_len);
}
bool hash_direct_first_step(const uint8_t* msg, int len, int hash_bytes, uint8_t** out_hash, int* out_len) {    /* signatures.rs:192 */
  if ((!msg && len) || !out_hash || !out_len || len < 0 || hash_bytes < 0 || hash_bytes > 65535) return false;
  return emit(direct_hash(SIG_DOMAIN, 8, msg, (size_t)len, (size_t)hash_bytes), out_hash, out_len);
}
// hash_composite / hash_composite_cip22 return ToBytes of a G1Projective (x || y || z, 144 bytes): the Jacobian representative that
// arkworks' scale_by_cofactor leaves (crates/bls-crypto/src/hash_to_curve/try_and_increment.rs:130, try_and_increment_cip22.rs:125 return
// `scaled` as it is, signatures.rs:143,215 write it).  Round 5 restates that schedule so that the BYTES agree and not only
// the point: GroupAffine::mul_bits over BitIteratorBE(COFACTOR) - res = zero; per bit, MSB first: res.double_in_place(); if bit:
// res.add_assign_mixed(p) - with ark-ec's a = 0 doubling (dbl-2009-l) and mixed addition (madd-2007-bl) on GroupProjective (SURVEY.md
// Appendix B.6; pinned revision arkworks-rs/algebra@8d76d181, source not on disk: restated from the published formulas).  The formulas are
// exact arithmetic mod q, so the representative is a function of (p, COFACTOR) alone; it is computed here on 64-bit Montgomery limbs
// (host64.h).  No reference vector pins these 144 bytes: tests check that into_affine() of them is the hash point the
// compat vectors pin, and the schedule against an independent big-integer restatement (oracle/py).
static void ark_scale_by_cofactor_tobytes(const Affine<Fq_>& p, uint8_t out[144]) {
  typedef HFp<P377> H;
  uint64_t w[6];
  p.x.to_ark(w); const H px = H::load(w);
  p.y.to_ark(w); const H py = H::load(w);
  H X = H::zero(), Y = H::one(), Z = H::zero();                          // GroupProjective::zero() = (0, 1, 0)
  const uint64_t cof[2] = {0x0000000000000000ULL, 0x170b5d4430000000ULL};  // G1 COFACTOR (ark-bls12-377 g1.rs), little-endian limbs
  auto dbl = [&]() {
    if (Z.is_zero()) return;
    const H a = X.sqr(), b = Y.sqr(), c = b.sqr();
    const H d = ((X + b).sqr() - a - c).dbl();
    const H e = a + a.dbl(), f = e.sqr();
    Z = (Z * Y).dbl();
    X = f - d - d;
    Y = (d - X) * e - c.dbl().dbl().dbl();
  };
  auto madd = [&]() {
    if (Z.is_zero()) { X = px; Y = py; Z = H::one(); return; }
    const H z1z1 = Z.sqr(), u2 = px * z1z1, s2 = (py * Z) * z1z1;
    if (memcmp(X.v, u2.v, sizeof X.v) == 0 && memcmp(Y.v, s2.v, sizeof Y.v) == 0) { dbl(); return; }
    const H h = u2 - X, hh = h.sqr(), i = hh.dbl().dbl();
    H j = h * i;
    const H r = (s2 - Y).dbl(), v = X * i;
    X = r.sqr() - j - v - v;
    j = (j * Y).dbl();
    Y = (v - X) * r - j;
    Z = (Z + h).sqr() - z1z1 - hh;
  };
  for (int i = 127; i >= 0; i--) {
    dbl();
    if ((cof[i >> 6] >> (i & 63)) & 1) madd();
  }
  uint64_t raw1[6] = {1, 0, 0, 0, 0, 0};
  const H unmont = H::load(raw1);                                        // x * (1 as a raw residue) = x R^-1: out of Montgomery form
  const H c[3] = {X * unmont, Y * unmont, Z * unmont};
  for (int k = 0; k < 3; k++) memcpy(out + 48 * k, c[k].v, 48);
}
static bool emit_projective_tobytes(const Affine<Fq_>& pre, uint8_t** out, int* out_len) {
  std::vector<uint8_t> v(144, 0);
  ark_scale_by_cofactor_tobytes(pre, v.data());
  return emit(v, out, out_len);
}
bool hash_composite(const uint8_t* msg, int mlen, const uint8_t* extra, int elen, uint8_t** out_hash, int* out_len) {   /* signatures.rs:143 */
  if ((!msg && mlen) || (!extra && elen) || !out_hash || !out_len || mlen < 0 || elen < 0) return false;
  Affine<Fq_> h, pre; int c;
  if (!hash_to_g1(true, false, SIG_DOMAIN, msg, (size_t)mlen, extra, (size_t)elen, h, c, &pre)) return false;
  return emit_projective_tobytes(pre, out_hash, out_len);
}
bool hash_composite_cip22(const uint8_t* msg, int mlen, const uint8_t* extra, int elen, uint8_t** out_hash, int* out_len,
                          uint8_t* attempt_counter) {                                                                   /* signatures.rs:215 */
  if ((!msg && mlen) || (!extra && elen) || !out_hash || !out_len || !attempt_counter || mlen < 0 || elen < 0) return false;
  Affine<Fq_> h, pre; int c;
  if (!hash_to_g1(true, true, SIG_DOMAIN, msg, (size_t)mlen, extra, (size_t)elen, h, c, &pre)) return false;
  *attempt_counter = (uint8_t)c;
  return emit_projective_tobytes(pre, out_hash, out_len);
}
bool hash_crh(const uint8_t* msg, int mlen, int hash_bytes, uint8_t** out_hash, int* out_len) {                         /* signatures.rs:169 */
  (void)hash_bytes;  // the Bowe-Hopwood CRH ignores the domain and the output length (composite.rs:79-86)
  if ((!msg && mlen) || !out_hash || !out_len || mlen < 0) return false;
  std::vector<uint8_t> o;
  if (!composite_crh(msg, (size_t)mlen, o)) return false;
  return emit(o, out_hash, out_len);
}
/* test hook: DirectHasher with an arbitrary domain (<= 8 bytes, may be empty).  what: 0 = crh (32 bytes), 1 = xof of `msg`,
   2 = hash = xof(domain, crh(domain, msg))  (hashers/direct.rs:20-78) */
bool celo_amd_direct_hasher(int what, const uint8_t* domain, int dlen, const uint8_t* msg, int mlen, int out_bytes, uint8_t* out) {
  if (!out || dlen < 0 || dlen > 8 || mlen < 0 || out_bytes < 0 || (!domain && dlen) || (!msg && mlen)) return false;
  std::vector<uint8_t> r = what == 0 ? direct_crh(domain, (size_t)dlen, msg, (size_t)mlen, (size_t)out_bytes)
                         : what == 1 ? direct_xof(domain, (size_t)dlen, msg, (size_t)mlen, (size_t)out_bytes)
                                     : direct_hash(domain, (size_t)dlen, msg, (size_t)mlen, (size_t)out_bytes);
  memcpy(out, r.data(), r.size());
  return true;
}
/* test hook: CompositeHasher::hash = xof(domain, crh(message), out_bytes) (hashers/mod.rs Hasher::hash) */
bool celo_amd_composite_hash(const uint8_t* domain8, const uint8_t* msg, int mlen, int out_bytes, uint8_t* out) {
  if (!domain8 || !out || mlen < 0 || out_bytes < 0) return false;
  std::vector<uint8_t> c;
  if (!composite_crh(msg, (size_t)mlen, c)) return false;
  std::vector<uint8_t> x = direct_xof(domain8, 8, c.data(), c.size(), (size_t)out_bytes);
  memcpy(out, x.data(), (size_t)out_bytes);
  return true;
}
/* test hook: hash-to-G1 with an arbitrary 8-byte domain (the reference's golden vectors use random domains), compressed 48-byte output */
bool celo_amd_hash_to_g1(bool composite, bool cip22, const uint8_t* domain8, const uint8_t* msg, int mlen, const uint8_t* extra, int elen,
                         uint8_t* out48, int* out_attempt) {
  if (!domain8 || !out48 || mlen < 0 || elen < 0 || (!composite && cip22)) return false;
  Affine<Fq_> h; int c;
  if (!hash_to_g1(composite, cip22, domain8, msg, (size_t)mlen, extra, (size_t)elen, h, c)) return false;
  g1_compress(h, false, out48);
  if (out_attempt) *out_attempt = c;
  return true;
}
static bool sign_with(const PrivateKey* sk, bool composite, bool cip22, const uint8_t* dom, const uint8_t* msg, int mlen, const uint8_t* extra,
                      int elen, Signature** out) {
  if (!sk || !out || mlen < 0 || elen < 0) return false;
  Affine<Fq_> h; int c;
  if (!hash_to_g1(composite, cip22, dom, msg, (size_t)mlen, extra, (size_t)elen, h, c)) return false;
  Xyzz<Fq_> r = scalar_mul_host(h, sk->k, 4);                 // PrivateKey::sign_raw (crates/bls-crypto/src/bls/secret.rs:65)
  Signature* s = new_signature();
  if (!s) return false;
  if (r.is_identity() || r.ZZ.is_zero_mod_p()) identity_jac<Fq_>(s->xyz);
  else { Fq_::mul(r.X, r.ZZ).to_ark(s->xyz); Fq_::mul(r.Y, r.ZZZ).to_ark(s->xyz + 6); r.ZZ.to_ark(s->xyz + 12); }
  *out = s;
  return true;
}
bool sign_message(const PrivateKey* sk, const uint8_t* msg, int mlen, const uint8_t* extra, int elen, bool composite, bool cip22,
                  Signature** out) {                                                                                  /* signatures.rs:44 */
  if (!hash_flags_supported(composite, cip22)) return false;
  return sign_with(sk, composite, cip22, SIG_DOMAIN, msg, mlen, extra, elen, out);
}
bool sign_pop(const PrivateKey* sk, const uint8_t* msg, int mlen, Signature** out) {                                  /* signatures.rs:74 */
  return sign_with(sk, false, false, POP_DOMAIN, msg, mlen, nullptr, 0, out);
}

// ---------------------------------------------------------------- verification (hash on the host, pairings / MSMs on the GPU)
static bool verify_with(const PublicKey* pk, bool composite, bool cip22, const uint8_t* dom, const uint8_t* msg, int mlen, const uint8_t* extra,
                        int elen, const Signature* sig, bool* out_verified) {
  if (!pk || !sig || !out_verified || mlen < 0 || elen < 0) return false;
  PhaseLog ph("verify_with");
  Affine<Fq_> h; int c;
  if (!hash_to_g1(composite, cip22, dom, msg, (size_t)mlen, extra, (size_t)elen, h, c)) return false;
  uint64_t hxy[12];
  h.x.to_ark(hxy); h.y.to_ark(hxy + 6);
  ph.mark("message -> G1 (host)");
  return celo_amd_verify_hash(pk, hxy, sig, out_verified);
}
bool verify_signature(const PublicKey* pk, const uint8_t* msg, int mlen, const uint8_t* extra, int elen, const Signature* sig,
                      bool composite, bool cip22, bool* out_verified) {                                               /* signatures.rs:244 */
  if (!hash_flags_supported(composite, cip22)) return false;
  return verify_with(pk, composite, cip22, SIG_DOMAIN, msg, mlen, extra, elen, sig, out_verified);
}
bool verify_pop(const PublicKey* pk, const uint8_t* msg, int mlen, const Signature* sig, bool* out_verified) {        /* signatures.rs:407 */
  return verify_with(pk, false, false, POP_DOMAIN, msg, mlen, nullptr, 0, sig, out_verified);
}
}
