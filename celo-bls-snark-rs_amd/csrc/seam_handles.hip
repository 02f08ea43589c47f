// Seam A, the handles (seam.h has the map of the units): the arenas behind PublicKey / Signature, key generation, the arkworks wire
// encodings, destructors, aggregate_* and init.
#include <list>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include "seam.h"

using namespace celo;
using namespace celo::seam;

namespace {
// Chunked slab with a free list.  A handle's address never moves (chunks are never reallocated or released), its contents are written
// once, by the entry point that creates it, before the caller sees it; release() puts the slot back and the next alloc() of that slot
// carries a new serial, which is what marks the device mirrors' copy of the slot stale.  Serials are 64-bit and never 0.
template <class T> struct HandleArena {
  static constexpr uint32_t CHUNK = 1u << 14;
  std::mutex mu;
  std::vector<T*> chunks;
  std::vector<uint32_t> free_slots;
  uint32_t next = 0;
  uint64_t serial = 0;
  T* alloc() {
    std::lock_guard<std::mutex> lk(mu);
    uint32_t s;
    if (!free_slots.empty()) { s = free_slots.back(); free_slots.pop_back(); }
    else {
      if (next == 0xffffffffu) return nullptr;
      if ((size_t)next == chunks.size() * CHUNK) {
        T* c = (T*)malloc((size_t)CHUNK * sizeof(T));
        if (!c) return nullptr;
        try { chunks.push_back(c); } catch (...) { free(c); return nullptr; }
      }
      s = next++;
    }
    T* p = &chunks[s / CHUNK][s % CHUNK];
    p->slot = s;
    p->serial = ++serial;
    return p;
  }
  bool release(T* p) {
    std::lock_guard<std::mutex> lk(mu);
    if (p->serial == 0) return false;                           // destroyed already: the slot must not enter the free list twice
    p->serial = 0;
    try { free_slots.push_back(p->slot); } catch (...) {}       // out of memory: the slot is lost, nothing else
    return true;
  }
  uint32_t high_water() { std::lock_guard<std::mutex> lk(mu); return next; }
};
HandleArena<PublicKey>& pk_arena() { static HandleArena<PublicKey> a; return a; }
HandleArena<Signature>& sig_arena() { static HandleArena<Signature> a; return a; }
uint8_t* alloc_bytes(size_t n) { return (uint8_t*)malloc(n ? n : 1); }
}  // namespace

namespace celo {
namespace seam {
PublicKey* new_public_key() { return pk_arena().alloc(); }
Signature* new_signature() { return sig_arena().alloc(); }
bool drop(PublicKey* p) { return pk_arena().release(p); }
bool drop(Signature* p) { return sig_arena().release(p); }
uint32_t public_key_high_water() { return pk_arena().high_water(); }
uint32_t signature_high_water() { return sig_arena().high_water(); }
bool emit(const std::vector<uint8_t>& v, uint8_t** out_bytes, int* out_len) {
  uint8_t* p = alloc_bytes(v.size());
  if (!p) return false;
  memcpy(p, v.data(), v.size());
  *out_bytes = p;
  *out_len = (int)v.size();
  return true;
}
// ---- G1 (48-byte x, flags in the top two bits of the last byte)
bool g1_decompress(const uint8_t* in, Affine<Fq_>& p, bool& inf) {
  const WireStatus st = wire_decode_g1(in, wire_consts(), false, p);
  inf = st == WIRE_INFINITY;
  return st != WIRE_INVALID;
}
void g1_compress(const Affine<Fq_>& p, bool inf, uint8_t* out) {
  memset(out, 0, 48);
  if (inf) { out[47] |= 0x40; return; }
  fq_to_bytes(p.x, out);
  if (wire_lex_largest(p.y)) out[47] |= 0x80;
}
// ---- G2 (96-byte x = c0 || c1, flags on c1's last byte)
bool g2_decompress(const uint8_t* in, Affine<Fq2_>& p, bool& inf) {
  const WireStatus st = wire_decode_g2(in, wire_consts(), false, p);
  inf = st == WIRE_INFINITY;
  return st != WIRE_INVALID;
}
void g2_compress(const Affine<Fq2_>& p, bool inf, uint8_t* out) {
  memset(out, 0, 96);
  if (inf) { out[95] |= 0x40; return; }
  fq_to_bytes(p.x.c0, out);
  fq_to_bytes(p.x.c1, out + 48);
  if (wire_lex_largest(p.y)) out[95] |= 0x80;
}
// A ChaCha20 stream seeded with 32 bytes from the operating system (runtime.h os_random): what rand::thread_rng() is in the reference
// (batch.rs:51 draws the batching exponents from it).  One system call per FFI call instead of one per exponent word.
bool os_seeded_rng(ChaCha20Rng& rng) {
  uint8_t seed[32];
  if (!os_random(seed, sizeof seed)) return false;
  memcpy(rng.key, seed, 32);
  return true;
}
}  // namespace seam
}  // namespace celo

extern "C" {

bool init(void) {  // lib.rs:28-36: force both lazy hashers (the Bowe-Hopwood generator table) and bring the device up
  size_t gens;
  (void)celo_composite_gens(&gens);
  (void)wire_consts();
  return celo_amd_init(0) == 0;
}

// ---------------------------------------------------------------- keys (crates/bls-snark-sys/src/signatures.rs:19-42)
bool generate_private_key(PrivateKey** out_private_key) {
  if (!out_private_key) return false;
  ChaCha20Rng rng;
  if (!os_seeded_rng(rng)) return false;
  PrivateKey* sk = new PrivateKey;
  for (;;) {
    for (int i = 0; i < 4; i++) sk->k[i] = rng.next_u64();
    sk->k[3] &= (1ULL << 61) - 1;  // 253 bits
    if (wire_cmp(sk->k, R_ORDER, 4) < 0) break;
  }
  *out_private_key = sk;
  return true;
}
bool private_key_to_public_key(const PrivateKey* in_private_key, PublicKey** out_public_key) {
  if (!in_private_key || !out_public_key) return false;
  uint64_t gen[24];
  if (!celo_amd_g2_generator(gen)) return false;
  Affine<Fq2_> g = {Fq2_::from_ark(gen), Fq2_::from_ark(gen + 12)};
  Xyzz<Fq2_> r = scalar_mul_host(g, in_private_key->k, 4);
  PublicKey* pk = new_public_key();
  if (!pk) return false;
  if (r.is_identity()) identity_jac<Fq2_>(pk->xyz);
  else {
    Fq2_::mul(r.X, r.ZZ).to_ark(pk->xyz);
    Fq2_::mul(r.Y, r.ZZZ).to_ark(pk->xyz + 12);
    r.ZZ.to_ark(pk->xyz + 24);
  }
  *out_public_key = pk;
  return true;
}

// ---------------------------------------------------------------- (de)serialisation (serialization.rs:13-117)
bool deserialize_private_key(const uint8_t* in_bytes, int in_len, PrivateKey** out) {
  if (!in_bytes || !out || in_len < 32) return false;
  PrivateKey* sk = new PrivateKey;
  memcpy(sk->k, in_bytes, 32);
  if (wire_cmp(sk->k, R_ORDER, 4) >= 0) { delete sk; return false; }
  *out = sk;
  return true;
}
bool serialize_private_key(const PrivateKey* in, uint8_t** out_bytes, int* out_len) {
  if (!in || !out_bytes || !out_len) return false;
  std::vector<uint8_t> v(32);
  memcpy(v.data(), in->k, 32);
  return emit(v, out_bytes, out_len);
}
bool deserialize_public_key(const uint8_t* in_bytes, int in_len, PublicKey** out) {
  if (!in_bytes || !out || in_len < 96) return false;
  Affine<Fq2_> p;
  bool inf;
  if (!g2_decompress(in_bytes, p, inf)) { log_err("deserialize_public_key: not a valid compressed G2 point"); return false; }
  PublicKey* pk = new_public_key();
  if (!pk) return false;
  if (inf) identity_jac<Fq2_>(pk->xyz);
  else {
    if (!in_subgroup(p)) { drop(pk); log_err("deserialize_public_key: point not in the prime-order subgroup"); return false; }
    affine_to_jac(p, pk->xyz);
  }
  *out = pk;
  return true;
}
// The reference memoises decompression in a 512-entry LRU keyed by the serialized bytes (serialization.rs:44-61,
// crates/bls-crypto/src/bls/cache.rs:36,49-65): validator keys recur epoch after epoch, and a hit replaces a square root and a
// subgroup check (~0.5 ms) by a 288-byte copy.  Decoding is a pure function, so the cache is not observable through the ABI.
bool deserialize_public_key_cached(const uint8_t* in_bytes, int in_len, PublicKey** out) {
  if (!in_bytes || in_len != 96 || !out) return deserialize_public_key(in_bytes, in_len, out);
  static std::mutex mu;
  struct Limbs { uint64_t xyz[36]; };
  static std::list<std::pair<std::string, Limbs>> lru;                                       // front = most recent
  static std::unordered_map<std::string, std::list<std::pair<std::string, Limbs>>::iterator> index;
  const std::string key((const char*)in_bytes, 96);
  {
    std::lock_guard<std::mutex> lk(mu);
    auto it = index.find(key);
    if (it != index.end()) {
      lru.splice(lru.begin(), lru, it->second);
      PublicKey* pk = new_public_key();
      if (!pk) return false;
      memcpy(pk->xyz, it->second->second.xyz, 288);
      *out = pk;
      return true;
    }
  }
  if (!deserialize_public_key(in_bytes, in_len, out)) return false;
  std::lock_guard<std::mutex> lk(mu);
  if (index.find(key) == index.end()) {
    Limbs v;
    memcpy(v.xyz, (*out)->xyz, 288);
    lru.emplace_front(key, v);
    index[key] = lru.begin();
    if (lru.size() > 512) { index.erase(lru.back().first); lru.pop_back(); }
  }
  return true;
}
bool serialize_public_key(const PublicKey* in, uint8_t** out_bytes, int* out_len) {
  if (!in || !out_bytes || !out_len) return false;
  Affine<Fq2_> p;
  bool fin = jac_to_affine<Fq2_>(in->xyz, p);
  std::vector<uint8_t> v(96);
  g2_compress(p, !fin, v.data());
  return emit(v, out_bytes, out_len);
}
bool serialize_public_key_uncompressed(const PublicKey* in, uint8_t** out_bytes, int* out_len) {
  if (!in || !out_bytes || !out_len) return false;
  Affine<Fq2_> p;
  bool fin = jac_to_affine<Fq2_>(in->xyz, p);
  std::vector<uint8_t> v(192, 0);
  if (fin) {
    fq_to_bytes(p.x.c0, v.data()); fq_to_bytes(p.x.c1, v.data() + 48);
    fq_to_bytes(p.y.c0, v.data() + 96); fq_to_bytes(p.y.c1, v.data() + 144);
  } else v[191] |= 0x40;
  return emit(v, out_bytes, out_len);
}
bool deserialize_signature(const uint8_t* in_bytes, int in_len, Signature** out) {
  if (!in_bytes || !out || in_len < 48) return false;
  Affine<Fq_> p;
  bool inf;
  if (!g1_decompress(in_bytes, p, inf)) { log_err("deserialize_signature: not a valid compressed G1 point"); return false; }
  Signature* s = new_signature();
  if (!s) return false;
  if (inf) identity_jac<Fq_>(s->xyz);
  else {
    if (!in_subgroup(p)) { drop(s); log_err("deserialize_signature: point not in the prime-order subgroup"); return false; }
    affine_to_jac(p, s->xyz);
  }
  *out = s;
  return true;
}
bool serialize_signature(const Signature* in, uint8_t** out_bytes, int* out_len) {
  if (!in || !out_bytes || !out_len) return false;
  Affine<Fq_> p;
  bool fin = jac_to_affine<Fq_>(in->xyz, p);
  std::vector<uint8_t> v(48);
  g1_compress(p, !fin, v.data());
  return emit(v, out_bytes, out_len);
}
bool serialize_signature_uncompressed(const Signature* in, uint8_t** out_bytes, int* out_len) {
  if (!in || !out_bytes || !out_len) return false;
  Affine<Fq_> p;
  bool fin = jac_to_affine<Fq_>(in->xyz, p);
  std::vector<uint8_t> v(96, 0);
  if (fin) { fq_to_bytes(p.x, v.data()); fq_to_bytes(p.y, v.data() + 48); }
  else v[95] |= 0x40;
  return emit(v, out_bytes, out_len);
}
// 96-byte x||y -> 48-byte compressed (serialization.rs:167-189); 192 -> 96 (serialization.rs:192-218)
bool compress_signature(const uint8_t* in, int in_len, uint8_t** out, int* out_len) {
  if (!in || !out || !out_len || in_len < 96) return false;
  Affine<Fq_> p;
  if (!wire_fq_from_bytes(in, p.x) || !wire_fq_from_bytes(in + 48, p.y)) return false;
  std::vector<uint8_t> v(48);
  g1_compress(p, false, v.data());
  return emit(v, out, out_len);
}
bool compress_pubkey(const uint8_t* in, int in_len, uint8_t** out, int* out_len) {
  if (!in || !out || !out_len || in_len < 192) return false;
  Affine<Fq2_> p;
  if (!wire_fq_from_bytes(in, p.x.c0) || !wire_fq_from_bytes(in + 48, p.x.c1) || !wire_fq_from_bytes(in + 96, p.y.c0) || !wire_fq_from_bytes(in + 144, p.y.c1))
    return false;
  std::vector<uint8_t> v(96);
  g2_compress(p, false, v.data());
  return emit(v, out, out_len);
}

// ---------------------------------------------------------------- destructors (serialization.rs:224-268)
bool destroy_private_key(PrivateKey* p) { if (!p) return false; delete p; return true; }
bool destroy_public_key(PublicKey* p) { return p && drop(p); }   // false for a handle destroyed before (its slot stays out of the free list)
bool destroy_signature(Signature* p) { return p && drop(p); }
bool free_vec(uint8_t* bytes, int len) { if (!bytes || len < 0) return false; free(bytes); return true; }   // buffers are malloc blocks: the length is not needed to release one

// ---------------------------------------------------------------- aggregation (signatures.rs:428-505)
// aggregate_public_keys and aggregate_public_keys_subtract route their list through PublicKeyCache::aggregate
// (crates/bls-crypto/src/bls/cache.rs:65-87), which collects the keys into a HashSet with BYTE-LEVEL equality of the Jacobian
// (x, y, z) limbs (cache.rs:95-104): a handle listed twice - or two handles holding the same limbs - counts once, whereas two
// different Jacobian representatives of one point count twice.  The cache's incremental update (subtract the keys that left,
// add the new ones) is an optimisation of "sum of the set"; only the set semantics is observable.  aggregate_signatures is a
// plain sum (Signature::aggregate, signature.rs:61-67).
static bool unique_key_limbs(const PublicKey* const* in, int n, std::vector<uint64_t>& buf, size_t first) {
  struct Ref { const uint64_t* p; };
  struct H { size_t operator()(const Ref& r) const { uint64_t h = 0xcbf29ce484222325ull; for (int i = 12; i < 24; i++) h = (h ^ r.p[i]) * 0x100000001b3ull; return (size_t)h; } };
  struct E { bool operator()(const Ref& a, const Ref& b) const { return memcmp(a.p, b.p, 288) == 0; } };
  std::unordered_set<Ref, H, E> seen;
  seen.reserve((size_t)n * 2 + 1);
  buf.resize(first * 36);
  for (int i = 0; i < n; i++) {
    if (!in[i]) return false;
    if (!seen.insert(Ref{in[i]->xyz}).second) continue;
    buf.insert(buf.end(), in[i]->xyz, in[i]->xyz + 36);
  }
  return true;
}
bool aggregate_public_keys(const PublicKey* const* in, int n, PublicKey** out) {
  if (!out || n < 0 || (n > 0 && !in)) return false;
  std::vector<uint64_t> buf;
  if (!unique_key_limbs(in, n, buf, 0)) return false;
  PublicKey* pk = new_public_key();
  if (!pk) return false;
  if (celo_amd_sum_jacobian_bls12_377_g2(buf.data(), buf.size() / 36, pk->xyz) != 0) { drop(pk); return false; }
  *out = pk;
  return true;
}
bool aggregate_public_keys_subtract(const PublicKey* agg, const PublicKey* const* in, int n, PublicKey** out) {
  if (!agg || !out || n < 0 || (n > 0 && !in)) return false;
  std::vector<uint64_t> buf;
  if (!unique_key_limbs(in, n, buf, 1)) return false;
  memcpy(buf.data(), agg->xyz, 288);
  for (size_t i = 1; i < buf.size() / 36; i++) {
    uint64_t* d = &buf[i * 36];
    Fq2_ y = Fq2_::from_ark(d + 12);                       // negate: (X, -Y, Z)
    Fq2_ ny = {wire_neg(y.c0), wire_neg(y.c1)};
    ny.to_ark(d + 12);
  }
  PublicKey* pk = new_public_key();
  if (!pk) return false;
  if (celo_amd_sum_jacobian_bls12_377_g2(buf.data(), buf.size() / 36, pk->xyz) != 0) { drop(pk); return false; }
  *out = pk;
  return true;
}
bool aggregate_signatures(const Signature* const* in, int n, Signature** out) {
  if (!out || n < 0 || (n > 0 && !in)) return false;
  std::vector<uint64_t> buf((size_t)n * 18);
  for (int i = 0; i < n; i++) { if (!in[i]) return false; memcpy(&buf[(size_t)i * 18], in[i]->xyz, 144); }
  Signature* s = new_signature();
  if (!s) return false;
  if (celo_amd_sum_jacobian_bls12_377_g1(buf.data(), (size_t)n, s->xyz) != 0) { drop(s); return false; }
  *out = s;
  return true;
}
}
