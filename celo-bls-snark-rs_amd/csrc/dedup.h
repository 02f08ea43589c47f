// De-duplication of compressed keys by their bytes: a hash table that finds, for every key of a batch, a representative with identical
// bytes, so that only the representatives go through the decoder (unit_dedup.hip) and every key then receives its representative's row
// and status.  What PublicKeyCache::deserialize of the reference (crates/bls-crypto/src/bls/cache.rs) is on the host - "the aggregated
// public key changes slowly" - for the bulk device paths.  Host and device from one source, as check.h and aggregate.h: the kernels of
// unit_dedup.hip run these templates one key per lane with device atomics (DedupDeviceOps there), the host twin below runs them key after
// key with plain stores (DedupHostOps; csrc/host_test.cpp ht_dedup_*, tests/dedup_asan_main.cpp).  Standard library only on the host side.
//
// The table: two uint32_t arrays of S slots, S = next_pow2(n) << slack_log (slack_log 0 .. 2, default 1: load <= 0.5), both initialised
// to 0xFFFFFFFF.  owner[s] is the index of the key that claimed slot s, first[s] the smallest index of any key that joined it.  Memory:
// 8 S bytes: 16 n .. 32 n at the default (at most 32 n, n just above a power of two), half of that at slack_log 0, twice at 2.  (S is
// held to 2^31, so that a slot number fits the 32-bit slot_of next to DEDUP_NONE; n itself is below 2^31.)
//
// Insert: probe linearly from mix(key) & (S - 1); at each slot cas(owner[s], EMPTY, i).  EMPTY back: the key owns the slot.  Otherwise
// the key's bytes are compared with those of key `returned`: equal joins the slot, different moves on.  On owning or joining,
// min(first[s], i) and slot_of[i] = s.  A slot is read only through what the atomic returns (the L2s of the XCDs are not coherent for
// plain loads inside one kernel); the kernel boundary publishes the table to k_dedup_rep.  The key bytes are inputs written before the
// launch, so comparing against another key's bytes needs no ordering.
// The probe cap: after max_probes slots (default 64, 1 .. 1024) the key stops and becomes its own representative (slot_of[i] = NONE) -
// it is simply decoded on its own.  That bounds the work at max_probes n comparisons for crafted keys that share one home slot (the keys
// are untrusted chain data and the mix is public: no secret seed is needed), and it makes a full table terminate.
//
// The contract of rep[i] = first[slot_of[i]] (i for a capped key), for every input and every race order:
//   rep[i] <= i,  key rep[i] has the bytes of key i,  rep[rep[i]] == rep[i].
// (An owner never changes, so two keys with equal bytes walk past the same foreign slots and stop at the same slot unless one is capped;
// every joiner of a slot has the owner's bytes; first[s] is one of the joiners, and it joined s itself.)  When no probe sequence reaches
// the cap, rep[i] is exactly the smallest j whose key equals key i.  Which keys hit the cap may differ from run to run; what is decoded
// from them never does.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define DEDUP_HD __host__ __device__ inline
#else
#define DEDUP_HD inline
#endif

namespace celo {

constexpr uint32_t DEDUP_EMPTY = 0xFFFFFFFFu, DEDUP_NONE = 0xFFFFFFFFu;
constexpr int DEDUP_SLACK_DEFAULT = 1, DEDUP_SLACK_MAX = 2, DEDUP_PROBES_DEFAULT = 64, DEDUP_PROBES_MAX = 1024;
// the rule behind celo_amd_key_dedup_set(-1, ..): the composed callers de-duplicate from DEDUP_N0 keys up; 0 = never.  By measurement on
// keys that are all distinct, the case where the table can only lose (tools/bench_key_dedup.py, profiles/bench_key_dedup.json)
constexpr uint64_t DEDUP_N0 = 0;
DEDUP_HD bool key_dedup_pick(uint64_t n) { return DEDUP_N0 != 0 && n >= DEDUP_N0; }

// S for n keys: the next power of two at or above n, times 2^slack_log, at most 2^31
DEDUP_HD uint64_t dedup_slots(uint64_t n, int slack_log) {
  uint64_t s = 1;
  while (s < n) s <<= 1;
  s <<= slack_log;
  return s > (uint64_t(1) << 31) ? (uint64_t(1) << 31) : s;
}

// the key as KB / 8 little-endian 64-bit words.  ALIGNED: the key lies at a multiple of 8 (KB is one, so every key of an 8-aligned batch does)
template <int KB, bool ALIGNED> DEDUP_HD void dedup_load(const uint8_t* key, uint64_t* w) {
  if constexpr (ALIGNED) {
    const uint64_t* k = reinterpret_cast<const uint64_t*>(key);
    for (int j = 0; j < KB / 8; j++) w[j] = k[j];
  } else {
    for (int j = 0; j < KB / 8; j++) {
      uint64_t v = 0;
      for (int b = 0; b < 8; b++) v |= (uint64_t)key[8 * j + b] << (8 * b);
      w[j] = v;
    }
  }
}

// 64 bits from all words of the key (12 for a G2 key, 6 for a G1 key): every step is a bijection of the state for a fixed word, so every
// byte takes part, the flag byte included.  tests/dedup_ref.py restates it.
DEDUP_HD uint64_t dedup_mix(const uint64_t* w, int words) {
  uint64_t h = 0x9E3779B97F4A7C15ull * (uint64_t)(words + 1);
  for (int j = 0; j < words; j++) {
    h ^= w[j];
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 29;
  }
  h ^= h >> 30; h *= 0xBF58476D1CE4E5B9ull;
  h ^= h >> 27; h *= 0x94D049BB133111EBull;
  return h ^ (h >> 31);
}
template <int KB, bool ALIGNED> DEDUP_HD uint64_t dedup_hash(const uint8_t* key) {
  uint64_t w[KB / 8];
  dedup_load<KB, ALIGNED>(key, w);
  return dedup_mix(w, KB / 8);
}

template <int KB, bool ALIGNED> DEDUP_HD bool dedup_equal(const uint64_t* w, const uint8_t* other) {
  uint64_t o[KB / 8];
  dedup_load<KB, ALIGNED>(other, o);
  uint64_t d = 0;
  for (int j = 0; j < KB / 8; j++) d |= w[j] ^ o[j];
  return d == 0;
}

// Key i of `keys` (n x KB bytes) into the table of mask + 1 slots: the slot it owns or joined, or DEDUP_NONE at the cap.
// A: cas(p, expect, v) and min(p, v), both returning the value before - device atomics in the kernel, plain code in the host twin
template <int KB, bool ALIGNED, class A>
DEDUP_HD uint32_t dedup_insert(const uint8_t* keys, uint32_t i, uint32_t* owner, uint32_t* first, uint32_t mask, uint32_t max_probes, A at) {
  uint64_t w[KB / 8];
  dedup_load<KB, ALIGNED>(keys + (size_t)i * KB, w);
  uint32_t s = (uint32_t)dedup_mix(w, KB / 8) & mask;
  for (uint32_t p = 0; p < max_probes; p++, s = (s + 1) & mask) {
    const uint32_t o = at.cas(owner + s, DEDUP_EMPTY, i);
    if (o == DEDUP_EMPTY || dedup_equal<KB, ALIGNED>(w, keys + (size_t)o * KB)) {
      at.min(first + s, i);
      return s;
    }
  }
  return DEDUP_NONE;
}
DEDUP_HD uint32_t dedup_rep(const uint32_t* first, uint32_t slot, uint32_t i) { return slot == DEDUP_NONE ? i : first[slot]; }

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host twin: the same templates, key after key
struct DedupHostOps {
  uint32_t cas(uint32_t* p, uint32_t expect, uint32_t v) const { const uint32_t old = *p; if (old == expect) *p = v; return old; }
  uint32_t min(uint32_t* p, uint32_t v) const { const uint32_t old = *p; if (v < old) *p = v; return old; }
};
// owner, first: S = dedup_slots(n, slack_log) entries each, written here; slot_of, rep, rank: n each; list: n (its first U entries are
// written: the representatives in index order; rank[list[r]] = r, and rank is DEDUP_NONE elsewhere).  Returns U
template <int KB> inline uint32_t dedup_host(const uint8_t* keys, uint32_t n, int slack_log, uint32_t max_probes, uint32_t* owner, uint32_t* first, uint32_t* slot_of,
                                             uint32_t* rep, uint32_t* list, uint32_t* rank) {
  const uint64_t S = dedup_slots(n, slack_log);
  for (uint64_t s = 0; s < S; s++) owner[s] = first[s] = DEDUP_EMPTY;
  for (uint32_t i = 0; i < n; i++) slot_of[i] = dedup_insert<KB, false>(keys, i, owner, first, (uint32_t)(S - 1), max_probes, DedupHostOps{});
  uint32_t U = 0;
  for (uint32_t i = 0; i < n; i++) {
    rep[i] = dedup_rep(first, slot_of[i], i);
    rank[i] = DEDUP_NONE;
    if (rep[i] == i) { rank[i] = U; list[U++] = i; }
  }
  return U;
}
#endif

}  // namespace celo
