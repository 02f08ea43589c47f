// Epoch blocks to bytes, digests and Groth16 public inputs (crates/epoch-snark/src/epoch_block.rs:106-236, encoding.rs:23-83,
// crates/bls-gadgets/src/utils.rs:2-56, gadgets/mod.rs:75-83), as host+device templates.  DESIGN.md section 6k.
//
// The reference builds a vector of bits B[0 .. n) - index, entropies and maximum_non_signers least significant bit first, every key as
// x.c0 and x.c1 in 377 bits each, MOST significant bit first, then the sign bit of y - and turns it into bytes with bits_be_to_bytes_le,
// which reverses the whole vector: bit p of the output, read as one little-endian integer, is B[n - 1 - p].  Seen from the output:
//   bits [755 r, 755 (r + 1))      the key of position NK - 1 - r (NK key positions), as the integer R = sign | x.c1 << 1 | x.c0 << 378
//   bits [755 NK, 755 NK + H)      the header, every field bit-reversed, the FIRST field on top
//   up to the next byte            zero
// so the stream is a concatenation of little-endian integers, the keys in reverse order.  A key's R (its "record", 24 u32 words, zero
// above bit 754) is computed once per key (epoch_key_record); an output word gathers its 32 bits from at most two neighbouring sources
// (epoch_pack_word).  755 = 3 mod 8: neighbouring keys share bytes at every alignment, which is why the output is gathered word by word
// and not scattered key by key.
//
// kind 0   first-epoch form       index(16) parent_entropy(128) maximum_non_signers(32) K keys                      H = 176
// kind 1   last-epoch form        index(16) epoch_entropy(128)  maximum_non_signers(32) K keys, the aggregated key  H = 176
// kind 2   inner CIP22            epoch_entropy(128) parent_entropy(128) K keys; extra = index(16) round(8) maximum_non_signers(32)   H = 256
// kind 3   pre-CIP22              index(16) maximum_non_signers(32) n_keys keys                                      H = 48
// K = max(n_keys, maximum_validators): positions n_keys .. K - 1 hold the G2 generator.
#pragma once
#include "hash_direct.h"

namespace celo {

constexpr uint32_t EPOCH_KEY_BITS = 755, EPOCH_REC_WORDS = 24, EPOCH_HDR_WORDS = 8;
constexpr uint32_t EPOCH_MAX_KEYS = 1u << 16;      // per block, padding included: no single maximum_validators sizes a buffer
constexpr size_t EPOCH_MAX_BLOCKS = size_t(1) << 24;
constexpr int EPOCH_KINDS = 4;

struct EpochRecord { uint32_t w[EPOCH_REC_WORDS]; };

HD uint32_t epoch_header_bits(int kind) { return kind == 2 ? 256u : kind == 3 ? 48u : 176u; }
// key positions after the header: the padded set, and the aggregated key of the last-epoch form
HD uint32_t epoch_key_slots(int kind, uint32_t n_keys, uint32_t max_validators) {
  const uint32_t k = kind == 3 || n_keys > max_validators ? n_keys : max_validators;
  return k + (kind == 1 ? 1u : 0u);
}
HD uint64_t epoch_encoded_bits(int kind, uint32_t n_keys, uint32_t max_validators) {
  return epoch_header_bits(kind) + (uint64_t)EPOCH_KEY_BITS * epoch_key_slots(kind, n_keys, max_validators);
}
HD bool epoch_block_ok(uint32_t n_keys, uint32_t max_validators) { return n_keys <= EPOCH_MAX_KEYS && max_validators <= EPOCH_MAX_KEYS; }

HD uint32_t epoch_rev32(uint32_t v) {
  v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
  v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
  v = ((v >> 4) & 0x0F0F0F0Fu) | ((v & 0x0F0F0F0Fu) << 4);
  v = ((v >> 8) & 0x00FF00FFu) | ((v & 0x00FF00FFu) << 8);
  return (v >> 16) | (v << 16);
}
// bits [p, p + 32) of the little-endian integer in w[0 .. nwords), zero outside it; p may be negative
HD uint32_t epoch_bits32(const uint32_t* w, int nwords, int64_t p) {
  if (p <= -32 || p >= 32 * (int64_t)nwords) return 0;
  const int64_t q = p + 32;
  const int i = (int)(q >> 5) - 1, sh = (int)(q & 31);
  const uint32_t a = i >= 0 ? w[i] : 0u, b = i + 1 < nwords ? w[i + 1] : 0u;
  return sh ? (a >> sh) | (b << (32 - sh)) : a;
}

// out |= x << shift for a 6-word x into 12 words
HD void epoch_or_shifted(uint64_t out[12], const uint64_t x[6], int shift) {
  const int q = shift >> 6, s = shift & 63;
#pragma unroll
  for (int i = 0; i < 6; i++) {
    out[i + q] |= x[i] << s;
    if (s && i + q + 1 < 12) out[i + q + 1] |= x[i] >> (64 - s);
  }
}
// One key: a row of 24 u64 (x.c0, x.c1, y.c0, y.c1 in arkworks Montgomery limbs) -> R = sign | x.c1 << 1 | x.c0 << 378, where sign is
// y.c1 > (q-1)/2 || (y.c1 == 0 && y.c0 > (q-1)/2) (encoding.rs:23-47).  The identity is arkworks' zero() = (0, 1): R = 0.
HD void epoch_key_record(const uint64_t* row, bool inf, uint32_t rec[EPOCH_REC_WORDS]) {
  uint64_t r[12];
#pragma unroll
  for (int i = 0; i < 12; i++) r[i] = 0;
  if (!inf) {
    uint64_t x0[6], x1[6], y0[6], y1[6];
    wire_ark_to_canonical<P377>(row, x0);
    wire_ark_to_canonical<P377>(row + 6, x1);
    wire_ark_to_canonical<P377>(row + 12, y0);
    wire_ark_to_canonical<P377>(row + 18, y1);
    uint64_t c1 = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) c1 |= y1[i];
    const bool sign = c1 ? wire_less<6>(P377::PM1_HALF64, y1) : wire_less<6>(P377::PM1_HALF64, y0);
    r[0] = sign ? 1 : 0;
    epoch_or_shifted(r, x1, 1);
    epoch_or_shifted(r, x0, 378);
  }
#pragma unroll
  for (int i = 0; i < 12; i++) { rec[2 * i] = (uint32_t)r[i]; rec[2 * i + 1] = (uint32_t)(r[i] >> 32); }
}

// the 128 bits of an entropy (16 bytes, or NULL for none: the same 128 zero bits, encode_entropy_cip22), bit-reversed as one integer
HD void epoch_rev_entropy(const uint8_t* e, uint32_t out[4]) {
#pragma unroll
  for (int j = 0; j < 4; j++) {
    uint32_t v = 0;
    if (e) for (int b = 3; b >= 0; b--) v = (v << 8) | e[4 * (3 - j) + b];
    out[j] = epoch_rev32(v);
  }
}
// the header of one block as a little-endian integer of epoch_header_bits(kind) bits, zero above them
HD void epoch_header(int kind, uint32_t index, uint32_t max_non_signers, const uint8_t* epoch_entropy, const uint8_t* parent_entropy, uint32_t hd[EPOCH_HDR_WORDS]) {
#pragma unroll
  for (int i = 0; i < (int)EPOCH_HDR_WORDS; i++) hd[i] = 0;
  const uint32_t idx = epoch_rev32(index & 0xFFFFu) >> 16;
  if (kind == 2) {
    epoch_rev_entropy(parent_entropy, hd);
    epoch_rev_entropy(epoch_entropy, hd + 4);
  } else if (kind == 3) {
    hd[0] = epoch_rev32(max_non_signers);
    hd[1] = idx;
  } else {
    hd[0] = epoch_rev32(max_non_signers);
    epoch_rev_entropy(kind == 0 ? parent_entropy : epoch_entropy, hd + 1);
    hd[5] = idx;
  }
}
// the 7 bytes of extra data of the inner form: index(16) round(8) maximum_non_signers(32), reversed like the block
HD void epoch_extra(uint32_t index, uint32_t round, uint32_t max_non_signers, uint8_t out[7]) {
  const uint32_t w0 = epoch_rev32(max_non_signers), w1 = (epoch_rev32(round & 0xFFu) >> 24) | ((epoch_rev32(index & 0xFFFFu) >> 16) << 8);
  for (int i = 0; i < 4; i++) out[i] = (uint8_t)(w0 >> (8 * i));
  for (int i = 0; i < 3; i++) out[4 + i] = (uint8_t)(w1 >> (8 * i));
}

// Word w (32 bits) of one block's output.  keys: the records of the block's own keys (n_keys of them); gen: the generator's record; sum: the
// record of the block's aggregated key (kind 1 only); nk = epoch_key_slots().  Words past the last bit come out zero: the padding.
HD uint32_t epoch_pack_word(int kind, uint64_t w, uint32_t n_keys, uint32_t nk, const uint32_t hd[EPOCH_HDR_WORDS], const uint32_t* keys, const uint32_t* gen,
                            const uint32_t* sum) {
  const int64_t p0 = (int64_t)(32 * w), top = (int64_t)EPOCH_KEY_BITS * nk;
  if (p0 >= top) return epoch_bits32(hd, EPOCH_HDR_WORDS, p0 - top);
  const uint32_t r = (uint32_t)(p0 / EPOCH_KEY_BITS);
  // the record at position r from the bottom is the key of position nk - 1 - r
  auto rec = [&](uint32_t rr) -> const uint32_t* {
    const uint32_t kk = nk - 1 - rr;
    if (kind == 1 && kk == nk - 1) return sum;
    return kk < n_keys ? keys + (size_t)kk * EPOCH_REC_WORDS : gen;
  };
  const int64_t off = p0 - (int64_t)EPOCH_KEY_BITS * r;
  uint32_t v = epoch_bits32(rec(r), EPOCH_REC_WORDS, off);
  if (off + 32 > (int64_t)EPOCH_KEY_BITS) {       // the window reaches into the next source
    if (r + 1 < nk) v |= epoch_bits32(rec(r + 1), EPOCH_REC_WORDS, off - EPOCH_KEY_BITS);
    else v |= epoch_bits32(hd, EPOCH_HDR_WORDS, off - EPOCH_KEY_BITS);
  }
  return v;
}

// Blake2s-256 under the personalisation OUT_DOMAIN = "ULforout" (hash_to_bits, epoch_block.rs:226-236) of len bytes held as little-endian
// words, zero-filled up to the next multiple of 64 bytes.  m and h stay in registers: every index below is a compile-time constant.
HD void epoch_blake2s(const uint32_t* msg, uint64_t len, uint32_t h[8]) {
  const uint8_t dom[8] = {'U', 'L', 'f', 'o', 'r', 'o', 'u', 't'};
  b2s_init(h, 32, 1, 1, 0, 0, 0, 0, dom);
  const uint64_t blocks = len ? (len + 63) / 64 : 1;
  for (uint64_t b = 0; b < blocks; b++) {
    uint32_t m[16];
#pragma unroll
    for (int i = 0; i < 16; i++) m[i] = msg[16 * b + i];
    const bool last = b + 1 == blocks;
    b2s_compress_inline(h, m, last ? len : 64 * (b + 1), last);
  }
}

// Two digests -> the two public inputs (hash_first_last_epoch_block + pack::<Fr, 376>, gadgets/mod.rs:75-83): S = the 512 digest bits, least
// significant bit of the first digest first; input 0 = S[0 .. 376) and input 1 = S[376 .. 512), each read MOST significant bit first.
// Canonical little-endian limbs; 376 and 136 bits are below r (377 bits), so neither can fail a range test.
HD void epoch_inputs(const uint32_t h_first[8], const uint32_t h_last[8], uint64_t out[12]) {
  uint32_t t[16], u[5], v[12];
#pragma unroll
  for (int i = 0; i < 8; i++) { t[i] = h_first[i]; t[8 + i] = h_last[i]; }
#pragma unroll
  for (int j = 0; j < 12; j++) v[j] = epoch_rev32(epoch_bits32(t, 16, 344 - 32 * j));   // bit q of input 0 is S[375 - q]
#pragma unroll
  for (int k = 0; k < 5; k++) u[k] = epoch_bits32(t, 16, 376 + 32 * k);                   // U = S >> 376, 136 bits
#pragma unroll
  for (int j = 0; j < 6; j++) out[j] = (uint64_t)v[2 * j] | ((uint64_t)v[2 * j + 1] << 32);
#pragma unroll
  for (int j = 0; j < 6; j++) {
    const uint32_t lo = epoch_rev32(epoch_bits32(u, 5, 104 - 64 * j)), hi = epoch_rev32(epoch_bits32(u, 5, 104 - 64 * j - 32));
    out[6 + j] = (uint64_t)lo | ((uint64_t)hi << 32);                                       // bit q of input 1 is U[135 - q]
  }
}

// the block that holds position x of an offsets array (off[0] <= x < off[nb]; empty blocks are skipped): the largest b with off[b] <= x
template <class T> HD uint32_t epoch_find_block(const T* off, uint32_t nb, T x) {
  uint32_t lo = 0, hi = nb;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

}  // namespace celo
