// Chains of epoch transitions: can the circuit ValidatorSetUpdate (crates/epoch-snark/src/gadgets/epochs.rs:97-283, single_update.rs:79-135,
// epoch_data.rs:223-233, crates/bls-gadgets/src/bls.rs:138-191) be satisfied by an initial block and a list of
// EpochTransition { block, aggregate_signature, bitmap } (crates/epoch-snark/src/api/prover.rs:22-82)?  This header is the rule alone: from the
// facts about one block - fields, counts and the flags the earlier stages left - to its status.  k_transition_status (unit_transitions.hip)
// and the host twin of host_test.cpp call the same function.
//
// Block b of a chain is its initial epoch or a transition whose predecessor is p = b - 1; the keys of p, selected by the bitmap under p,
// sign b.  The first status that applies is reported:
//    0  accepted (for a transition: so far - the product decides between 0 and 10)
//    1  a key of b does not decode or lies outside G2
//    2  p has status 1: the signing set is unknown
//    3  index[b] != index[p] + 1 as integers (no wrap; a transition with index 0 always lands here)         epoch_data.rs:223-233
//    4  n_keys(b) != n_keys(p): the circuit's num_validators is fixed                                       single_update.rs:92
//    5  the chain's INITIAL block has a non-zero epoch_entropy and parent_entropy[b] != epoch_entropy[p]    epochs.rs:193, single_update.rs:104-107
//    6  signers < n_keys(p) - max_non_signers[p] (saturating at 0), or no signer at all                     bls.rs:187
//    7  a SELECTED key of p is the padding key, the G2 generator                                            bls.rs:147-148, epoch_block.rs:94-96
//    8  the signature does not decode or lies outside G1
//    9  the hash found no counter
//   10  the product is not one (placed by the caller of the rule, from the pairing engine's verdict)
// An initial block can only get 0 or 1.
#pragma once
#include <cstdint>
#include <cstddef>
#if defined(__HIPCC__)
#define TR_FN __host__ __device__ inline
#else
#define TR_FN inline
#endif

namespace celo {

enum TransitionStatus : uint8_t {
  TR_OK = 0, TR_BAD_KEY = 1, TR_BAD_SET = 2, TR_INDEX = 3, TR_KEY_COUNT = 4, TR_ENTROPY = 5, TR_THRESHOLD = 6, TR_PADDING_KEY = 7, TR_BAD_SIGNATURE = 8,
  TR_NO_COUNTER = 9, TR_PRODUCT = 10
};

struct TransitionFacts {
  bool initial;                     // the first block of its chain: nothing below `bad_key` is read
  bool bad_key, pred_bad_key;       // the block statuses of b and p (epoch_encode_blocks status 1)
  uint32_t index, pred_index;
  uint32_t n_keys, pred_n_keys;
  bool entropy_live;                // the chain's initial block has a non-zero epoch_entropy
  bool entropy_equal;               // parent_entropy[b] == epoch_entropy[p], 16 bytes, a NULL array read as zeros
  uint32_t signers;                 // non-zero bytes of the bitmap under p
  uint32_t pred_max_non_signers;
  bool padding_selected;            // a selected key of p equals the G2 generator
  uint8_t sig_wire;                 // the decoder's status of the signature: 0 decoded, 1 the identity's encoding, 2 / 3 refused
  uint8_t attempt;                  // the hash counter, 255 = none found
};

TR_FN uint8_t transition_status(const TransitionFacts& f) {
  if (f.bad_key) return TR_BAD_KEY;
  if (f.initial) return TR_OK;
  if (f.pred_bad_key) return TR_BAD_SET;
  if ((uint64_t)f.index != (uint64_t)f.pred_index + 1) return TR_INDEX;
  if (f.n_keys != f.pred_n_keys) return TR_KEY_COUNT;
  if (f.entropy_live && !f.entropy_equal) return TR_ENTROPY;
  const uint32_t need = f.pred_n_keys > f.pred_max_non_signers ? f.pred_n_keys - f.pred_max_non_signers : 0;
  if (f.signers == 0 || f.signers < need) return TR_THRESHOLD;
  if (f.padding_selected) return TR_PADDING_KEY;
  if (f.sig_wire >= 2) return TR_BAD_SIGNATURE;
  if (f.attempt == 255) return TR_NO_COUNTER;
  return TR_OK;
}

// 16 bytes at a + 16 i against 16 bytes at b + 16 j; a NULL array is all zero
TR_FN bool transition_entropy_equal(const uint8_t* a, size_t i, const uint8_t* b, size_t j) {
  for (int k = 0; k < 16; k++)
    if ((a ? a[16 * i + k] : 0) != (b ? b[16 * j + k] : 0)) return false;
  return true;
}
TR_FN bool transition_entropy_nonzero(const uint8_t* a, size_t i) {
  if (!a) return false;
  for (int k = 0; k < 16; k++) if (a[16 * i + k]) return true;
  return false;
}
// does a selected, present key among rows [k0, k1) equal `gen` (24 u64, the decoded Montgomery limbs of the G2 generator)?
TR_FN bool transition_padding_selected(const uint64_t* rows, const uint8_t* inf, const uint8_t* bits, uint32_t k0, uint32_t k1, const uint64_t* gen) {
  for (uint32_t k = k0; k < k1; k++) {
    if (!bits[k] || (inf && inf[k])) continue;
    const uint64_t* r = rows + (size_t)k * 24;
    bool eq = true;
    for (int w = 0; w < 24 && eq; w++) eq = r[w] == gen[w];
    if (eq) return true;
  }
  return false;
}

}  // namespace celo
