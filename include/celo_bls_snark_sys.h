/* celo_bls_snark_sys.h — "Seam A" (SURVEY.md §8b): the C ABI of crates/bls-snark-sys, rebuilt over the gfx950 hot path.
 *
 * Same symbol names, argument order and ownership rules as the reference (file:line cited per entry) so that existing
 * cgo / FFI callers link unchanged.  `bool` return = "no internal error" (reference: convert_result_to_bool,
 * crates/bls-snark-sys/src/lib.rs:21-27); verdicts are separate out-params.
 *
 * All 36 symbols of the reference are exported: lifecycle, key handles, (de)serialisation and compression, aggregate_*, sign / hash /
 * verify / batch-verify with BOTH hashers (DIRECT: Blake2s CRH + Blake2Xs XOF; COMPOSITE: Bowe-Hopwood-Pedersen CRH over
 * ed-on-BW6-761 + Blake2Xs XOF), plain and CIP22 try-and-increment with the deployed `compat` bit logic, Groth16 `verify`
 * and the two epoch encoders.  `(composite = false, cip22 = true)` is an error exactly as in the reference
 * (signatures.rs:61,265,321,387).  Single-key decoding, single hashes and bit-packing run on the host; every MSM and pairing, the
 * message hashing of the batch entry points (every hasher, from 256 messages up) and the whole of batch_verify_strict's
 * Batch::verify chain run on the GPU.  Re-entrant: callable from any number of host threads (no global lock).
 *
 * Differences from the reference, all deliberate:
 *   - hash_composite / hash_composite_cip22 return ToBytes of a G1Projective (x || y || z, 144 B).  Since round 5 these are the bytes of the
 *     Jacobian representative arkworks' scale_by_cofactor leaves (MSB-first double-and-add with its dbl-2009-l / madd-2007-bl formulas,
 *     restated in csrc/seam_hash.hip ark_scale_by_cofactor_tobytes); rounds 1-4 returned (x, y, 1).  No reference vector pins these bytes
 *     (the reference's tests compare points), so the restatement is checked against the pinned hash POINTS and an independent big-integer
 *     replay of the same schedule - until a vector exists, callers should still compare after into_affine().
 *   - an epoch block that lists the point at infinity as a validator key is refused by encode_epoch_block_to_bytes* and verify
 *     (the reference's read_pubkeys accepts it).
 *   - a compressed point whose last byte has BOTH flag bits set (0xC0) is rejected, like ark-serialize's SWFlags::from_u8.
 */
#ifndef CELO_BLS_SNARK_SYS_H
#define CELO_BLS_SNARK_SYS_H
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct PrivateKey PrivateKey; /* opaque: Fr                      (crates/bls-crypto/src/bls/secret.rs:12) */
typedef struct PublicKey PublicKey;   /* opaque: G2 point, Jacobian      (crates/bls-crypto/src/bls/public.rs:16) */
typedef struct Signature Signature;   /* opaque: G1 point, Jacobian      (crates/bls-crypto/src/bls/signature.rs:17) */

/* #[repr(C)] structs of crates/bls-snark-sys/src/utils.rs:20-82 */
typedef struct Buffer { const uint8_t* ptr; size_t len; } Buffer;
typedef struct MessageFFI { Buffer data; Buffer extra; const PublicKey* public_key; const Signature* sig; } MessageFFI;
typedef struct BatchMessageFFI {
  Buffer data; Buffer extra;
  const PublicKey* const* public_keys; size_t public_keys_len;
  const Signature* const* signatures; size_t signatures_len;
} BatchMessageFFI;

bool init(void);                                                                       /* lib.rs:31 */
bool generate_private_key(PrivateKey** out_private_key);                               /* signatures.rs:19 */
bool private_key_to_public_key(const PrivateKey* in_private_key, PublicKey** out_public_key); /* signatures.rs:28 */

bool deserialize_private_key(const uint8_t* in_bytes, int in_len, PrivateKey** out);   /* serialization.rs:13 */
bool serialize_private_key(const PrivateKey* in, uint8_t** out_bytes, int* out_len);   /* serialization.rs:26 */
bool deserialize_public_key(const uint8_t* in_bytes, int in_len, PublicKey** out);     /* serialization.rs:35  (96-byte compressed G2, subgroup-checked) */
bool deserialize_public_key_cached(const uint8_t* in_bytes, int in_len, PublicKey** out); /* serialization.rs:44 */
bool serialize_public_key(const PublicKey* in, uint8_t** out_bytes, int* out_len);     /* serialization.rs:63 */
bool serialize_public_key_uncompressed(const PublicKey* in, uint8_t** out_bytes, int* out_len); /* serialization.rs:72 */
bool deserialize_signature(const uint8_t* in_bytes, int in_len, Signature** out);      /* serialization.rs:81  (48-byte compressed G1) */
bool serialize_signature(const Signature* in, uint8_t** out_bytes, int* out_len);      /* serialization.rs:90 */
bool serialize_signature_uncompressed(const Signature* in, uint8_t** out_bytes, int* out_len); /* serialization.rs:99 */
bool compress_signature(const uint8_t* in, int in_len, uint8_t** out, int* out_len);   /* serialization.rs:167 (96 -> 48 bytes) */
bool compress_pubkey(const uint8_t* in, int in_len, uint8_t** out, int* out_len);      /* serialization.rs:192 (192 -> 96 bytes) */

bool destroy_private_key(PrivateKey* p);                                               /* serialization.rs:224 */
bool free_vec(uint8_t* bytes, int len);                                                /* serialization.rs:236 */
bool destroy_public_key(PublicKey* p);                                                 /* serialization.rs:248 */
bool destroy_signature(Signature* p);                                                  /* serialization.rs:260 */

bool aggregate_public_keys(const PublicKey* const* in, int n, PublicKey** out);        /* signatures.rs:428 */
bool aggregate_public_keys_subtract(const PublicKey* agg, const PublicKey* const* in, int n, PublicKey** out); /* signatures.rs:454 */
bool aggregate_signatures(const Signature* const* in, int n, Signature** out);         /* signatures.rs:485 */

bool sign_message(const PrivateKey* sk, const uint8_t* msg, int msg_len, const uint8_t* extra, int extra_len,
                  bool should_use_composite, bool should_use_cip22, Signature** out_signature);              /* signatures.rs:44 */
bool sign_pop(const PrivateKey* sk, const uint8_t* msg, int msg_len, Signature** out_signature);           /* signatures.rs:74 */
bool hash_direct(const uint8_t* msg, int msg_len, uint8_t** out_hash, int* out_len, bool use_pop);         /* signatures.rs:93  (97 bytes: x || y || inf) */
bool hash_direct_with_attempt(const uint8_t* msg, int msg_len, uint8_t** out_hash, int* out_len, int* out_attempt, bool use_pop); /* :117 */
bool hash_direct_first_step(const uint8_t* msg, int msg_len, int hash_bytes, uint8_t** out_hash, int* out_len); /* signatures.rs:192 */
bool hash_composite(const uint8_t* msg, int msg_len, const uint8_t* extra, int extra_len, uint8_t** out_hash, int* out_len); /* signatures.rs:143 (144 bytes: x || y || z) */
bool hash_crh(const uint8_t* msg, int msg_len, int hash_bytes, uint8_t** out_hash, int* out_len);          /* signatures.rs:169 (48 bytes: Bowe-Hopwood CRH x-coordinate) */
bool hash_composite_cip22(const uint8_t* msg, int msg_len, const uint8_t* extra, int extra_len, uint8_t** out_hash, int* out_len,
                          uint8_t* attempt_counter);                                                       /* signatures.rs:215 */
/* test hook: DirectHasher (hashers/direct.rs:20-78) with an explicit domain of 0..8 bytes.  what: 0 = crh (writes 32 bytes; out_bytes is
 * the XOF length it is keyed on), 1 = xof(domain, msg, out_bytes), 2 = hash = xof(domain, crh(domain, msg, out_bytes), out_bytes). */
bool celo_amd_direct_hasher(int what, const uint8_t* domain, int domain_len, const uint8_t* msg, int msg_len, int out_bytes, uint8_t* out);
/* test hook: CompositeHasher::hash(domain, msg, out_bytes) = Blake2Xs XOF of the Bowe-Hopwood CRH (hashers/composite.rs:88-97) */
bool celo_amd_composite_hash(const uint8_t* domain8, const uint8_t* msg, int msg_len, int out_bytes, uint8_t* out);
/* test hook: try-and-increment with an explicit 8-byte domain; out48 = compressed G1 point */
bool celo_amd_hash_to_g1(bool composite, bool cip22, const uint8_t* domain8, const uint8_t* msg, int msg_len, const uint8_t* extra,
                         int extra_len, uint8_t* out48, int* out_attempt);
bool verify_signature(const PublicKey* pk, const uint8_t* msg, int msg_len, const uint8_t* extra, int extra_len, const Signature* sig,
                      bool should_use_composite, bool should_use_cip22, bool* out_verified);               /* signatures.rs:244 */
bool verify_pop(const PublicKey* pk, const uint8_t* msg, int msg_len, const Signature* sig, bool* out_verified); /* signatures.rs:407 */
bool batch_verify_signature(const MessageFFI* messages, size_t messages_len, bool should_use_composite, bool should_use_cip22,
                            bool* verified);                                                               /* signatures.rs:290 */
bool batch_verify_strict(const BatchMessageFFI* batches, size_t batches_len, bool should_use_composite, bool should_use_cip22,
                         bool* out_results);                                                               /* signatures.rs:343 */

/* snark (crates/bls-snark-sys/src/snark/) */
typedef struct EpochBlockFFI {                 /* snark/epoch_block.rs:109-127, passed BY VALUE */
  uint16_t index; uint8_t round;
  const uint8_t* epoch_entropy;                /* 16 bytes or NULL */
  const uint8_t* parent_entropy;               /* 16 bytes or NULL */
  const uint8_t* pubkeys;                      /* pubkeys_num * 96 bytes, compressed G2 */
  size_t pubkeys_num; uint32_t maximum_non_signers; size_t maximum_validators;
} EpochBlockFFI;
bool verify(const uint8_t* vk, uint32_t vk_len, const uint8_t* proof, uint32_t proof_len, EpochBlockFFI first_epoch,
            EpochBlockFFI last_epoch);                                                                       /* snark/mod.rs:23 */
bool encode_epoch_block_to_bytes_cip22(unsigned short index, unsigned char round, const uint8_t* epoch_entropy,
                                       const uint8_t* parent_entropy, unsigned int maximum_non_signers, unsigned int maximum_validators,
                                       const PublicKey* const* added_public_keys, int added_public_keys_len, uint8_t** out_bytes,
                                       int* out_len, uint8_t** out_extra_data_bytes, int* out_extra_data_len);  /* snark/epoch_block.rs:17 */
bool encode_epoch_block_to_bytes(unsigned short index, unsigned int maximum_non_signers, const PublicKey* const* added_public_keys,
                                 int added_public_keys_len, uint8_t** out_bytes, int* out_len);              /* snark/epoch_block.rs:69 */

/* GPU verification core: what verify_signature / verify_pop (signatures.rs:244,407) compute once the message has been
 * hashed to G1 — e(sig, -g2) * e(H(m), pk) == 1 (crates/bls-crypto/src/bls/public.rs:94-120).  message_hash_xy: affine
 * G1 point, 12 u64, arkworks Montgomery limbs. */
bool celo_amd_verify_hash(const PublicKey* pk, const uint64_t* message_hash_xy, const Signature* sig, bool* out_verified);
/* The BLS12-377 G2 generator (affine, 24 u64, arkworks Montgomery limbs). */
bool celo_amd_g2_generator(uint64_t out_xy[24]);

#ifdef __cplusplus
}
#endif
#endif
