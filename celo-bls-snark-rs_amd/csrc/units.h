// Every function that one translation unit defines and another calls, declared once.  The units are linked into a shared library, where an
// undefined celo:: symbol is no link error: a prototype re-typed at the caller that drifts from its definition builds cleanly and fails at
// load time, or at the first call.  So no .hip file declares another unit's function itself: callers and the defining unit include this header,
// a member of MsmApi / MsmAuxApi that is defined differently does not compile.  A plain function defined differently DOES compile (it is an
// overload, and the declared one stays undefined): the guard for those is tests/test_abi_symbols.py, which checks that the library is left
// with no undefined celo:: symbol.
// Light on purpose (capi.hip and the seam_*.hip units include it): no field, curve or kernel header; the groups, fields and handles are opaque here.
#pragma once
#include <cstddef>
#include <cstdint>
#include "runtime.h"

namespace celo {
struct G1_377; struct G2_377; struct G_761;      // msm.h: the three group configurations
struct P377; struct P253; struct P761;           // fp_consts.h
template <class P> struct Fp;                    // fp.h
typedef Fp<P377> Fr761;                          // the scalar field of BW6-761 is the base field of BLS12-377 (ntt.h)
typedef Fp<P253> Fr377;                          // the scalar field of BLS12-377
struct FixedTable;                               // msm_fixed.h: a key's fixed-base tables
struct ProvingKey;                               // unit_prover.hip: a loaded Groth16 proving key (fixed-base tables of its four queries)
struct R1cs;                                     // unit_r1cs.hip: constraint matrices on the device
struct VerifyingKey;                             // groth16_verify_unit.h: a loaded Groth16 verifying key (its input bases' window tables)
struct G16Bw6; struct G16Bls;                    // groth16_verify.h: the two curves of the Groth16 verifier
struct WireConsts;                               // wire.h
struct EdPoint;                                  // pedersen.h
struct BvJob { BatchRun keys, sigs; };           // unit_batchverify.hip: the chained Batch::verify in three steps

// ---- the MSM of group G (msm_unit.h holds the definitions; unit_<group>.hip and unit_<group>_aux.hip instantiate them).  Two templates because
// each group is built as two translation units: the halves own separate engine pools and separate "last call" records.
template <class G> struct MsmApi {
  // flags: bit 0 = bases vouched to lie in the prime-order subgroup, bit 1 = rows (0, 1) are the identity (the prover's queries)
  static int host(const uint64_t* b, const uint8_t* inf, const uint64_t* s, size_t n, int flags, uint64_t* out);
  static int dev(const void* b, const void* inf, const void* s, size_t n, int subgroup, uint64_t* out, void* st);
  static int multi_host(const int* devs, int nd, const uint64_t* b, const uint8_t* inf, const uint64_t* s, size_t n, uint64_t* out);
  static int multi_dev(const int* devs, int nd, const void* const* b, const void* const* inf, const void* const* s, const size_t* n_per, uint64_t* out);
  static int multi_windows(const int* devs, int nd, int resident, const void* const* b, const void* const* inf, const void* const* s, size_t n, int subgroup,
                           uint64_t* out);
  static int window_shard(const void* b, const void* inf, const void* s, size_t n, int subgroup, int shard, int nshards, uint64_t* out_xyzz, int* bit_lo, void* st);
  static int join_windows(const uint64_t* xyzz, const int* bit_lo, int nshards, uint64_t* out);
  // fixed-base form: per-key tables.  resident = 1: DEVICE pointers
  static int fixed_build(const void* b, const void* inf, size_t n, int resident, int cf, FixedTable** out);
  static int fixed_run(const FixedTable* T, const void* s, size_t n_sc, int resident, uint64_t* out, void* st);
  static int selftest_accumulate(const uint64_t* gen_xy, uint32_t runs, uint32_t len, uint32_t seed, uint32_t check, int chunked, uint32_t* differ);
  static void big_timings(float ms[5], int cfg[3]);
  static void big_set_c(int c);
};
template <class G> struct MsmAuxApi {
  static int batch_host(const uint64_t* b, const uint8_t* inf, const uint64_t* s, const uint32_t* off, size_t m, int subgroup_points, uint64_t* out);
  static int batch_begin(const void* b, const void* inf, const void* s, int resident, const uint32_t* off, size_t m, int subgroup_points, BatchRun* run);
  static void batch_end(BatchRun* run, int drained);
  static int timings(float ms[5], int cfg[3]);
  static void note_big_call();
  static int set_c(int c);
  static int gen_points(void* d_out, size_t n, uint64_t seed, const uint64_t* gen_xy, size_t ngens, uint32_t per, void* st);
  static int sum_jac(const uint64_t* jac, size_t k, uint64_t* out);
};
extern template struct MsmApi<G1_377>; extern template struct MsmApi<G2_377>; extern template struct MsmApi<G_761>;
extern template struct MsmAuxApi<G1_377>; extern template struct MsmAuxApi<G2_377>; extern template struct MsmAuxApi<G_761>;
int fixed_table_release(FixedTable* T);          // unit_g1_377.hip: the group-agnostic ends of a fixed-base handle
int fixed_table_info(const FixedTable* T, size_t* n, int* window_bits, int* windows, size_t* table_bytes, float* build_ms);

// ---- NTT and witness map over FR = Fr761 / Fr377 (unit_ntt.hip, unit_prover.hip)
template <class FR> int ntt_run(uint64_t* data, unsigned log_n, const uint64_t* omega, const uint64_t* coset, int coset_after, const uint64_t* scale, int dev, void* stream);
int ntt_timings(float ms[4], int* passes);
template <class FR>
int witness_map_run(uint64_t* a, uint64_t* b, uint64_t* c, unsigned log_n, const uint64_t* omega, const uint64_t* omega_inv, const uint64_t* coset,
                    const uint64_t* coset_inv, const uint64_t* n_inv, const uint64_t* z_inv, int out_canonical, int dev, void* stream);

// ---- pairing (unit_pairing.hip, unit_pairing761.hip, unit_pairing377_wide.hip)
int pairing_run_377(const uint64_t* g1, const uint8_t* inf1, const uint64_t* g2, const uint8_t* inf2, const uint32_t* offsets, size_t m, uint8_t* is_one, uint64_t* gt, int mode);
int pairing_run_761(const uint64_t* g1, const uint8_t* inf1, const uint64_t* g2, const uint8_t* inf2, const uint32_t* offsets, size_t m, uint8_t* is_one, uint64_t* gt, int mode);
int pairing_stage_377(uint32_t k, size_t m, PairingStage* st);
// kernel_ms (optional, here and below): the time the call's own "last call" record reports for THIS call, handed to the caller
int pairing_run_staged_377(PairingStage* st, const uint32_t* offsets, size_t m, uint8_t* is_one, float* kernel_ms = nullptr);
int pairing_timings_377(float ms[4]);
int pairing_stage_761(uint32_t k, size_t m, PairingStage* st);
int pairing_run_staged_761(PairingStage* st, const uint32_t* offsets, size_t m, uint8_t* is_one, float* kernel_ms = nullptr);
// the staged entry points of a curve's engine as one type (runtime.h StagedProduct, groth16_verify_unit.h G16Dev)
struct Pairing377 {
  static int stage(uint32_t k, size_t m, PairingStage* st) { return pairing_stage_377(k, m, st); }
  static int run_staged(PairingStage* st, const uint32_t* off, size_t m, uint8_t* is_one, float* ms) { return pairing_run_staged_377(st, off, m, is_one, ms); }
};
struct Pairing761 {
  static int stage(uint32_t k, size_t m, PairingStage* st) { return pairing_stage_761(k, m, st); }
  static int run_staged(PairingStage* st, const uint32_t* off, size_t m, uint8_t* is_one, float* ms) { return pairing_run_staged_761(st, off, m, is_one, ms); }
};
void final_exp_w3_377(const uint32_t* prod, uint8_t* is_one, uint64_t* gt, uint32_t m, hipStream_t s);
void final_exp_w2_377(const uint32_t* prod, uint8_t* is_one, uint64_t* gt, uint32_t m, hipStream_t s);

// ---- chained Batch::verify (unit_batchverify.hip)
int batch_verify_377_run(const void* pk_xy, const void* pk_inf, const void* sig_xy, const void* sig_inf, const void* exponents, int resident, const uint32_t* offsets,
                         const void* hash_xy, const void* hash_inf, const uint64_t neg_g2_xy[24], size_t m, uint8_t* out_ok);
int draw_exponents_run(const uint32_t key[8], const uint32_t* offsets, size_t m, uint64_t* out);
int bv_begin_keys(BvJob* j, const void* pk_xy, const void* pk_inf, const void* exponents, int resident, const uint32_t* offsets, size_t m);
int bv_begin_sigs(BvJob* j, const void* sig_xy, const void* sig_inf, const void* exponents, int resident, const uint32_t* offsets, size_t m);
int bv_finish(BvJob* j, int begun_ok, const void* hash_xy, const void* hash_inf, int resident, const uint64_t neg_g2_xy[24], size_t m, uint8_t* out_ok);
int bv_mirror_scatter(int words, const uint64_t* up_xy, const uint8_t* up_inf, const uint32_t* slots, uint64_t* mirror_xy, uint8_t* mirror_inf, size_t k, hipStream_t stream);
int bv_mirror_gather(int words, const uint64_t* mirror_xy, const uint8_t* mirror_inf, const uint32_t* slots, uint64_t* out_xy, uint8_t* out_inf, size_t n, hipStream_t stream);
int bv_draw_exponents(const uint32_t key[8], const uint32_t* d_offsets, size_t m, size_t tot, uint64_t* d_out, hipStream_t stream);

// ---- point decoding and normalisation (unit_wire.hip, unit_wire761.hip).  group 0 / 1: BLS12-377 G1 / G2, 2: BW6-761
int wire_decompress(int g2, const uint8_t* in, size_t n, int check, uint64_t* out, uint8_t* status, int dev, void* stream, float* kernel_ms = nullptr);
int wire377_decode(int g2, int compressed, const uint8_t* in, size_t n, int check, uint64_t* out, uint8_t* status, int dev, void* stream, float* kernel_ms = nullptr);
int wire377_launch_decode(int g2, int compressed, const uint8_t* d_in, size_t n, int check, uint64_t* d_out, uint8_t* d_st, hipStream_t stream);
int wire_normalize(int group, const uint64_t* jac, size_t n, uint64_t* out_xy, uint8_t* inf);
int wire_consts_device(WireConsts& out);
int wire_consts_warm();                          // the upload of wire_consts_device alone (first use on the calling thread's device), for units that do not see wire.h
float wire_last_ms();
int wire761_decode(int g2, int compressed, const uint8_t* in, size_t n, int check, uint64_t* out, uint8_t* status, int dev, void* stream);
// the serialized Groth16 proving key of curve 0 = BW6-761 / 1 = BLS12-377: the layout walk and the loader
int wire_key_layout(int curve, const uint8_t* bytes, size_t len, int form, uint64_t out[16]);
int wire_key_load(int curve, const uint8_t* bytes, size_t len, int form, int window_bits, ProvingKey** out_key, uint64_t* first_bad);
void wire761_last_timings(float ms[4]);
// the subgroup pass of the BW6-761 decoders and of check_points_bw6_761_*: 0 = the endomorphism form (k_endo761), 1 = the r P ladder (k_subgroup761)
int wire761_set_subgroup_test(int form);
int wire761_subgroup_test();
void wire761_launch_ladder(uint64_t* d_rows, uint8_t* d_st, size_t n, hipStream_t s);
// ---- compressed BLS12-377 keys decoded once per distinct byte string (unit_dedup.hip; dedup.h).  As wire_decompress, plus out_rep (n
// representatives, or NULL; a device pointer with dev) and out_decoded (the number of keys that went through the decoder; a host pointer, or
// NULL).  The stage times go to the call's own record (key_dedup_last); a composed caller times the whole of it with its own event pair
int wire_decompress_dedup(int g2, const uint8_t* in, size_t n, int check, uint64_t* out, uint8_t* status, uint32_t* out_rep, uint64_t* out_decoded, int dev, void* stream);
int key_dedup_set(int on, int slack_log, int max_probes);       // on: -1 the rule (dedup.h key_dedup_pick), 0 never, 1 always - for the composed callers
int key_dedup_get(int out[3]);                   // on, slack_log, max_probes as they stand (the defaults resolved)
bool key_dedup_use(size_t n);                   // what the switch says for a composed call with n keys
int key_dedup_last(uint64_t counts[2], float ms[4]);
// ---- bulk validation of affine rows (unit_check.hip; check.h).  cg 0 / 1: BLS12-377 G1 / G2, 2 / 3: BW6-761 G1 / G2; level 1: the curve
// equation, 2: and the subgroup.  dev: xy, inf and status are device pointers, the work runs on `stream`; first_bad is a host pointer (may be NULL)
int check_points(int cg, const uint64_t* xy, const uint8_t* inf, size_t n, int level, uint8_t* status, uint64_t* first_bad, int dev, void* stream);
float check_points_last_ms();
// k_endo761 on the rows at status 0: status 3 where [a]P + [b]phi(P) != O, and that row of d_zero_rows (may be d_rows itself, or NULL) zeroed
void check761_launch_endo(int g2, const uint64_t* d_rows, uint64_t* d_zero_rows, uint8_t* d_st, size_t n, hipStream_t s);
// ---- point encoding and the key / proof writers (unit_wire_encode.hip).  group as above; compressed: 1 = x with the sign flag, 0 = x || y
int wire_encode(int group, int compressed, const uint64_t* rows, const uint8_t* inf, size_t n, uint8_t* out, uint8_t* status, int dev, void* stream);
float wire_encode_last_ms();
void wire_encode_key_timings(float ms[3]);
int wire_key_size(int curve, size_t n_inputs, size_t n_vars, size_t n_h, int form, int vk_only, uint64_t* len);
int wire_key_serialize(int curve, const uint64_t* vk, size_t n_inputs, const uint64_t* rows, size_t n_vars, size_t n_h, int form, uint8_t* out, size_t cap,
                       uint64_t* out_len, uint64_t* first_bad);
int wire761_proof_serialize(const uint64_t* a_xyz, const uint64_t* b_xyz, const uint64_t* c_xyz, uint8_t* out);

// ---- hash to G1 (unit_hash.hip; the composite hasher's generator table is seam_hash.hip's).  mode, for both groups: 0 direct, 1 the CIP22
// tail (msgs are the inner CRHs), 2 composite, 3 composite CIP22: one CRH per message (pedersen_crh_run), then the tail over the 48-byte inners
// dev = 1 (G1 and the CRH): the bytes, rows and attempts are DEVICE pointers and the work is enqueued on the caller's stream; the offsets are host
// arrays in both forms, and both return after the work has drained.  kernel_ms: what celo_amd_hash_last_ms reports for the call - for mode 3 the
// tail's round loop alone, as the record (the CRH's time is overwritten there)
int hash_to_g1_direct_run(const uint8_t* domain, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* extras, const uint64_t* extra_off, size_t n, uint64_t* out_xy,
                          uint8_t* attempts, int mode, int dev = 0, void* stream = nullptr, float* kernel_ms = nullptr);
int pedersen_crh_run(const uint8_t* msgs, const uint64_t* msg_off, size_t n, uint8_t* out48, int dev = 0, void* stream = nullptr, float* kernel_ms = nullptr);
// ---- hash to G2 (unit_hash.hip): the same round loop, rows of 24 limbs; compat 0 / 1: the flags as the XOF gives them / the deployed remap
int hash_to_g2_run(const uint8_t* domain, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* extras, const uint64_t* extra_off, size_t n, int compat,
                   uint64_t* out_xy, uint8_t* attempts, int mode);
int hash_to_g2_one_run(const uint8_t* domain, const uint8_t* msg, size_t mlen, const uint8_t* extra, size_t elen, int mode, int compat, uint64_t* out_xy, int* attempt);
int hash_g2_set_lane_budget_log(int log);
void hash_g2_last_split(float ms[2]);
float hash_last_ms();
int hash_last_rounds();
// unit_hash_lanes.hip: k_pedersen_crh_lanes on st, `grid` workgroups of CRH_BLOCK lanes with L lanes per message (L = 2 .. 256; 64 KB of dynamic LDS)
void crh_lanes_launch(uint32_t grid, hipStream_t st, const EdPoint* gens, const uint8_t* msgs, const uint64_t* off, uint8_t* out, uint32_t n, uint32_t L);
int crh_set_lanes(int lanes);                    // lanes per message of the CRH kernel: 0 = the rule (pedersen.h crh_pick_lanes), else 1, 2, 4 .. 256
int crh_last_lanes();                            // the width the last CRH kernel ran with
const EdPoint* celo_composite_gens(size_t* count);

// ---- batched fixed-base scalar multiplication and Groth16 setup (unit_setup.hip)
int fixed_base_mul(int group, const uint64_t* gen, const void* scalars, size_t n, void* out_xy, void* inf, int dev, void* stream);
int fixed_base_set_window(int c);
template <class F>                               // F = Fp<P761> (BW6-761, both groups) or Fp<P377> (BLS12-377 G1); scalar_bits: of the group order
int fixed_base_tables(const uint64_t* gens, const uint8_t* inf, size_t n, int scalar_bits, int c, uint32_t* d_table, uint8_t* d_tinf, hipStream_t s);
void setup_last_timings(float ms[8]);
int groth16_setup(int curve, const uint64_t* qa, const uint64_t* qb, const uint64_t* qc, size_t n_vars, size_t n_inputs, const uint64_t* zt, const uint64_t* tau, size_t n_h,
                  const uint64_t* toxic, const uint64_t* g1_xy, const uint64_t* g2_xy, int window_bits, uint64_t* out_vk, uint64_t* out_rows, ProvingKey** out_key);
int groth16_setup_r1cs(int curve, const R1cs* r, unsigned log_n, const uint64_t* omega, const uint64_t* tau, const uint64_t* toxic, const uint64_t* g1_xy,
                       const uint64_t* g2_xy, int window_bits, uint64_t* out_vk, uint64_t* out_rows, ProvingKey** out_key);

// ---- batched variable-base scalar multiplication and batched signing (unit_varbase.hip).  group 0 / 1: BLS12-377 G1 / G2, 2: BW6-761
int scalar_mul_batch(int group, int subgroup, const void* xy, const void* inf, const void* scalars, size_t n_scalars, size_t n, void* out_xy, void* out_inf, int dev,
                     void* stream);
int scalar_mul_set_window(int c);
int scalar_mul_set_chunk_rows(uint32_t rows);
void scalar_mul_last_ms(float ms[4]);
int sign_batch_377(const uint64_t* sk, size_t n_sk, const uint8_t* domain, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* extras, const uint64_t* extra_off,
                   size_t n, int mode, uint8_t* out_sig48, uint8_t* attempts);

// ---- masked segmented point sums: the aggregated key of every seal from its signer bitmap (unit_seals.hip).  group 0 / 1: BLS12-377 G1 / G2
int aggregate_by_bitmap(int group, const void* xy, const void* inf, const uint32_t* offsets, size_t n_sets, const void* bits, size_t m, void* out_xy, void* out_inf,
                        void* out_count, int dev, void* stream);
int aggregate_set_lanes(int lanes);
int aggregate_set_complement(int mode);
// the last aggregate_by_bitmap / verify_aggregated_seals call: path (-1 for a bare sum), the lane width used, the stage times
void seals_last(int* path, int* lanes, float ms[8]);
int verify_aggregated_seals_377(const uint64_t* pk_xy, const uint8_t* pk_inf, const uint32_t* offsets, size_t n_sets, const uint8_t* bits, const uint32_t* min_signers,
                                const uint8_t* domain, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* extras, const uint64_t* extra_off, int hash_mode,
                                const uint8_t* sig48, const uint64_t neg_g2_xy[24], size_t m, int mode, const uint32_t* key, uint8_t* out_ok, uint8_t* out_status);

// ---- epoch blocks to bytes, public inputs and verdicts (unit_epoch.hip; epoch.h).  nb blocks: the per-block fields and the offsets are
// host arrays in both forms; keys (keys_form 0: 96-byte compressed G2 keys, 1: affine rows of 24 u64 with keys_inf or NULL) and the entropies
// (nb x 16 bytes or NULL) are device pointers with dev = 1.  The layout of celo_epoch_blocks (include/celo_bls_amd.h)
struct EpochBlocks {
  const uint16_t* index; const uint8_t* round; const uint32_t* max_non_signers; const uint32_t* max_validators;
  const uint8_t* epoch_entropy; const uint8_t* parent_entropy; const void* keys; const uint8_t* keys_inf; const uint32_t* key_off; int keys_form;
};
int epoch_encoded_size(int kind, uint64_t n_keys, uint64_t max_validators, uint64_t* bytes);
int epoch_encode_blocks(const EpochBlocks* b, size_t nb, int kind, const uint64_t* out_off, void* out, void* extras, void* status, int dev, void* stream);
int epoch_public_inputs(const EpochBlocks* first, const EpochBlocks* last, size_t m, void* out_inputs, void* out_status, int dev, void* stream);
int verify_epoch_proofs(const VerifyingKey* vk, const uint8_t* proofs, const EpochBlocks* first, const EpochBlocks* last, size_t m, int mode, const uint32_t* key,
                        uint8_t* out_ok, uint8_t* out_status);
void epoch_last(float ms[8]);
// for unit_transitions.hip: the refusals of a set of blocks (2, no device touched), and the blocks on the device up to their packed bytes of
// kind `kind` (block b at out_off[b]; a block of length 0 is left out), enqueued on cs.stream(); times into log in the order of epoch_last
struct EpochStaged {
  const uint16_t* index; const uint8_t* round; const uint32_t* mns; const uint32_t* key_off; const uint8_t* ee; const uint8_t* pe;   // the fields, nb each
  const uint64_t* rows; const uint8_t* inf;      // key_off[nb] decoded keys (24 u64 each) and their identity flags
  const uint8_t* status;                         // nb: 1 = a key of the block does not decode or lies outside G2
  uint8_t* bytes;                                // out_off[nb] bytes
};
int epoch_refuse_blocks(const EpochBlocks& b, size_t nb, bool need_round);
int epoch_stage_bytes(CallScope& cs, EvLog& log, const EpochBlocks& b, size_t nb, int kind, const uint64_t* out_off, EpochStaged* out);

// ---- chains of epoch transitions to verdicts (unit_transitions.hip; transitions.h)
int verify_epoch_transitions(const EpochBlocks* blocks, size_t nb, const uint32_t* chain_off, size_t n_chains, const uint8_t* bits, const uint8_t* sig48,
                             const uint8_t* domain, const uint64_t neg_g2_xy[24], int mode, uint8_t* out_ok, uint8_t* out_status, uint8_t* out_chain_ok, uint8_t* out_crh,
                             uint8_t* out_attempts, uint64_t* out_asig_xy, uint8_t* out_asig_inf);
void transitions_last(int* path, float ms[8]);

// ---- constraint matrices (unit_r1cs.hip)
int r1cs_load(int curve, size_t m, size_t n_vars, size_t n_inputs, const uint64_t* const row_ptr[3], const uint32_t* const col[3], const uint64_t* const val[3],
              const uint64_t nnz[3], R1cs** out, uint64_t* first_bad);
int r1cs_info(const R1cs* r, uint64_t out[8]);
void r1cs_free(R1cs* r);
void r1cs_shape(const R1cs* r, int* curve, int* device, size_t* m, size_t* n_vars, size_t* n_inputs);
int r1cs_rows(const R1cs* r, const uint64_t* z, unsigned log_n, uint64_t* oa, uint64_t* ob, uint64_t* oc, int dev, void* stream);
int r1cs_check(const R1cs* r, const uint64_t* z, int64_t* first_unsatisfied);
int r1cs_qap_at_tau(const R1cs* r, unsigned log_n, const uint64_t* omega, const uint64_t* tau, uint64_t* oa, uint64_t* ob, uint64_t* oc, uint64_t* ozt, int dev, void* stream);
void r1cs_note_ms(int slot, float v);
void r1cs_last_timings(float ms[8]);

// ---- Groth16 prover (unit_prover.hip).  curve 0 = BW6-761, 1 = BLS12-377
int groth16_prove_761_run(const uint64_t* a_query, size_t na, const uint64_t* b_g2_query, size_t nb, const uint64_t* h_query, size_t nh, const uint64_t* l_query, size_t nl,
                          const uint64_t* alpha_g1, const uint64_t* beta_g2, const uint64_t* assignment, size_t n_assign, size_t n_aux, const uint64_t* h, size_t n_h,
                          uint64_t* out_a, uint64_t* out_b, uint64_t* out_c);
int groth16_prove_377_run(const uint64_t* a_query, size_t na, const uint64_t* b_g2_query, size_t nb, const uint64_t* h_query, size_t nh, const uint64_t* l_query, size_t nl,
                          const uint64_t* alpha_g1, const uint64_t* beta_g2, const uint64_t* assignment, size_t n_assign, size_t n_aux, const uint64_t* h, size_t n_h,
                          uint64_t* out_a, uint64_t* out_b, uint64_t* out_c);
int groth16_key_load(int curve, const uint64_t* a_query, size_t na, const uint64_t* b_g2_query, size_t nb, const uint64_t* h_query, size_t nh, const uint64_t* l_query,
                     size_t nl, const uint64_t* alpha_g1, const uint64_t* beta_g2, int window_bits, ProvingKey** out);
int groth16_key_load_dev(int curve, const uint64_t* d_a, const uint8_t* d_ainf, size_t na, const uint64_t* d_b, const uint8_t* d_binf, size_t nb, const uint64_t* d_h,
                         const uint8_t* d_hinf, size_t nh, const uint64_t* d_l, const uint8_t* d_linf, size_t nl, const uint64_t* a0, const uint64_t* b0,
                         const uint64_t* alpha_g1, const uint64_t* beta_g2, int window_bits, ProvingKey** out);
void groth16_key_free(ProvingKey* k);
int groth16_prove_keyed(const ProvingKey* k, const uint64_t* assignment, size_t n_assign, size_t n_aux, const uint64_t* h, size_t n_h, uint64_t* out_a, uint64_t* out_b,
                        uint64_t* out_c);
// z_mode 0: z is a host pointer; 1: a device pointer the call leaves as it is; 2: a device pointer the call may overwrite
int groth16_prove_r1cs(const ProvingKey* k, const R1cs* r, const uint64_t* z, int z_mode, unsigned log_n, const uint64_t* omega, const uint64_t* omega_inv,
                       const uint64_t* coset, const uint64_t* coset_inv, const uint64_t* n_inv, const uint64_t* z_inv, uint64_t* out_a, uint64_t* out_b, uint64_t* out_c);
void groth16_key_shape(const ProvingKey* k, int* curve, size_t rows[4]);

// ---- the HashToBits circuit of the hash-helper proof over Fr(BLS12-377) (unit_hashbits.hip; hashbits.h).  The first three and
// hashbits_assignment_host are pure host functions (no device needed)
int hashbits_sizes(size_t m, uint64_t out[8]);
int hashbits_write_csr(size_t m, uint64_t* const row_ptr[3], uint32_t* const col[3], uint64_t* const val[3]);
int hashbits_assignment_host(const uint8_t* rows48, size_t m, int bit_order, uint64_t* z);
int hashbits_r1cs_load(size_t m, R1cs** out);
int hashbits_assignment(const uint8_t* rows48, size_t m, int bit_order, uint64_t* z, int dev, void* stream);
int hashbits_public_inputs(const uint8_t* rows48, size_t n_proofs, size_t m, int bit_order, uint64_t* out, int dev, void* stream);
int hash_helper_prove(const ProvingKey* k, const R1cs* r, const uint8_t* rows48, size_t m, int bit_order, unsigned log_n, const uint64_t* omega, const uint64_t* omega_inv,
                      const uint64_t* coset, const uint64_t* coset_inv, const uint64_t* n_inv, const uint64_t* z_inv, uint64_t* out_a, uint64_t* out_b, uint64_t* out_c,
                      uint64_t* out_inputs);
void hash_helper_last(float ms[8]);

// ---- Groth16 verification of many proofs under one key (groth16_verify_unit.h holds the definitions; unit_groth16_verify.hip instantiates
// them for C = G16Bw6 and unit_groth16_verify377.hip for C = G16Bls).  Rows: affine arkworks limbs, C::G1W / C::G2W u64 each
// the most public inputs (n_abc - 1) a loader takes: the narrow loaders of both curves, and the wide loaders of BLS12-377.  groth16_verify.h's
// G16_MAX_INPUTS / G16_MAX_INPUTS_WIDE (what the parse and the kernels' bounds use) are held equal to them by groth16_verify_unit.h
constexpr size_t VK_MAX_INPUTS = 64, VK_MAX_INPUTS_WIDE = 1024;
template <class C> struct G16Api {
  static int vk_load(const uint64_t* alpha_g1, const uint64_t* beta_g2, const uint64_t* gamma_g2, const uint64_t* delta_g2, const uint64_t* gamma_abc_g1, size_t n_abc,
                     VerifyingKey** out, size_t max_inputs = VK_MAX_INPUTS);
  static int vk_load_serialized(const uint8_t* bytes, size_t len, VerifyingKey** out, size_t max_inputs = VK_MAX_INPUTS);
  static int verify(const VerifyingKey* vk, const uint64_t* a_xy, const uint8_t* a_inf, const uint64_t* b_xy, const uint8_t* b_inf, const uint64_t* c_xy,
                    const uint8_t* c_inf, const uint8_t* proofs, const uint64_t* inputs, size_t m, int mode, const uint32_t* key, uint8_t* out_ok);
  // the serialized entry with the inputs (m x n_in x N64 u64, canonical) and one status byte per proof already on the DEVICE (unit_epoch.hip): a
  // proof whose byte is set is handled as one that does not decode.  out_refused (m host bytes, may be NULL): 1 where the proof took part in
  // no product - the caller's byte, a point that does not decode or lies outside its subgroup, an input out of range
  static int verify_staged(const VerifyingKey* vk, const uint8_t* proofs, const uint64_t* d_inputs, const uint8_t* d_pre_status, size_t m, int mode, const uint32_t* key,
                           uint8_t* out_ok, uint8_t* out_refused);
};
extern template struct G16Api<G16Bw6>; extern template struct G16Api<G16Bls>;
// what the two curves share (unit_groth16_verify.hip): the handles that are alive, the last call's record, the exponent draw
void groth16_vk_adopt(VerifyingKey* vk);
bool groth16_vk_is_live(const VerifyingKey* vk, int curve);
int groth16_vk_inputs(const VerifyingKey* vk, int curve);        // the number of public inputs of a live handle of `curve`, or -1
int groth16_vk_release(VerifyingKey* vk);
void groth16_verify_note(int path, int window_bits, const float ms[8], int lanes, int n_inputs);
int groth16_draw_exponents_run(const uint32_t key[8], size_t m, uint64_t* out);
int groth16_verify_last(int* path, int* window_bits, float ms[8]);
int groth16_set_input_lanes(int lanes);          // lanes per input sum of a BLS12-377 call: 0 = the rule (groth16_verify.h g16_pick_lanes), else 1, 2, 4 .. 256
int groth16_input_lanes();                       // the forced width, or 0
int groth16_inputs_last(int* lanes, int* n_inputs);
// generate_hash_helper's verifier in one call (unit_hashbits.hip): rows to the device, canonical inputs made there, verify_staged on them
int hash_helper_verify(const VerifyingKey* vk, const uint8_t* rows48, size_t n_proofs, size_t m, int bit_order, const uint8_t* proofs, int mode, const uint32_t* key,
                       uint8_t* out_ok);
int wire377_proof_serialize(const uint64_t* a_xyz, const uint64_t* b_xyz, const uint64_t* c_xyz, uint8_t* out);      // unit_wire_encode.hip

int ubench_fp_run(float out[9]);                 // unit_ubench.hip
}  // namespace celo
