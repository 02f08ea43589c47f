/* celo_bls_amd.h — C ABI of the MI355X (gfx950) MSM / pairing / NTT hot path.
 *
 * "Seam B" of SURVEY.md §8b: the thin extern "C" shim that replaces the arkworks call sites
 * of celo-bls-snark-rs.  Each entry cites the reference interface it stands in for.
 *
 * Conventions (identical to what a Rust shim over arkworks 0.1 types would hand over):
 *   - limbs little-endian u64; base-field elements in arkworks Montgomery form
 *     (R = 2^384 for BLS12-377 Fq, 2^768 for BW6-761 Fq); Fq2 = c0 || c1;
 *   - scalars canonical (Fr::into_repr()): 4 x u64 (BLS12-377 Fr) / 6 x u64 (BW6-761 Fr), must be < r;
 *   - affine bases x || y, with an optional byte-per-point infinity array (NULL = none);
 *   - results: Jacobian (X, Y, Z) in Montgomery form, identity encoded Z = 0 — the in-memory
 *     layout of GroupProjective{x,y,z};
 *   - return 0 = ok, non-zero = device/runtime error (a caller maps it to `false` like
 *     crates/bls-snark-sys/src/lib.rs:21-27 convert_result_to_bool);
 *   - *_dev variants take DEVICE pointers (inputs already resident in HBM) and a hipStream_t
 *     (as void*; NULL = default stream); the result still lands in host memory.
 * Threading (the reference's callers are synchronous, re-entrant and multi-threaded -
 * crates/bls-snark-sys/src/cache.rs:5, signatures.rs:343-400): every function is synchronous and may be called from any host
 * thread at any time.  There is no global lock: each MSM / pairing / NTT call checks an engine instance (workspace, pinned
 * staging, its own non-blocking HIP stream) out of a per-device pool, so independent calls overlap on the GPU; single
 * pairing-product checks from concurrent threads are combined into shared launches.  Bulk decode / hash calls are serialised
 * among themselves only.  Several devices can be driven from one process: celo_amd_use_device() binds the calling thread to a
 * device, the msm_*_multi entry points shard one MSM over a device list internally.
 */
#ifndef CELO_BLS_AMD_H
#define CELO_BLS_AMD_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Selects the process's DEFAULT device: the one every host thread uses unless it bound itself to another with
 * celo_amd_use_device (HIP's current device is per thread; each entry point re-applies the right one on its calling thread).
 * Returns 0, or non-zero if there is no gfx950 device (100) or `device` is out of range (101).  Never calling it = device 0. */
int celo_amd_init(int device);
/* Binds the CALLING host thread to `device` for all its later calls (engines, tables and streams are per device). */
int celo_amd_use_device(int device);
/* Page-locked host memory for the arrays a caller hands to the host-pointer entry points (msm_<group>, msm_batch_<group>, ...): the
 * transfers of such a buffer run at the link's rate from the first call on and do not hold the calling thread (a pageable range is
 * pinned by the HIP runtime the first time it is copied from: DESIGN.md section 4 "Buffers the runtime has never seen" - 2^20 G1 terms
 * 4.6-4.9 ms per call from newly allocated vectors, 4.0-4.2 ms from reused or page-locked ones).  A wrapper that converts the caller's
 * points into limbs anyway writes them here.  Free with celo_amd_host_free; 0 on success. */
int celo_amd_host_alloc(size_t bytes, void** out);
int celo_amd_host_free(void* p);
/* Number of HIP devices visible to the process (at most 16 are used). */
int celo_amd_device_count(int* count);
/* "gfx950:..." string of the active device into buf; returns 0. */
int celo_amd_device_name(char* buf, size_t buflen);

/* ---- MSM.  Replaces VariableBaseMSM::multi_scalar_mul(&[GAffine], &[BigInt]) at
 *   crates/bls-crypto/src/bls/signature.rs:85  (G1, Signature::batch)
 *   crates/bls-crypto/src/bls/public.rs:61     (G2, PublicKey::batch)
 *   ark_groth16::create_proof_no_zk via crates/epoch-snark/src/api/prover.rs:78,112 (BW6-761 / BLS12-377 prover MSMs) */
int msm_bls12_377_g1(const uint64_t* bases_xy /* n*12 */, const uint8_t* inf, const uint64_t* scalars /* n*4 */, size_t n,
                     uint64_t out_xyz[18]);
int msm_bls12_377_g2(const uint64_t* bases_xy /* n*24 */, const uint8_t* inf, const uint64_t* scalars /* n*4 */, size_t n,
                     uint64_t out_xyz[36]);
int msm_bw6_761_g1(const uint64_t* bases_xy /* n*24 */, const uint8_t* inf, const uint64_t* scalars /* n*6 */, size_t n,
                   uint64_t out_xyz[36]);
int msm_bw6_761_g2(const uint64_t* bases_xy /* n*24 */, const uint8_t* inf, const uint64_t* scalars /* n*6 */, size_t n,
                   uint64_t out_xyz[36]);
int msm_bls12_377_g1_dev(const void* d_bases_xy, const void* d_inf, const void* d_scalars, size_t n, uint64_t out_xyz[18], void* stream);
/* The G1 MSM for bases the caller vouches to be elements of the prime-order subgroup G1 - what Signature::batch hands over
 * (crates/bls-crypto/src/bls/signature.rs:70-89: a Signature of the reference is one by construction - checked deserialisation
 * signature.rs:31-57, sign, sums) and what a Groth16 proving key holds.  Same result as msm_bls12_377_g1; the library may split every
 * scalar with the endomorphism phi(x, y) = (beta x, y) = -[x^2](x, y): n terms of 253 bits become 2 n terms of 127 bits - half the
 * windows, half the bucket reduction, half the final Horner chain (csrc/msm.h k_glv_expand, gls.h).  For a base outside the subgroup
 * the result is unspecified (use msm_bls12_377_g1, which is VariableBaseMSM on any curve point). */
int msm_bls12_377_g1_subgroup(const uint64_t* bases_xy, const uint8_t* inf, const uint64_t* scalars, size_t n, uint64_t out_xyz[18]);
int msm_bls12_377_g1_subgroup_dev(const void* d_bases_xy, const void* d_inf, const void* d_scalars, size_t n, uint64_t out_xyz[18], void* hip_stream);
/* Likewise for G2 and bases that are elements of the prime-order subgroup G2 - what PublicKey::batch hands over
 * (crates/bls-crypto/src/bls/public.rs:47-65: a PublicKey is one by construction): k = k0 + k1 x^2, [x^2]P = psi^2(P). */
int msm_bls12_377_g2_subgroup(const uint64_t* bases_xy, const uint8_t* inf, const uint64_t* scalars, size_t n, uint64_t out_xyz[36]);
int msm_bls12_377_g2_subgroup_dev(const void* d_bases_xy, const void* d_inf, const void* d_scalars, size_t n, uint64_t out_xyz[36], void* hip_stream);
int msm_bls12_377_g2_dev(const void* d_bases_xy, const void* d_inf, const void* d_scalars, size_t n, uint64_t out_xyz[36], void* stream);
int msm_bw6_761_g1_dev(const void* d_bases_xy, const void* d_inf, const void* d_scalars, size_t n, uint64_t out_xyz[36], void* stream);
int msm_bw6_761_g2_dev(const void* d_bases_xy, const void* d_inf, const void* d_scalars, size_t n, uint64_t out_xyz[36], void* stream);

/* ---- one MSM sharded over several devices of this process (index-range shards, no data-path collective;
 * the reference's callers are ONE process - crates/bls-snark-sys/src/signatures.rs:343, crates/epoch-snark/src/api/prover.rs:78).
 * devices[ndev]: device ordinals (a device may appear more than once: that many engines run on it concurrently); one host
 * thread per entry computes the partial sum of its contiguous slice on its device, the Jacobian partials (144 / 288 bytes
 * each) are folded on the host.  Same conventions and results as the single-device entry points.
 * _multi: HOST pointers, n terms cut into ndev equal index ranges.
 * _multi_dev: per-shard DEVICE pointers (shard d resident on devices[d]: d_bases[d], d_inf[d] or d_inf == NULL, d_scalars[d],
 * n_per[d] terms). */
int msm_bls12_377_g1_multi(const int* devices, int ndev, const uint64_t* bases_xy, const uint8_t* inf, const uint64_t* scalars, size_t n, uint64_t out_xyz[18]);
int msm_bls12_377_g2_multi(const int* devices, int ndev, const uint64_t* bases_xy, const uint8_t* inf, const uint64_t* scalars, size_t n, uint64_t out_xyz[36]);
int msm_bw6_761_g1_multi(const int* devices, int ndev, const uint64_t* bases_xy, const uint8_t* inf, const uint64_t* scalars, size_t n, uint64_t out_xyz[36]);
int msm_bw6_761_g2_multi(const int* devices, int ndev, const uint64_t* bases_xy, const uint8_t* inf, const uint64_t* scalars, size_t n, uint64_t out_xyz[36]);
int msm_bls12_377_g1_multi_dev(const int* devices, int ndev, const void* const* d_bases, const void* const* d_inf, const void* const* d_scalars, const size_t* n_per, uint64_t out_xyz[18]);
int msm_bls12_377_g2_multi_dev(const int* devices, int ndev, const void* const* d_bases, const void* const* d_inf, const void* const* d_scalars, const size_t* n_per, uint64_t out_xyz[36]);
int msm_bw6_761_g1_multi_dev(const int* devices, int ndev, const void* const* d_bases, const void* const* d_inf, const void* const* d_scalars, const size_t* n_per, uint64_t out_xyz[36]);
int msm_bw6_761_g2_multi_dev(const int* devices, int ndev, const void* const* d_bases, const void* const* d_inf, const void* const* d_scalars, const size_t* n_per, uint64_t out_xyz[36]);

/* ---- the same MSM partitioned by WINDOW instead of by index range ("alternative partitioning"): every listed
 * device holds ALL n bases and scalars and owns a contiguous range of the Pippenger windows - 1/ndev of the bucket additions, only its
 * windows' buckets to reduce, only its share of the final Horner chain; the ndev partial sums are joined on the host with the doublings
 * between the ranges (total = sum_g 2^bit(g) P_g).  This is the form that scales ONE MSM of up to ~2^21 terms over the GPUs of a node
 * (an index-range shard of 2^20 / 8 terms is bound by the pipeline's fixed latencies); it costs ndev-fold base memory, so the prover's
 * 2^24-term MSMs keep the index-range form above.  Same conventions and results as the single-device entry points; the _subgroup
 * forms take bases the caller vouches to be in the prime-order subgroup (see msm_bls12_377_g1_subgroup).
 * _multi_windows: HOST pointers (each shard stages the whole input onto its device).
 * _multi_windows_dev: d_bases[d] / d_inf[d] (or d_inf == NULL) / d_scalars[d] = the replica of the n terms resident on devices[d]. */
int msm_bls12_377_g1_multi_windows(const int* devices, int ndev, const uint64_t* bases_xy, const uint8_t* inf, const uint64_t* scalars, size_t n, uint64_t out_xyz[18]);
int msm_bls12_377_g1_subgroup_multi_windows(const int* devices, int ndev, const uint64_t* bases_xy, const uint8_t* inf, const uint64_t* scalars, size_t n, uint64_t out_xyz[18]);
int msm_bls12_377_g2_multi_windows(const int* devices, int ndev, const uint64_t* bases_xy, const uint8_t* inf, const uint64_t* scalars, size_t n, uint64_t out_xyz[36]);
int msm_bls12_377_g2_subgroup_multi_windows(const int* devices, int ndev, const uint64_t* bases_xy, const uint8_t* inf, const uint64_t* scalars, size_t n, uint64_t out_xyz[36]);
int msm_bw6_761_g1_multi_windows(const int* devices, int ndev, const uint64_t* bases_xy, const uint8_t* inf, const uint64_t* scalars, size_t n, uint64_t out_xyz[36]);
int msm_bw6_761_g2_multi_windows(const int* devices, int ndev, const uint64_t* bases_xy, const uint8_t* inf, const uint64_t* scalars, size_t n, uint64_t out_xyz[36]);
int msm_bls12_377_g1_multi_windows_dev(const int* devices, int ndev, const void* const* d_bases, const void* const* d_inf, const void* const* d_scalars, size_t n, uint64_t out_xyz[18]);
int msm_bls12_377_g1_subgroup_multi_windows_dev(const int* devices, int ndev, const void* const* d_bases, const void* const* d_inf, const void* const* d_scalars, size_t n, uint64_t out_xyz[18]);
int msm_bls12_377_g2_multi_windows_dev(const int* devices, int ndev, const void* const* d_bases, const void* const* d_inf, const void* const* d_scalars, size_t n, uint64_t out_xyz[36]);
int msm_bls12_377_g2_subgroup_multi_windows_dev(const int* devices, int ndev, const void* const* d_bases, const void* const* d_inf, const void* const* d_scalars, size_t n, uint64_t out_xyz[36]);
int msm_bw6_761_g1_multi_windows_dev(const int* devices, int ndev, const void* const* d_bases, const void* const* d_inf, const void* const* d_scalars, size_t n, uint64_t out_xyz[36]);
int msm_bw6_761_g2_multi_windows_dev(const int* devices, int ndev, const void* const* d_bases, const void* const* d_inf, const void* const* d_scalars, size_t n, uint64_t out_xyz[36]);
/* One rank's share of a window-partitioned MSM when the GPUs belong to DIFFERENT processes (one process per GPU, bench.py under
 * torch.distributed.run): the partial sum over the windows shard `shard` of `nshards` owns, as X || Y || ZZ || ZZZ (arkworks limbs:
 * 4 x 6 u64 for G1 of BLS12-377, 4 x 12 u64 for the other groups; ZZ = 0: the identity), and *bit_lo = the first scalar bit of the
 * shard's range.  The ranks exchange the fixed-size records (one all-gather) and every rank joins them with msm_*_join_windows. */
int msm_bls12_377_g1_window_shard_dev(const void* d_bases_xy, const void* d_inf, const void* d_scalars, size_t n, int subgroup, int shard, int nshards,
                                      uint64_t out_xyzz[24], int* bit_lo, void* hip_stream);
int msm_bls12_377_g2_window_shard_dev(const void* d_bases_xy, const void* d_inf, const void* d_scalars, size_t n, int subgroup, int shard, int nshards,
                                      uint64_t out_xyzz[48], int* bit_lo, void* hip_stream);
int msm_bw6_761_window_shard_dev(const void* d_bases_xy, const void* d_inf, const void* d_scalars, size_t n, int shard, int nshards,
                                 uint64_t out_xyzz[48], int* bit_lo, void* hip_stream);
/* total = sum_g 2^bit_lo[g] P_g over nshards records in shard order (bit_lo ascending); host-side, 64-bit limbs. */
int msm_bls12_377_g1_join_windows(const uint64_t* xyzz /* nshards x 24 */, const int* bit_lo, int nshards, uint64_t out_xyz[18]);
int msm_bls12_377_g2_join_windows(const uint64_t* xyzz /* nshards x 48 */, const int* bit_lo, int nshards, uint64_t out_xyz[36]);
int msm_bw6_761_join_windows(const uint64_t* xyzz /* nshards x 48 */, const int* bit_lo, int nshards, uint64_t out_xyz[36]);

/* ---- FIXED-BASE MSM: per-key tables for bases that stay while the scalars change - the Groth16 prover's queries
 * (crates/epoch-snark/src/api/prover.rs:78,112 hand the SAME Parameters to every proof; they are created once,
 * crates/epoch-snark/src/api/setup.rs:63-105).  _precompute builds, in the device memory of the calling thread's device, the table
 * T[j][i] = 2^(c j) P_i for the W = ceil((scalar bits + 1) / c) digit positions of a scalar (affine, device form: n W x 128 B for G1 of
 * BLS12-377, n W x 256 B for the other groups; window_bits c = 0 picks it from n, 16 <= c <= 22) and returns an opaque handle.
 * _fixed then computes sum_i k_i P_i for the first n_scalars <= n bases (the shorter side decides, as VariableBaseMSM zips) with ALL
 * signed c-bit digits in ONE set of 2^(c-1) buckets: one bucket reduction instead of W, no Horner chain over windows, and - c not being
 * bound to the 16 bits of the variable-base windows - fewer digits per scalar, i.e. fewer bucket additions (19 instead of 24 per
 * 377-bit scalar at c = 20).  Same result as msm_* (which stays VariableBaseMSM: nothing is cached behind its back).
 * A base may be flagged as the identity (inf); a base whose 2^(c j) multiple is the identity is handled.  The handle is bound to the
 * device it was built on (a call from a thread bound to another device returns 101) and may be used from several host threads at once.
 * Size limits (the pipeline's 32-bit run offsets): n W < 2^31 and n W NV < 2^32 with NV = the 2^15-bucket virtual windows of a c-bit digit
 * (1 at c = 16, then 3, 5, 9, 17, 33, 65 at c = 17 .. 22).  For the 377-bit scalars of BW6-761 that is n < 2^26.4 at c = 16, 2^25.9 at 17,
 * 2^25.3 at 18, 2^24.5 at 19 (a 2^24-term key, the prover's size, fits), 2^23.7 at 20, 2^22.8 at 21, 2^21.8 at 22; for the 253-bit scalars
 * of BLS12-377 about 1.5 times that.  window_bits = 0 starts from the measured optimum (20 / 21) and steps down until the limits hold;
 * an explicit window_bits that does not fit returns 2.
 * celo_amd_msm_fixed_info: the table's shape, its size in bytes and its build time (HIP events). */
int msm_bls12_377_g1_precompute(const uint64_t* bases_xy /* n*12 */, const uint8_t* inf, size_t n, int window_bits, void** out_handle);
int msm_bls12_377_g2_precompute(const uint64_t* bases_xy /* n*24 */, const uint8_t* inf, size_t n, int window_bits, void** out_handle);
int msm_bw6_761_g1_precompute(const uint64_t* bases_xy /* n*24 */, const uint8_t* inf, size_t n, int window_bits, void** out_handle);
int msm_bw6_761_g2_precompute(const uint64_t* bases_xy /* n*24 */, const uint8_t* inf, size_t n, int window_bits, void** out_handle);
int msm_bls12_377_g1_precompute_dev(const void* d_bases_xy, const void* d_inf, size_t n, int window_bits, void** out_handle);
int msm_bls12_377_g2_precompute_dev(const void* d_bases_xy, const void* d_inf, size_t n, int window_bits, void** out_handle);
int msm_bw6_761_g1_precompute_dev(const void* d_bases_xy, const void* d_inf, size_t n, int window_bits, void** out_handle);
int msm_bw6_761_g2_precompute_dev(const void* d_bases_xy, const void* d_inf, size_t n, int window_bits, void** out_handle);
int msm_bls12_377_g1_fixed(const void* handle, const uint64_t* scalars /* n_scalars*4 */, size_t n_scalars, uint64_t out_xyz[18]);
int msm_bls12_377_g2_fixed(const void* handle, const uint64_t* scalars /* n_scalars*4 */, size_t n_scalars, uint64_t out_xyz[36]);
int msm_bw6_761_g1_fixed(const void* handle, const uint64_t* scalars /* n_scalars*6 */, size_t n_scalars, uint64_t out_xyz[36]);
int msm_bw6_761_g2_fixed(const void* handle, const uint64_t* scalars /* n_scalars*6 */, size_t n_scalars, uint64_t out_xyz[36]);
int msm_bls12_377_g1_fixed_dev(const void* handle, const void* d_scalars, size_t n_scalars, uint64_t out_xyz[18], void* hip_stream);
int msm_bls12_377_g2_fixed_dev(const void* handle, const void* d_scalars, size_t n_scalars, uint64_t out_xyz[36], void* hip_stream);
int msm_bw6_761_g1_fixed_dev(const void* handle, const void* d_scalars, size_t n_scalars, uint64_t out_xyz[36], void* hip_stream);
int msm_bw6_761_g2_fixed_dev(const void* handle, const void* d_scalars, size_t n_scalars, uint64_t out_xyz[36], void* hip_stream);
int celo_amd_msm_fixed_release(void* handle);
int celo_amd_msm_fixed_info(const void* handle, size_t* n, int* window_bits, int* windows, size_t* table_bytes, float* build_ms);

/* ---- batched MSMs: m independent instances in one call; instance p owns points/scalars [offsets[p], offsets[p+1])
 * (offsets has m+1 entries), out_xyz holds m Jacobian results back to back.  This is the shape of Batch::verify
 * (crates/bls-crypto/src/bls/batch.rs:69,76 — one G2 and one G1 MSM over the batch's signers) when
 * batch_verify_strict (crates/bls-snark-sys/src/signatures.rs:343-400) is handed many batches; the reference loops over
 * them serially (signatures.rs:358).  Instances of up to 1024 points run on the batched kernels; a call with a larger instance
 * (or with no point at all) is processed one instance at a time on the large-MSM pipeline.
 * Dispatch of the batched kernels (reported by celo_amd_msm_last_timings): the window c is 3 bits, one more
 * from 128, 256, 512 and 1024 points in the call's largest instance; the number of windows is (bits + c) / c for bits = the
 * length of the longest scalar present.  A scalar is its container modulo 2^SCALAR_BITS (253 for BLS12-377, 377 for BW6-761):
 * container bits from there up are ignored - they neither change the result nor count towards `bits` - on the batched kernels as
 * on the large pipeline and on msm_<group>. */
int msm_batch_bls12_377_g1(const uint64_t* bases_xy, const uint8_t* inf, const uint64_t* scalars, const uint32_t* offsets, size_t m, uint64_t* out_xyz /* m*18 */);
int msm_batch_bls12_377_g2(const uint64_t* bases_xy, const uint8_t* inf, const uint64_t* scalars, const uint32_t* offsets, size_t m, uint64_t* out_xyz /* m*36 */);
/* The same call for bases the caller vouches to be elements of the prime-order subgroup G2 - public keys: a PublicKey of the reference is
 * one by construction (checked deserialisation crates/bls-crypto/src/bls/public.rs:123-149, secret keys, sums) - which is what
 * Batch::verify hands over (batch.rs:69).  Same result; the library may then split every scalar with the endomorphism psi (psi(P) = [x]P
 * on G2): an instance of n points with up to 253-bit scalars becomes one of up to 4 n points with 64-bit scalars (csrc/msm.h, k_gls_expand):
 * nd = 2 digits for a longest scalar of 65..126 bits, 3 up to 189, 4 beyond, wherever nd times the largest instance stays within 1024 points
 * (the window then follows the expanded size and there are (64 + c) / c windows); no split up to 64 bits or beyond that size.
 * For a base outside the subgroup the result is unspecified (use msm_batch_bls12_377_g2, which is VariableBaseMSM on any curve point). */
int msm_batch_bls12_377_g2_subgroup(const uint64_t* bases_xy, const uint8_t* inf, const uint64_t* scalars, const uint32_t* offsets, size_t m, uint64_t* out_xyz /* m*36 */);
int msm_batch_bw6_761_g1(const uint64_t* bases_xy, const uint8_t* inf, const uint64_t* scalars, const uint32_t* offsets, size_t m, uint64_t* out_xyz /* m*36 */);
int msm_batch_bw6_761_g2(const uint64_t* bases_xy, const uint8_t* inf, const uint64_t* scalars, const uint32_t* offsets, size_t m, uint64_t* out_xyz /* m*36 */);

/* ---- Batch::verify for m batches in one call, chained on the device (crates/bls-crypto/src/bls/batch.rs:44-84: per batch
 * P = sum_j e_j pk_j (G2 MSM), S = sum_j e_j sig_j (G1 MSM), accept iff e(S, -g2) * e(H(m), P) == 1; the FFI loops over batches
 * serially, crates/bls-snark-sys/src/signatures.rs:358).  Batch b owns keys / signatures / exponents [offsets[b], offsets[b+1])
 * (at most 1024 each); hash_xy[b] = H(m_b) affine; neg_g2_xy = the negated G2 generator, affine (the caller's constant; the
 * library restates no curve constant here).  Both batch MSMs run concurrently on two engines; their Jacobian results are
 * normalised ON the device straight into the pairing engine's input slots - nothing returns to the host but the m verdicts
 * out_ok[b] in {0, 1}.  *_inf: optional byte-per-point identity flags (NULL = none; a batch whose hash is flagged is checked without
 * that pair).  Exponents: canonical 4 x u64 (Batch::verify draws 128 + log2(n) random bits; the window count adapts
 * to the longest one present).  _dev: every pointer except offsets, neg_g2_xy and out_ok is a DEVICE pointer.
 * PRECONDITION: every public key pk_xy[i] is an element of the prime-order subgroup G2 and every signature an element of G1 - what the
 * reference's PublicKey / Signature values are by construction (checked deserialisation crates/bls-crypto/src/bls/public.rs:123-149,
 * signature.rs:31-57; secret keys; sums of such) and what Batch::verify therefore assumes.  The key sums use the endomorphism psi(P) = [x]P,
 * which holds on G2 only: for a key that is on the twist but outside G2 (e.g. decoded with decompress_bls12_377_g2(check_subgroup = 0))
 * the verdict is unspecified.  A caller holding unchecked points must run them through decompress_*(check_subgroup = 1) first - or use
 * msm_batch_bls12_377_g2 + msm_batch_bls12_377_g1 + pairing_product_is_one_batch_bls12_377, which are VariableBaseMSM on any curve point. */
int batch_verify_bls12_377(const uint64_t* pk_xy /* tot x 24 */, const uint8_t* pk_inf /* tot or NULL */, const uint64_t* sig_xy /* tot x 12 */,
                           const uint8_t* sig_inf /* tot or NULL */, const uint64_t* exponents /* tot x 4 */, const uint32_t* offsets /* m+1 */,
                           const uint64_t* hash_xy /* m x 12 */, const uint8_t* hash_inf /* m or NULL */, const uint64_t neg_g2_xy[24], size_t m,
                           uint8_t* out_ok /* m */);
int batch_verify_bls12_377_dev(const void* d_pk_xy, const void* d_pk_inf, const void* d_sig_xy, const void* d_sig_inf, const void* d_exponents,
                               const uint32_t* offsets, const void* d_hash_xy, const void* d_hash_inf, const uint64_t neg_g2_xy[24], size_t m,
                               uint8_t* out_ok /* m */);

/* The random exponents Seam A's batch_verify_strict draws for one call, as its device kernel produces them (tests / tooling): signer i
 * of the call (i < offsets[m]) gets the first (128 + ceil(log2 n_b) + 7) / 8 bytes - n_b the size of its batch, as
 * byte_count_from_target_batch_size, crates/bls-crypto/src/bls/batch.rs:23-28 - of block i of the ChaCha20 stream (RFC 7539 block
 * function, 64-bit block counter, zero nonce) under `key`, little-endian in 4 x u64.  out: offsets[m] x 4 u64, host.  batch.rs:51-58 draws
 * the same number of bytes per signer from rand::thread_rng(). */
int celo_amd_draw_batch_exponents(const uint32_t key[8], const uint32_t* offsets /* m+1 */, size_t m, uint64_t* out);

/* ---- pairing product check.  Replaces `Bls12_377::product_of_pairings(&pairs) == Fq12::one()` at
 *   crates/bls-crypto/src/bls/public.rs:102    (PublicKey::verify_sig: 2 pairs)
 *   crates/bls-crypto/src/bls/signature.rs:149 (Signature::batch_verify_hashes: n+1 pairs, one final exponentiation)
 * g1_xy: k affine G1 points (k*12 u64), g2_xy: k affine G2 points (k*24 u64), optional infinity byte arrays (a pair with
 * an infinite point contributes 1, as in ark-ec).  *is_one = 1 iff the product of the k pairings is the identity of GT.
 * The batch form checks m independent products in one launch: product p covers pairs [offsets[p], offsets[p+1]),
 * offsets has m+1 entries — the per-batch checks of Batch::verify (crates/bls-crypto/src/bls/batch.rs:83) for many
 * batches at once (crates/bls-snark-sys/src/signatures.rs:358 loops over them serially). */
int pairing_product_is_one_bls12_377(const uint64_t* g1_xy, const uint8_t* inf1, const uint64_t* g2_xy, const uint8_t* inf2, size_t k,
                                     int* is_one);
int pairing_product_is_one_batch_bls12_377(const uint64_t* g1_xy, const uint8_t* inf1, const uint64_t* g2_xy, const uint8_t* inf2,
                                           const uint32_t* offsets, size_t m, uint8_t* is_one);
/* Test/inspection hook: the GT value itself (72 u64 per product: the arkworks in-memory Fq12, Montgomery form);
 * miller_only != 0 skips the final exponentiation (product of Miller-loop values). */
int celo_amd_pairing_gt_bls12_377(const uint64_t* g1_xy, const uint8_t* inf1, const uint64_t* g2_xy, const uint8_t* inf2,
                                  const uint32_t* offsets, size_t m, int miller_only, uint64_t* gt72);
/* BW6-761: the pairing product check underneath ark_groth16::verify_proof (crates/epoch-snark/src/api/verifier.rs:35, reached
 * from the FFI `verify` at crates/bls-snark-sys/src/snark/mod.rs:23-45):
 *   e(A,B) * e(acc,-gamma) * e(C,-delta) == e(alpha,beta)   <=>   product over {(A,B),(acc,-gamma),(C,-delta),(-alpha,beta)} == 1.
 * g1_xy: k*24 u64, g2_xy: k*24 u64 (G2 coordinates are in Fq: M-type sextic twist). */
int pairing_product_is_one_bw6_761(const uint64_t* g1_xy, const uint8_t* inf1, const uint64_t* g2_xy, const uint8_t* inf2, size_t k,
                                   int* is_one);
/* The batch form, as for BLS12-377: m independent products in one call, product p over pairs [offsets[p], offsets[p+1]),
 * is_one[p] = 1 iff it is the identity (an empty product is) - what a verifier of many proofs calls (m products of four pairs). */
int pairing_product_is_one_batch_bw6_761(const uint64_t* g1_xy, const uint8_t* inf1, const uint64_t* g2_xy, const uint8_t* inf2,
                                         const uint32_t* offsets, size_t m, uint8_t* is_one);
int celo_amd_pairing_gt_bw6_761(const uint64_t* g1_xy, const uint8_t* inf1, const uint64_t* g2_xy, const uint8_t* inf2,
                                const uint32_t* offsets, size_t m, int miller_only, uint64_t* gt72);
/* ms[4] = {miller loops, GT products, final exponentiations, total} of the last pairing call (HIP events). */
int celo_amd_pairing_last_timings(float ms[4]);

/* ---- radix-2 NTT over Fr(BW6-761) (= Fq of BLS12-377, 377 bits), in place, natural order in and out: the witness-map
 * FFTs of the Groth16 prover.  Replaces ark-poly 0.1 Radix2EvaluationDomain::{fft, ifft,
 * coset_fft, coset_ifft}_in_place as called by ark_groth16::create_proof_no_zk (crates/epoch-snark/src/api/prover.rs:78,112).
 * data: n = 2^log_n elements, arkworks Montgomery limbs (6 u64 each).  omega: the domain's group_gen (its inverse for an
 * inverse transform).  coset: NULL, or a generator g: every x_i is multiplied by g^i BEFORE the transform (coset_after =
 * 0: coset_fft with g = the coset offset) or AFTER it (coset_after = 1: coset_ifft with g = offset^-1).  scale: NULL, or a
 * factor applied to every output (size_inv for the inverse transforms).  log_n <= 28: a larger log_n returns 2 before anything is
 * allocated or launched, here and in every entry below that takes a log_n (both fields, the witness maps included). */
int ntt_bw6_761_fr(uint64_t* data, unsigned log_n, const uint64_t omega[6], const uint64_t* coset, int coset_after, const uint64_t* scale);
int ntt_bw6_761_fr_dev(uint64_t* d_data, unsigned log_n, const uint64_t omega[6], const uint64_t* coset, int coset_after,
                       const uint64_t* scale, void* hip_stream);
/* ms[4] = {load/convert, butterfly passes, bit-reversal store, total}, passes = number of butterfly launches (last NTT call). */
int celo_amd_ntt_last_timings(float ms[4], int* passes);

/* ---- Groth16 prover over BW6-761 after R1CS synthesis: what ark_groth16::create_proof_no_zk does
 * with the constraint evaluations and the proving key, as called at crates/epoch-snark/src/api/prover.rs:78,112.
 *
 * groth16_witness_map_bw6_761: R1CStoQAP::witness_map (ark-groth16 0.1 r1cs_to_qap.rs) from the point where a, b, c hold the
 * evaluations of the QAP polynomials over the domain (n = 2^log_n elements each, arkworks Montgomery limbs, the input-consistency
 * rows included: groth16_r1cs_rows below makes them from the constraint matrices and the assignment, and
 * groth16_prove_r1cs_with_key starts from there; a caller that has a, b, c starts here): ifft(a, b, c); coset_fft(a, b, c);
 * ab = (a o b - c) * vanishing_inv; coset_ifft(ab).  On return a holds h (n coefficients; b and c are scratch) - as field
 * elements, or with out_canonical != 0 as canonical integers (Fr::into_repr(), what the h MSM takes).  Domain constants from the
 * caller (nothing of ark-poly is restated): omega = group_gen, omega_inv, coset = the coset offset (F::multiplicative_generator()),
 * coset_inv, size_inv = n^-1, vanishing_inv = (coset^n - 1)^-1 - all arkworks Montgomery limbs.
 *
 * groth16_prove_bw6_761: the proof with r = s = 0 (create_proof_no_zk):
 *   A = a_query[0] + MSM(a_query[1..], assignment) + alpha_g1          B = b_g2_query[0] + MSM(b_g2_query[1..], assignment) + beta_g2
 *   C = MSM(l_query, aux) + MSM(h_query, h)
 * queries: affine points (24 u64 each); assignment: n_assignment canonical scalars (public inputs without the leading 1, then the
 * witness), aux = its last n_aux entries; h: n_h canonical scalars.  As in VariableBaseMSM::multi_scalar_mul the shorter of bases
 * and scalars decides each MSM's length.  The four MSMs run concurrently on four engines.  Results: Jacobian, arkworks layout.
 * The point at infinity: a proving key holds it for every variable absent from A, B or the auxiliary part (ark-groth16 generator.rs), as
 * GroupAffine::zero() = (x, y, infinity) = (0, 1, true).  These entry points take coordinates only, so a query row - or query[0], alpha, beta
 * - with x = 0 and y = 1 IS the identity here (it contributes nothing whatever its scalar); on none of the groups involved is (0, 1) an
 * element of the prime-order group, so no key element is shadowed (csrc/msm.h k_flag_ark_zero).  The plain msm_* entry points do NOT
 * apply this rule: they take the identity through their `inf` byte arrays. */
int groth16_witness_map_bw6_761(uint64_t* a, uint64_t* b, uint64_t* c, unsigned log_n, const uint64_t omega[6], const uint64_t omega_inv[6], const uint64_t coset[6],
                                const uint64_t coset_inv[6], const uint64_t size_inv[6], const uint64_t vanishing_inv[6], int out_canonical);
int groth16_witness_map_bw6_761_dev(uint64_t* d_a, uint64_t* d_b, uint64_t* d_c, unsigned log_n, const uint64_t omega[6], const uint64_t omega_inv[6],
                                    const uint64_t coset[6], const uint64_t coset_inv[6], const uint64_t size_inv[6], const uint64_t vanishing_inv[6],
                                    int out_canonical, void* hip_stream);
int groth16_prove_bw6_761(const uint64_t* a_query, size_t na, const uint64_t* b_g2_query, size_t nb, const uint64_t* h_query, size_t nh, const uint64_t* l_query,
                          size_t nl, const uint64_t alpha_g1[24], const uint64_t beta_g2[24], const uint64_t* assignment, size_t n_assignment, size_t n_aux,
                          const uint64_t* h, size_t n_h, uint64_t out_a[36], uint64_t out_b[36], uint64_t out_c[36]);

/* ---- the proof against a LOADED key: groth16_load_key_* builds the fixed-base tables of the four queries once (msm_*_precompute above; the
 * reference creates its Parameters once, crates/epoch-snark/src/api/setup.rs:63-105, and hands the same ones to every
 * create_proof_no_zk, prover.rs:78,112); groth16_prove_with_key then computes A, B, C of groth16_prove_bw6_761 / _bls12_377 with four
 * msm_*_fixed calls (concurrent, one engine each) and no query crossing PCIe again.  Same arguments, identity-row rule, results and
 * error behaviour as the entry points above; a_query[0] / b_g2_query[0] / alpha / beta are kept with the key.  window_bits: the tables'
 * window size (0 = automatic).  A key is bound to the device it was loaded on (101 from another) and may prove from several threads. */
int groth16_load_key_bw6_761(const uint64_t* a_query, size_t na, const uint64_t* b_g2_query, size_t nb, const uint64_t* h_query, size_t nh, const uint64_t* l_query, size_t nl,
                             const uint64_t alpha_g1[24], const uint64_t beta_g2[24], int window_bits, void** out_key);
int groth16_load_key_bls12_377(const uint64_t* a_query, size_t na, const uint64_t* b_g2_query, size_t nb, const uint64_t* h_query, size_t nh, const uint64_t* l_query, size_t nl,
                               const uint64_t alpha_g1[12], const uint64_t beta_g2[24], int window_bits, void** out_key);
int groth16_prove_with_key(const void* key, const uint64_t* assignment, size_t n_assignment, size_t n_aux, const uint64_t* h, size_t n_h, uint64_t* out_a, uint64_t* out_b,
                           uint64_t* out_c);
int groth16_free_key(void* key);

/* ---- the same three steps over BLS12-377: the hash-helper proof of an epoch (crates/epoch-snark/src/api/prover.rs:83-118,
 * create_proof_no_zk::<BLSCurve, _> at :112), whose witness map runs over Fr(BLS12-377) (253 bits, 2-adicity 47; elements are 4 u64 in
 * arkworks Montgomery form, R = 2^256) and whose queries are BLS12-377 points: a_query / h_query / l_query / alpha_g1 in G1 (affine
 * 12 u64), b_g2_query / beta_g2 in G2 (24 u64); assignment and h are canonical 4-u64 scalars; A and C come back as G1 Jacobian
 * (18 u64), B as G2 Jacobian (36 u64).  Same argument meaning, transforms and error behaviour as the BW6-761 entry points above. */
int ntt_bls12_377_fr(uint64_t* data, unsigned log_n, const uint64_t omega[4], const uint64_t* coset, int coset_after, const uint64_t* scale);
int ntt_bls12_377_fr_dev(uint64_t* d_data, unsigned log_n, const uint64_t omega[4], const uint64_t* coset, int coset_after,
                         const uint64_t* scale, void* hip_stream);
int groth16_witness_map_bls12_377(uint64_t* a, uint64_t* b, uint64_t* c, unsigned log_n, const uint64_t omega[4], const uint64_t omega_inv[4], const uint64_t coset[4],
                                  const uint64_t coset_inv[4], const uint64_t size_inv[4], const uint64_t vanishing_inv[4], int out_canonical);
int groth16_witness_map_bls12_377_dev(uint64_t* d_a, uint64_t* d_b, uint64_t* d_c, unsigned log_n, const uint64_t omega[4], const uint64_t omega_inv[4],
                                      const uint64_t coset[4], const uint64_t coset_inv[4], const uint64_t size_inv[4], const uint64_t vanishing_inv[4],
                                      int out_canonical, void* hip_stream);
int groth16_prove_bls12_377(const uint64_t* a_query, size_t na, const uint64_t* b_g2_query, size_t nb, const uint64_t* h_query, size_t nh, const uint64_t* l_query,
                            size_t nl, const uint64_t alpha_g1[12], const uint64_t beta_g2[24], const uint64_t* assignment, size_t n_assignment, size_t n_aux,
                            const uint64_t* h, size_t n_h, uint64_t out_a[18], uint64_t out_b[36], uint64_t out_c[18]);

/* ---- bulk decoding of compressed points: n keys or signatures in arkworks 0.1 wire form
 * (G1: 48 B, G2: 96 B; x little-endian, flag bits 0x80 = "y is the larger root", 0x40 = infinity in the last byte) to
 * affine (x, y) in arkworks Montgomery limbs - the layout the MSM and pairing entry points take.  One point per GPU lane:
 * the square root (table-driven in Fq, the norm method in Fq2), the sign choice and, with check_subgroup != 0, r*P == O.
 * Replaces the per-key work of PublicKey::deserialize / Signature::deserialize (crates/bls-crypto/src/bls/public.rs:123-149,
 * signature.rs:31-57: GroupAffine::deserialize = get_point_from_x + is_in_correct_subgroup_assuming_on_curve) and of the
 * per-validator loop of the epoch FFI (crates/bls-snark-sys/src/snark/epoch_block.rs:187-196).
 * status[i]: 0 = decoded, 1 = the encoding of the point at infinity, 2 = not a valid encoding (x >= q or no y exists),
 * 3 = on the curve but outside the prime-order subgroup; out_xy[i] is all zero unless status[i] == 0. */
int decompress_bls12_377_g1(const uint8_t* in /* n x 48 */, size_t n, int check_subgroup, uint64_t* out_xy /* n x 12 */, uint8_t* status /* n */);
int decompress_bls12_377_g2(const uint8_t* in /* n x 96 */, size_t n, int check_subgroup, uint64_t* out_xy /* n x 24 */, uint8_t* status /* n */);
int decompress_bls12_377_g1_dev(const uint8_t* d_in, size_t n, int check_subgroup, uint64_t* d_out_xy, uint8_t* d_status, void* hip_stream);
int decompress_bls12_377_g2_dev(const uint8_t* d_in, size_t n, int check_subgroup, uint64_t* d_out_xy, uint8_t* d_status, void* hip_stream);
/* ---- the same decoding with each distinct byte string decoded once (csrc/dedup.h, csrc/unit_dedup.hip): a validator set changes by a
 * handful of keys per epoch, so the keys of many blocks are almost all repeats - what PublicKeyCache::deserialize
 * (crates/bls-crypto/src/bls/cache.rs, "the aggregated public key changes slowly") is on the host.  A device hash table over the raw bytes
 * finds, for every key, a representative with identical bytes; only the representatives go through the decoder above; every key then
 * receives its representative's row and status.  out_xy and status are exactly those of decompress_bls12_377_g1 / _g2.
 *   out_rep (n, or NULL): rep[i] <= i, key rep[i] has the bytes of key i, rep[rep[i]] == rep[i]; unless a probe sequence of the table
 *                         reached its cap (below), rep[i] is the smallest j whose key equals key i
 *   out_decoded (or NULL): the number of keys that went through the decoder: the number of distinct keys, plus the keys that hit the cap
 * Refusals, the n = 0 answer (0; *out_decoded = 0) and the return codes are those of the plain entries; the refusals need no device.  The
 * _dev forms take device pointers for in (any byte alignment), out_xy, status and out_rep, a host pointer for out_decoded, run on
 * hip_stream and return after the work has drained (one 8-byte read of the number of representatives sizes the decoder's launch).
 * Memory beside the outputs: 8 S + 16 n bytes with S = next_pow2(n) << slack_log table slots, and the decoded representatives. */
int decompress_bls12_377_g1_dedup(const uint8_t* in /* n x 48 */, size_t n, int check_subgroup, uint64_t* out_xy /* n x 12 */, uint8_t* status /* n */,
                                  uint32_t* out_rep /* n, or NULL */, uint64_t* out_decoded /* or NULL */);
int decompress_bls12_377_g2_dedup(const uint8_t* in /* n x 96 */, size_t n, int check_subgroup, uint64_t* out_xy /* n x 24 */, uint8_t* status /* n */,
                                  uint32_t* out_rep /* n, or NULL */, uint64_t* out_decoded /* or NULL */);
int decompress_bls12_377_g1_dedup_dev(const uint8_t* d_in, size_t n, int check_subgroup, uint64_t* d_out_xy, uint8_t* d_status, uint32_t* d_out_rep, uint64_t* out_decoded,
                                      void* hip_stream);
int decompress_bls12_377_g2_dedup_dev(const uint8_t* d_in, size_t n, int check_subgroup, uint64_t* d_out_xy, uint8_t* d_status, uint32_t* d_out_rep, uint64_t* out_decoded,
                                      void* hip_stream);
/* The switch.  on: whether the composed entry points that decode compressed validator keys (epoch_encode_blocks_bls12_377,
 * epoch_public_inputs_bw6_761, verify_epoch_proofs_bw6_761, verify_epoch_transitions_bls12_377) de-duplicate them: -1 the rule
 * (csrc/dedup.h key_dedup_pick), 0 never, 1 always; their outputs are the same either way.  The four _dedup entries above always
 * de-duplicate.  slack_log 0 .. 2 (-1: the default, 1): the table has next_pow2(n) << slack_log slots.  max_probes 1 .. 1024 (0: the
 * default, 64): a key that has probed so many slots without finding its bytes or a free slot is decoded on its own - the bound on the
 * work for crafted keys that share one slot.  Process-wide; 2 for any other value, and nothing changes.  _get: on, slack_log, max_probes
 * as they stand. */
int celo_amd_key_dedup_set(int on, int slack_log, int max_probes);
int celo_amd_key_dedup_get(int out[3]);
/* The last de-duplicating call that succeeded (a _dedup entry, or the key decoding of a composed call): counts = keys, keys decoded;
 * ms (HIP events) = table + representatives + compaction, gather, decode, scatter. */
int celo_amd_key_dedup_last(uint64_t counts[2], float ms[4]);
/* Jacobian -> affine for n points in one launch (Montgomery's trick inside each lane): replaces
 * ProjectiveCurve::batch_normalization_into_affine as called before every MSM (crates/bls-crypto/src/bls/signature.rs:82,
 * public.rs:58).  jac: n x (X, Y, Z) arkworks Montgomery limbs (G1: 18 u64, G2: 36 u64 per point; identity = Z == 0);
 * out_xy: n x (x, y) in the layout the MSM / pairing entry points take, a zero row and inf[i] = 1 for the identity. */
int normalize_bls12_377_g1(const uint64_t* jac /* n x 18 */, size_t n, uint64_t* out_xy /* n x 12 */, uint8_t* inf /* n */);
int normalize_bls12_377_g2(const uint64_t* jac /* n x 36 */, size_t n, uint64_t* out_xy /* n x 24 */, uint8_t* inf /* n */);
/* kernel time (HIP events) of the last decompress / normalize call */
int celo_amd_decompress_last_ms(float* ms);

/* ---- bulk decoding of serialized BW6-761 points (the curve of every prover MSM): arkworks 0.1
 * CanonicalDeserialize of G1 (y^2 = x^3 - 1) and G2 (the M-twist y^2 = x^3 + 4, coordinates in Fq) points, 96 B per coordinate,
 * little-endian, flags in the two top bits of the last byte (0x40 infinity, 0x80 "y is the larger root").  One point per GPU lane
 * (csrc/wire761.h, csrc/unit_wire761.hip): the square root rhs^((q+1)/4), the sign choice and, when checked, r*P == O with
 * r = r_BW6 = q_BLS12-377 - the predicate of ark-ec 0.1 is_in_correct_subgroup_assuming_on_curve, evaluated as [a]P + [b]phi(P) == O for the
 * endomorphism a + b phi of degree exactly r (two 189-bit scalars in one ladder; the argument is at check_points_* below and in
 * csrc/wire761.h), with the 377-bit ladder kept as its twin (celo_amd_wire761_set_subgroup_test).
 *   decompress_bw6_761_*:          96 B points; check_subgroup != 0 is GroupAffine::deserialize (what ark-groth16 runs per point of a
 *                                  ProvingKey / VerifyingKey / Proof: crates/epoch-snark/src/api/setup.rs:12,17-20, the "serialized byte
 *                                  arrays of compressed elements" of crates/bls-snark-sys/src/snark/mod.rs:13-17), 0 skips the subgroup test.
 *   decode_uncompressed_bw6_761_*: 192 B points (x, then y with the flags on y's last byte); check != 0: on the curve and in the subgroup
 *                                  (deserialize_uncompressed - stricter than ark 0.1, which may skip the curve equation: an off-curve point
 *                                  is status 2 here), check == 0: the canonical range only (deserialize_unchecked).
 * out_xy: n x 24 u64, affine (x, y) in arkworks Montgomery limbs - the layout msm_bw6_761_* take - all zero unless status[i] == 0.
 * status[i], checks in this order: flags 0xC0 -> 2; infinity flag -> 1 (before any range check); a coordinate >= q -> 2; no square root
 * (compressed) or off the curve (uncompressed, checked) -> 2; checked and r*P != O -> 3; else 0.  The _dev forms take device pointers
 * and run on hip_stream (0: the null stream); calls are serialised per process. */
int decompress_bw6_761_g1(const uint8_t* in /* n x 96 */, size_t n, int check_subgroup, uint64_t* out_xy /* n x 24 */, uint8_t* status /* n */);
int decompress_bw6_761_g2(const uint8_t* in /* n x 96 */, size_t n, int check_subgroup, uint64_t* out_xy /* n x 24 */, uint8_t* status /* n */);
int decompress_bw6_761_g1_dev(const uint8_t* d_in, size_t n, int check_subgroup, uint64_t* d_out_xy, uint8_t* d_status, void* hip_stream);
int decompress_bw6_761_g2_dev(const uint8_t* d_in, size_t n, int check_subgroup, uint64_t* d_out_xy, uint8_t* d_status, void* hip_stream);
int decode_uncompressed_bw6_761_g1(const uint8_t* in /* n x 192 */, size_t n, int check, uint64_t* out_xy /* n x 24 */, uint8_t* status /* n */);
int decode_uncompressed_bw6_761_g2(const uint8_t* in /* n x 192 */, size_t n, int check, uint64_t* out_xy /* n x 24 */, uint8_t* status /* n */);
/* Which subgroup test the BW6-761 decoders above run - and with them groth16_load_key_bw6_761_serialized, the serialized BW6-761 verifiers
 * and check_points_bw6_761_*: 0 = the endomorphism form (the default), 1 = the r*P ladder, its definition.  Verdicts and rows are identical;
 * the switch exists for the same-run comparison (tools/bench_subgroup.py) and the tests.  Process-wide; 2 for any other value. */
int celo_amd_wire761_set_subgroup_test(int form);
/* ---- validation of points held as affine rows: is_on_curve / is_in_correct_subgroup for all four groups, in bulk (csrc/check.h,
 * csrc/unit_check.hip; one row per GPU lane).  Every other group entry point of this header trusts its rows ("points off the curve are not
 * validated"; the _subgroup entries, batch_verify_bls12_377 and verify_aggregated_seals_bls12_377 rest on "the caller vouches"): a caller that
 * holds limb rows rather than wire bytes validates them here first.
 *   xy:    n rows of affine (x, y) in arkworks Montgomery limbs - BLS12-377 G1 12 u64; BLS12-377 G2 24 u64 (x.c0, x.c1, y.c0, y.c1); BW6-761
 *          G1 and G2 24 u64 - the layout the MSM, pairing and key entry points take.  Only read.
 *   inf:   n identity flags, or NULL for none.
 *   level: 1 = the curve equation only; 2 = the curve and the prime-order subgroup.
 *   out_status[i], the first that applies (the decoders' codes): 1 the flag is set - the coordinates are not looked at; 2 a coordinate (an Fq2
 *          component) is not below q as the limbs stand, or (x, y) is not on the curve; 3 (level 2) on the curve but r*P != O; 0 good.
 *   out_first_bad: may be NULL; the smallest i with status 2 or 3, n if there is none.  A host pointer in the _dev forms as well.
 * Returns 0 whatever the statuses are, and for n = 0; 2 with nothing written and before any device use for xy or out_status NULL (n > 0), a
 * level outside {1, 2} or n > 2^31 - 1.  The _dev forms take device pointers for xy, inf and out_status, run on hip_stream (0: the null
 * stream) and return after the work has drained; calls are serialised per process.
 * The subgroup tests are the decoders': for BLS12-377 the endomorphism tests of decompress_bls12_377_* (phi(P) == -[x^2]P on G1, psi(P) == [x]P
 * on G2), for BW6-761 the following.  phi(x, y) = (beta x, y) with beta a primitive cube root of unity in Fq satisfies phi^2 + phi + 1 = 0 on
 * both curves.  With x = 0x8508c00000000001, a = (2x^3 - 2x^2 - x + 1)/3 and b = (x^3 - x^2 - 2x - 1)/3 have a^2 - ab + b^2 = r exactly, so
 * a + b phi is an endomorphism of degree r whose kernel has r points; beta is chosen (one root for G1, the other for G2) so that phi acts on
 * the order-r subgroup as the lambda with a + b lambda = 0 (mod r), hence the kernel IS the subgroup: [a]P + [b]phi(P) == O exactly when
 * r*P == O, for every curve point, with no cofactor condition.  (The better-known vector (x + 1, x^3 - x^2 + 1) has norm 3r and is wrong on
 * G2, whose cofactor is divisible by 3: (0, 2) passes it.)  About 2 430 field products per point where the ladder takes 4 720. */
int check_points_bls12_377_g1(const uint64_t* xy /* n x 12 */, const uint8_t* inf /* n or NULL */, size_t n, int level, uint8_t* out_status /* n */, uint64_t* out_first_bad);
int check_points_bls12_377_g2(const uint64_t* xy /* n x 24 */, const uint8_t* inf /* n or NULL */, size_t n, int level, uint8_t* out_status /* n */, uint64_t* out_first_bad);
int check_points_bw6_761_g1(const uint64_t* xy /* n x 24 */, const uint8_t* inf /* n or NULL */, size_t n, int level, uint8_t* out_status /* n */, uint64_t* out_first_bad);
int check_points_bw6_761_g2(const uint64_t* xy /* n x 24 */, const uint8_t* inf /* n or NULL */, size_t n, int level, uint8_t* out_status /* n */, uint64_t* out_first_bad);
int check_points_bls12_377_g1_dev(const uint64_t* d_xy, const uint8_t* d_inf, size_t n, int level, uint8_t* d_out_status, uint64_t* out_first_bad, void* hip_stream);
int check_points_bls12_377_g2_dev(const uint64_t* d_xy, const uint8_t* d_inf, size_t n, int level, uint8_t* d_out_status, uint64_t* out_first_bad, void* hip_stream);
int check_points_bw6_761_g1_dev(const uint64_t* d_xy, const uint8_t* d_inf, size_t n, int level, uint8_t* d_out_status, uint64_t* out_first_bad, void* hip_stream);
int check_points_bw6_761_g2_dev(const uint64_t* d_xy, const uint8_t* d_inf, size_t n, int level, uint8_t* d_out_status, uint64_t* out_first_bad, void* hip_stream);
/* kernel time (HIP events) of the last check_points_* call */
int celo_amd_check_points_last_ms(float* ms);
/* ---- the same uncompressed forms for BLS12-377 (csrc/wire.h wire_decode_row_*, csrc/unit_wire.hip k_decode377u): what
 * GroupAffine::deserialize_uncompressed / deserialize_unchecked run per point of a large ProvingKey<Bls12_377> - no square root per point.
 * in: n x 96 B (G1: x, then y) / n x 192 B (G2: x.c0, x.c1, y.c0, y.c1); the flags sit on the last byte of y (G2: of y.c1).  out_xy and
 * status as decompress_bls12_377_* write them.  check != 0: the canonical range, the curve equation (y^2 = x^3 + 1; y^2 = x^3 + B' over Fq2,
 * the twist constant of decompress_bls12_377_g2) and the subgroup tests of decompress_bls12_377_*; check == 0: the canonical range only.
 * status[i], meaning and order as for decode_uncompressed_bw6_761_*: flags 0xC0 -> 2; infinity flag -> 1 (before any range check); a
 * component >= q -> 2; off the curve (checked) -> 2; outside the subgroup (checked) -> 3; else 0.  A set 0x80 bit alone is ignored (the
 * y that is written is the y that is read); a high bit on any other component makes it >= q.  Rows are all zero unless status[i] == 0.
 * Returns 0; 2: n > 2^31 - 1, a NULL pointer, or a _dev out_xy that is not 8-byte aligned (the rows are stored as 64-bit words); 10;
 * 100.  n == 0 returns 0.  The _dev forms take device pointers and run on hip_stream (0: the null stream); calls are serialised per
 * process with decompress_bls12_377_*. */
int decode_uncompressed_bls12_377_g1(const uint8_t* in /* n x 96 */, size_t n, int check, uint64_t* out_xy /* n x 12 */, uint8_t* status /* n */);
int decode_uncompressed_bls12_377_g2(const uint8_t* in /* n x 192 */, size_t n, int check, uint64_t* out_xy /* n x 24 */, uint8_t* status /* n */);
int decode_uncompressed_bls12_377_g1_dev(const uint8_t* d_in, size_t n, int check, uint64_t* d_out_xy, uint8_t* d_status, void* hip_stream);
int decode_uncompressed_bls12_377_g2_dev(const uint8_t* d_in, size_t n, int check, uint64_t* d_out_xy, uint8_t* d_status, void* hip_stream);
/* ---- a serialized ark-groth16 0.1 ProvingKey<BW6_761> (the reference's Groth16Parameters, crates/epoch-snark/src/api/setup.rs:12,17-20),
 * in the derive order of the struct; a Vec is a u64 little-endian length followed by its elements:
 *   vk { alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1: Vec<G1> }, beta_g1, delta_g1,
 *   a_query: Vec<G1>, b_g1_query: Vec<G1>, b_g2_query: Vec<G2>, h_query: Vec<G1>, l_query: Vec<G1>
 * (the VK prefix is the one csrc/seam_epoch.hip verify parses).  form: 0 = compressed, checked (ProvingKey::deserialize); 1 = uncompressed,
 * checked (deserialize_uncompressed); 2 = uncompressed, unchecked (deserialize_unchecked).  Points are 96 B (form 0) or 192 B.
 *
 * groth16_key_layout_bw6_761: a host walk of that structure (no device call).  out[16]:
 *   [0] bytes per point        [1] len                      [2] / [3]   gamma_abc_g1: count / byte offset of its first point
 *   [4] / [5]   a_query        [6] / [7]   b_g1_query       [8] / [9]   b_g2_query      [10] / [11] h_query      [12] / [13] l_query
 *   [14] byte offset of beta_g1 (delta_g1 follows)          [15] the number of points in the key
 * (alpha_g1, beta_g2, gamma_g2, delta_g2 are the points at offsets 0, 1, 2, 3 x [0].)  Points are indexed in serialization order:
 * 0 alpha_g1, 1-3 beta/gamma/delta_g2, then gamma_abc_g1, beta_g1, delta_g1, a_query, b_g1_query, b_g2_query, h_query, l_query.
 * Returns 0, 2 (bad arguments), 30 (truncated: the input ends inside a length field or a section), 31 (bytes left over after l_query)
 * or 32 (a length field whose byte size does not fit 64 bits).  Lengths are checked against what is left before any product is formed.
 *
 * groth16_load_key_bw6_761_serialized: the layout walk, one copy of the bytes to the device, every point of every section decoded and checked
 * there (those create_proof_no_zk never reads included: gamma_*, delta_*, beta_g1, b_g1_query - a corrupt one fails the load as ark's
 * deserialize would), the four queries decoded straight into the buffers their fixed-base tables are built from (no decoded limbs return to
 * the host), then the key groth16_load_key_bw6_761 would build with alpha_g1 = vk.alpha_g1 and beta_g2 = vk.beta_g2; a point at infinity in
 * a query is that row's identity.  It proves with groth16_prove_with_key and is released with groth16_free_key.  Returns the layout codes
 * above, 2 (bad arguments, or an empty a_query / b_g2_query: the proof needs their first rows), 33 (a point was rejected: status 2 or 3
 * above; *first_bad_point = its index in serialization order), or the codes of groth16_load_key_bw6_761.  On any failure everything is
 * freed and *out_key stays NULL; first_bad_point (may be NULL) is written only with 33. */
int groth16_key_layout_bw6_761(const uint8_t* bytes, size_t len, int form, uint64_t out[16]);
int groth16_load_key_bw6_761_serialized(const uint8_t* bytes, size_t len, int form, int window_bits, void** out_key, uint64_t* first_bad_point);
/* ---- the same for a serialized ProvingKey<Bls12_377> - the reference's hash-helper parameters (Parameters.hash_to_bits,
 * crates/epoch-snark/src/api/setup.rs:17-20, consumed at prover.rs:112).  One walk and one loader with the BW6-761 entries above: the struct
 * order, the forms, the return codes, the index space of first_bad_point and the cleanup are theirs word for word.  What differs is that
 * points have two sizes: a G1 point is P bytes (48 compressed, 96 uncompressed) and a G2 point 2 P.  out[0] = P; alpha_g1, beta_g2, gamma_g2
 * and delta_g2 sit at offsets 0, P, 3 P, 5 P and the length field of gamma_abc_g1 at 7 P; among the vectors only b_g2_query has the double
 * stride.  A compressed VerifyingKey with k gamma_abc_g1 entries is 7 x 48 + 8 + 48 k bytes: what groth16_vk_load_bls12_377_serialized reads.
 * The loader decodes form 0 with the kernels of decompress_bls12_377_* and forms 1 / 2 with those of decode_uncompressed_bls12_377_*, one
 * launch per section, G1 rows of 12 u64 and G2 rows of 24; the handle is the one groth16_load_key_bls12_377 would build, proves with
 * groth16_prove_with_key / groth16_prove_r1cs_with_key and is released with groth16_free_key. */
int groth16_key_layout_bls12_377(const uint8_t* bytes, size_t len, int form, uint64_t out[16]);
int groth16_load_key_bls12_377_serialized(const uint8_t* bytes, size_t len, int form, int window_bits, void** out_key, uint64_t* first_bad_point);
/* ms[0]: kernel time of the last decompress_bw6_761_* / decode_uncompressed_bw6_761_* call; ms[1..3]: the last serialized key load's (either
 * curve) transfer of the bytes, decoding (all sections and the rejection scan) and fixed-base table build */
int celo_amd_wire761_last_timings(float ms[4]);

/* ---- Groth16 verification over BW6-761 for m proofs under ONE verifying key (BLS12-377: the next block): ark_groth16::prepare_verifying_key + verify_proof
 * (crates/epoch-snark/src/api/verifier.rs:35, what the FFI `verify` runs per proof) from the inputs to the verdict bytes on the device -
 * what a light client checking many epoch proofs, or a service checking proofs of many provers, calls instead of one msm_bw6_761_g1 and one
 * pairing_product_is_one_bw6_761 per proof.  The Groth16 counterpart of batch_verify_bls12_377.
 *
 * groth16_vk_load_bw6_761: the key from affine arkworks limbs (24 u64 per point; gamma_abc_g1: n_abc rows, n_abc - 1 public inputs).  Kept on
 * the device: -alpha, beta, -gamma, -delta and, per input base gamma_abc[j], j >= 1, one signed-digit window table (csrc/fixed_base.h,
 * generalised from one generator to n_abc - 1 bases) - an input's multiple is then one mixed addition per window and no doubling.  The window
 * width c is the widest of 10 .. 4 bits whose tables fit 64 MiB (10 bits up to 15 inputs, 7 bits at 64); celo_amd_groth16_verify_last
 * reports it.  A row that is all zero, or arkworks' (0, 1), is the point at infinity.
 * groth16_vk_load_bw6_761_serialized: the same from VerifyingKey::serialize bytes (alpha_g1 | beta_g2 | gamma_g2 | delta_g2 | u64 n_abc |
 * gamma_abc_g1, compressed), decoded and CHECKED as VerifyingKey::deserialize does (curve, prime-order subgroup).
 * Returns 0; 2: a NULL pointer or n_abc == 0; 36: n_abc - 1 > 64 public inputs (out of scope); 30 / 31: the serialized key ends early /
 * has bytes left over; 33: a point of it does not decode or is outside the subgroup; 10: allocation failure; 100: no device.  The argument
 * and length checks come first and need no device.  The handle is bound to the device it was loaded on (101 from a thread bound to another),
 * is read-only after the load and may be used from several host threads at once; groth16_vk_free releases it (2: not a live handle).
 *
 * groth16_verify_batch_bw6_761: out_ok[i] = 1 iff verify_proof(pvk, (A_i, B_i, C_i), inputs_i) would return true:
 *   e(A_i, B_i) e(acc_i, -gamma) e(C_i, -delta) e(-alpha, beta) == 1,   acc_i = gamma_abc[0] + sum_j inputs_i[j] gamma_abc[j + 1].
 * a_xy / b_xy / c_xy: m rows of 24 u64 (affine arkworks limbs); *_inf: optional identity bytes (NULL = none) - a pair with a point at
 * infinity contributes 1, as in ark-ec; inputs: m x (n_abc - 1) x 6 u64, CANONICAL integers (may be NULL when n_abc == 1).  An input that
 * is not below r makes that proof's verdict 0: ark cannot represent such a value, and treating x and x + r alike would let one statement
 * be presented under two encodings.
 * groth16_verify_batch_bw6_761_serialized: proofs = m x 288 B, Proof::serialize (A | B | C compressed).  The bytes cross once; every point
 * is decoded and checked on the device (decompress_bw6_761_*_dev, check_subgroup = 1) into the rows the verifier reads; a proof with a point
 * that does not decode or is outside the prime-order subgroup gets verdict 0 - that proof alone.
 * mode 0 ("each"): m independent products of four pairs in one batched pairing call.  No precondition.
 * mode 1 ("combined"): the random linear combination
 *   prod_i e(r_i A_i, B_i) * e(sum r_i acc_i, -gamma) * e(sum r_i C_i, -delta) * e(-(sum r_i) alpha, beta) == 1
 * - m + 3 Miller loops and ONE final exponentiation instead of 4 m and m, paid for with m 128-bit ladders and two m-term MSMs.  If it holds,
 * every proof whose status is clean gets 1; if not, the call runs mode 0 and returns its verdicts: out_ok means the same in both modes
 * (up to the soundness error 2^-127 of the combination).  PRECONDITION of mode 1, as for batch_verify_bls12_377: every A_i, C_i is an element
 * of G1 and every B_i of G2 (the prime-order subgroups) - the combination argument holds in a group of prime order only.  The serialized
 * entry always guarantees it; a caller of the limb entry holding unchecked points uses mode 0 or decodes them with check_subgroup = 1.
 * Exponents: r_i = 2^127 | (the low 127 bits of the first 16 bytes, little-endian, of block i of the ChaCha20 stream under `key`) - the
 * block function of celo_amd_draw_batch_exponents.  The top bit is fixed: every ladder has the same length.  key: 8 x u32, or NULL for
 * 32 bytes from the operating system per call (getrandom, as batch_verify_strict seeds its stream) - what a verifier uses; a fixed key
 * is for tests.  celo_amd_groth16_draw_exponents returns them (m x 2 u64, host).
 * Choosing a mode (one MI355X, two inputs, profiles/bench_groth16_verify.json): a call has a floor of 65-90 ms in either
 * mode.  Mode 0 takes 79 / 67 / 146 ms for 64 / 1 024 / 16 421 proofs, mode 1 92 / 87 / 92 ms: combined / each = 1.16, 1.30, 0.63.  Use mode 0
 * up to a few thousand proofs and mode 1 above (the crossover lies between 1 024 and 16 421 proofs and was not bracketed further).
 * Returns 0; 2: a NULL pointer, mode not 0 / 1, m > 2^24, a handle that is not live; 101; 10; 100.  m == 0 returns 0 and touches nothing.
 * Limits: at most 64 public inputs, m <= 2^24 proofs per call; products are laid out at offsets 0, 4, 8, ... (each) or as one product of
 * m + 3 pairs (combined) in the pairing engine's own input slots.
 *
 * celo_amd_groth16_verify_last: of the last successful verify call of the process - *path: 0 each, 1 combined accepted, 2 combined rejected
 * then each; *window_bits: c of its key; ms[8]: [0] decoding, [1] input sums, [2] exponents and ladders, [4] pairing products, [6] transfers
 * to the device (HIP events), [3] the two MSMs and (sum r) alpha, [5] the whole call (wall).  Any pointer may be NULL. */
int groth16_vk_load_bw6_761(const uint64_t alpha_g1[24], const uint64_t beta_g2[24], const uint64_t gamma_g2[24], const uint64_t delta_g2[24],
                            const uint64_t* gamma_abc_g1 /* n_abc x 24 */, size_t n_abc, void** out_vk);
int groth16_vk_load_bw6_761_serialized(const uint8_t* bytes, size_t len, void** out_vk);
int groth16_vk_free(void* vk);
int groth16_verify_batch_bw6_761(const void* vk, const uint64_t* a_xy /* m x 24 */, const uint8_t* a_inf, const uint64_t* b_xy /* m x 24 */, const uint8_t* b_inf,
                                 const uint64_t* c_xy /* m x 24 */, const uint8_t* c_inf, const uint64_t* inputs /* m x (n_abc - 1) x 6 */, size_t m, int mode,
                                 const uint32_t* key /* 8, or NULL */, uint8_t* out_ok /* m */);
int groth16_verify_batch_bw6_761_serialized(const void* vk, const uint8_t* proofs /* m x 288 */, const uint64_t* inputs, size_t m, int mode,
                                            const uint32_t* key /* 8, or NULL */, uint8_t* out_ok /* m */);
int celo_amd_groth16_draw_exponents(const uint32_t key[8], size_t m, uint64_t* out /* m x 2 */);
int celo_amd_groth16_verify_last(int* path, int* window_bits, float ms[8]);

/* ---- The same verifier over BLS12-377: ark_groth16::prepare_verifying_key + verify_proof over Bls12_377, the check of the hash-helper
 * proof (crates/epoch-snark/src/api/prover.rs:83-118) that a prover pipeline makes BEFORE it computes the BW6-761 proof over it - a helper
 * proof that does not verify makes the outer circuit unsatisfiable.  One template with the BW6-761 entries above (csrc/groth16_verify_unit.h):
 * the contract, the modes, the exponents, the limits and the return codes are theirs word for word; what differs is the shape of the data.
 * Rows: G1 12 u64, G2 24 u64 (c0 then c1 per coordinate, as msm_bls12_377_g2 takes them); inputs: m x (n_abc - 1) x 4 u64, canonical
 * integers below the 253-bit r.  Serialized key: alpha_g1 (48 B) | beta_g2 (96) | gamma_g2 (96) | delta_g2 (96) | u64 LE n_abc |
 * gamma_abc_g1 (48 each); serialized proof: A (48) | B (96) | C (48) = 192 B; decoded and checked as `deserialize` does
 * (decompress_bls12_377_*_dev, check_subgroup = 1).
 * Window tables: entries are 2 x 16 words (the 14 limbs of a coordinate in the field's stored form), 128 B; the widest of 10 .. 4 bits whose
 * tables fit 64 MiB is 10 bits up to 39 inputs and 9 bits from 40 to 64.
 * Wide keys.  groth16_vk_load_bls12_377_wide[_serialized] take the arguments and return the codes of the two loaders above, and accept up to
 * 1024 public inputs (n_abc <= 1025; 36 above) where those stop at 64: the hash-helper proof of n epochs has ceil(384 n / 252) + ceil(512 n / 252)
 * inputs, 509 at the production size of 143 epochs.  The window rule is the same; the last input count of 10 .. 4 bits is 39 | 70 | 128 | 221 | 381 |
 * 642 | 1024 (1024 inputs at 4 bits fill the 64 MiB exactly; 143 epochs get 5 bits, 287 epochs with 1022 inputs are the most that fit).  The
 * handle is an ordinary BLS12-377 handle: every entry here, groth16_vk_free and celo_amd_groth16_verify_last take it; a BW6-761 entry
 * refuses it with 2.  Past 64 inputs one lane per proof is too little (509 inputs at 5 bits: about 26 000 dependent additions), so the
 * input sums of such a key are the work of L lanes per proof, folded through LDS (csrc/groth16_verify.h g16_pick_lanes: L follows the input
 * count and falls as the batch grows; a key of at most 64 inputs keeps the one-lane kernel).
 * celo_amd_groth16_set_input_lanes: a test and tuning switch, no device call.  0: the rule; 1, 2, 4, .. 256: every later BLS12-377 verify
 * call of the process runs its input sums with that many lanes per proof, whatever the key.  2: any other value.
 * celo_amd_groth16_inputs_last: the lanes per input sum and the key's public-input count of the last successful verify call (either
 * curve; BW6-761 always reports 1 lane).  2: a NULL pointer.
 * groth16_vk_free, celo_amd_groth16_draw_exponents and celo_amd_groth16_verify_last serve both curves.  A handle knows its curve: a
 * BLS12-377 handle given to a BW6-761 entry, or the reverse, returns 2 before anything is read.
 * Dispatch: a product of four pairs is one more than the BLS12-377 latency path takes, so mode 0 runs the per-pair lane kernels below
 * 16 384 proofs and the shared-accumulator kernel from there; the combined product of m + 3 pairs takes the 8-pair product up to m = 5 and the
 * pairwise tree from m = 6.
 * Choosing a mode (one MI355X, two inputs, profiles/bench_groth16_verify_377.json): a call has a floor of
 * about 4.7 ms (each) and 8.2 ms (combined).  Mode 0 takes 4.76 / 4.87 / 22.9 ms for 64 / 1 024 / 16 421 proofs, mode 1 8.21 / 8.92 / 11.5 ms:
 * combined / each = 1.73, 1.83, 0.50.  Use mode 0 up to a few thousand proofs and mode 1 above (the crossover lies between 1 024 and 16 421
 * proofs and was not bracketed further).  Against the loop of one msm_bls12_377_g1 and one four-pair pairing_product_is_one_bls12_377 per
 * proof (3.80 ms per proof), mode 0 is 51 x cheaper per proof at 64 proofs.
 * groth16_serialize_proof_bls12_377: Proof::serialize (192 B) from the arkworks Jacobian points groth16_prove_bls12_377 /
 * groth16_prove_with_key return (18 / 36 / 18 u64); Z == 0 encodes the identity.  Host only, through the encoders of compress_bls12_377_*.
 * 2: a NULL pointer. */
int groth16_vk_load_bls12_377(const uint64_t alpha_g1[12], const uint64_t beta_g2[24], const uint64_t gamma_g2[24], const uint64_t delta_g2[24],
                              const uint64_t* gamma_abc_g1 /* n_abc x 12 */, size_t n_abc, void** out_vk);
int groth16_vk_load_bls12_377_serialized(const uint8_t* bytes, size_t len, void** out_vk);
int groth16_verify_batch_bls12_377(const void* vk, const uint64_t* a_xy /* m x 12 */, const uint8_t* a_inf, const uint64_t* b_xy /* m x 24 */, const uint8_t* b_inf,
                                   const uint64_t* c_xy /* m x 12 */, const uint8_t* c_inf, const uint64_t* inputs /* m x (n_abc - 1) x 4 */, size_t m, int mode,
                                   const uint32_t* key /* 8, or NULL */, uint8_t* out_ok /* m */);
int groth16_verify_batch_bls12_377_serialized(const void* vk, const uint8_t* proofs /* m x 192 */, const uint64_t* inputs, size_t m, int mode,
                                              const uint32_t* key /* 8, or NULL */, uint8_t* out_ok /* m */);
int groth16_serialize_proof_bls12_377(const uint64_t a_xyz[18], const uint64_t b_xyz[36], const uint64_t c_xyz[18], uint8_t out[192]);
int groth16_vk_load_bls12_377_wide(const uint64_t alpha_g1[12], const uint64_t beta_g2[24], const uint64_t gamma_g2[24], const uint64_t delta_g2[24],
                                   const uint64_t* gamma_abc_g1 /* n_abc x 12 */, size_t n_abc, void** out_vk);
int groth16_vk_load_bls12_377_wide_serialized(const uint8_t* bytes, size_t len, void** out_vk);
int celo_amd_groth16_set_input_lanes(int lanes);
int celo_amd_groth16_inputs_last(int* lanes, int* n_inputs);

/* ---- bulk ENCODING into the same wire form: n affine points (arkworks Montgomery limbs, the rows the decoders, normalize_* and the MSM
 * entry points use) -> n encodings, one point per GPU lane.  Replaces n calls of GroupAffine::serialize (compress_*: x little-endian with
 * 0x80 on the last byte when y is the lexicographically larger of (y, -y)) or serialize_uncompressed (encode_uncompressed_*: x then y, no
 * sign bit) - ark-serialize 0.1 CanonicalSerialize; the identity is all-zero bytes with 0x40 on the last byte in both forms.
 * A row is the identity when inf != NULL && inf[i] != 0, or when the row is all zero (what normalize_* and the decoders emit; never a
 * point of these curves).  A row (0, 1) is a pair of field elements like any other here.  inf may be NULL.
 * status[i]: 0 encoded; 1 identity written; 2 a coordinate's limbs are not below q - not a field element: the output row is all zero,
 * no flag.  Neither the curve equation nor the subgroup is checked, as arkworks checks neither when it serializes.
 * compress_bw6_761 / encode_uncompressed_bw6_761 serve G1 and G2 of BW6-761 (one coordinate field, and the encoding does not involve the
 * curve constant).  Returns 0; 2: n > 2^31 - 1, a required pointer NULL, or a _dev rows / output pointer that is not 8-byte aligned (the
 * kernels move 64-bit words); 10: allocation failure; 100: no device.  n == 0 returns 0.  The _dev forms take device pointers and run
 * on hip_stream (0: the null stream); calls are serialised per process. */
int compress_bls12_377_g1(const uint64_t* rows /* n x 12 */, const uint8_t* inf, size_t n, uint8_t* out /* n x 48 */, uint8_t* status /* n */);
int compress_bls12_377_g2(const uint64_t* rows /* n x 24 */, const uint8_t* inf, size_t n, uint8_t* out /* n x 96 */, uint8_t* status /* n */);
int encode_uncompressed_bls12_377_g1(const uint64_t* rows /* n x 12 */, const uint8_t* inf, size_t n, uint8_t* out /* n x 96 */, uint8_t* status /* n */);
int encode_uncompressed_bls12_377_g2(const uint64_t* rows /* n x 24 */, const uint8_t* inf, size_t n, uint8_t* out /* n x 192 */, uint8_t* status /* n */);
int compress_bw6_761(const uint64_t* rows /* n x 24 */, const uint8_t* inf, size_t n, uint8_t* out /* n x 96 */, uint8_t* status /* n */);
int encode_uncompressed_bw6_761(const uint64_t* rows /* n x 24 */, const uint8_t* inf, size_t n, uint8_t* out /* n x 192 */, uint8_t* status /* n */);
int compress_bls12_377_g1_dev(const uint64_t* d_rows, const uint8_t* d_inf, size_t n, uint8_t* d_out, uint8_t* d_status, void* hip_stream);
int compress_bls12_377_g2_dev(const uint64_t* d_rows, const uint8_t* d_inf, size_t n, uint8_t* d_out, uint8_t* d_status, void* hip_stream);
int encode_uncompressed_bls12_377_g1_dev(const uint64_t* d_rows, const uint8_t* d_inf, size_t n, uint8_t* d_out, uint8_t* d_status, void* hip_stream);
int encode_uncompressed_bls12_377_g2_dev(const uint64_t* d_rows, const uint8_t* d_inf, size_t n, uint8_t* d_out, uint8_t* d_status, void* hip_stream);
int compress_bw6_761_dev(const uint64_t* d_rows, const uint8_t* d_inf, size_t n, uint8_t* d_out, uint8_t* d_status, void* hip_stream);
int encode_uncompressed_bw6_761_dev(const uint64_t* d_rows, const uint8_t* d_inf, size_t n, uint8_t* d_out, uint8_t* d_status, void* hip_stream);
/* ---- the writers of what groth16_load_key_bw6_761_serialized and Seam A's verify read.
 * groth16_serialize_key_bw6_761: ProvingKey::<BW6_761>::serialize (form 0) / serialize_uncompressed (form 1) from the out_vk / out_rows
 * buffers of groth16_setup_bw6_761 (vk: alpha_g1, beta_g2, gamma_g2, delta_g2, n_inputs rows of gamma_abc_g1; rows: beta_g1, delta_g1,
 * a_query[n_vars], b_g1_query[n_vars], b_g2_query[n_vars], h_query[n_h], l_query[n_vars - n_inputs]; 24 u64 each), in the layout
 * groth16_key_layout_bw6_761 parses.  rows == NULL: VerifyingKey::serialize of vk alone (n_vars and n_h are not looked at).  The rows cross
 * to the device once, every contiguous run of points is encoded there straight to its byte offset, the bytes cross back once.  Here a row
 * (0, 1 in Montgomery form) - arkworks' GroupAffine::zero(), what groth16_setup_* emits - is the identity too, as for groth16_load_key_*.
 * *out_len is the size of the serialization whenever the counts are valid.  Returns 0; 2: a NULL vk / out / out_len, form not 0 or 1,
 * n_inputs == 0, n_inputs > n_vars, more than 2^31 - 1 points; 35: cap < *out_len; 33: a row that is no pair of field elements (limbs not
 * below q), *first_bad_point (may be NULL) = its index in serialization order, the index space of groth16_load_key_bw6_761_serialized -
 * with 35 and with 33 nothing is written to out; 10: allocation failure; 100: no device.  Nothing is kept allocated on any path.
 * groth16_serialized_key_size_bw6_761: that size from the counts alone (no device call); vk_only != 0: the VerifyingKey's.
 * groth16_serialize_proof_bw6_761: Proof::serialize (A, B, C compressed, 288 B: the `proof` argument of verify) from the arkworks Jacobian
 * points groth16_prove_* returns; Z == 0 encodes the identity.  Host only (three points, the same encoder).  2: a NULL pointer. */
int groth16_serialized_key_size_bw6_761(size_t n_inputs, size_t n_vars, size_t n_h, int form, int vk_only, uint64_t* len);
int groth16_serialize_key_bw6_761(const uint64_t* vk, size_t n_inputs, const uint64_t* rows /* NULL: the VerifyingKey alone */, size_t n_vars, size_t n_h,
                                  int form /* 0 compressed, 1 uncompressed */, uint8_t* out, size_t cap, uint64_t* out_len, uint64_t* first_bad_point /* NULL allowed */);
int groth16_serialize_proof_bw6_761(const uint64_t a_xyz[36], const uint64_t b_xyz[36], const uint64_t c_xyz[36], uint8_t out[288]);
/* The same writer and size function for ProvingKey<Bls12_377> / VerifyingKey<Bls12_377>, from the out_vk / out_rows buffers of
 * groth16_setup_bls12_377 and groth16_setup_r1cs_bls12_377 in their documented order: G1 rows are 12 u64, the G2 rows (beta_g2, gamma_g2,
 * delta_g2 and those of b_g2_query) 24 u64.  The layout is the one groth16_key_layout_bls12_377 parses; with rows == NULL the output is what
 * groth16_vk_load_bls12_377_serialized reads.  Forms, return codes, the (0, 1) identity rule and first_bad_point as above. */
int groth16_serialized_key_size_bls12_377(size_t n_inputs, size_t n_vars, size_t n_h, int form, int vk_only, uint64_t* len);
int groth16_serialize_key_bls12_377(const uint64_t* vk, size_t n_inputs, const uint64_t* rows /* NULL: the VerifyingKey alone */, size_t n_vars, size_t n_h,
                                    int form /* 0 compressed, 1 uncompressed */, uint8_t* out, size_t cap, uint64_t* out_len, uint64_t* first_bad_point /* NULL allowed */);
/* kernel time in ms of the last compress_* / encode_uncompressed_* call (or of the last key writer's launches); the last
 * groth16_serialize_key_bw6_761 call's three phases: rows to the device, encoding, bytes back (what tools/bench_wire_encode.py reports). */
int celo_amd_wire_encode_last_ms(float* ms);
int celo_amd_wire_encode_key_timings(float ms[3]);

/* ---- batched hash-to-G1, DIRECT hasher: n messages per launch, one per GPU lane.
 * Replaces n calls of TryAndIncrement<DirectHasher, G1>::hash_with_attempt(domain, message, extra_data)
 * (crates/bls-crypto/src/hash_to_curve/try_and_increment.rs:87-139; DirectHasher = Blake2s CRH + Blake2Xs XOF,
 * crates/bls-crypto/src/hashers/direct.rs:23-80) as Signature::batch_verify issues them (bls/signature.rs:111-114), with the
 * deployed `compat` bit logic.  domain: the 8-byte personalisation (SIG_DOMAIN "ULforxof" / POP_DOMAIN "ULforpop",
 * crates/bls-crypto/src/lib.rs:75,78).  msgs / extras: concatenated bytes, message i = msgs[msg_off[i] .. msg_off[i+1]),
 * likewise extras (extra_off == NULL: no extra data anywhere).  out_xy: n x 12 u64, affine (x, y) in arkworks Montgomery
 * limbs (the G1 layout of the MSM / pairing entry points); attempts[i]: the counter that produced the point, 255 = no
 * counter below 255 did (the reference returns an error there; out row zero). */
int hash_to_g1_direct_bls12_377(const uint8_t domain[8], const uint8_t* msgs, const uint64_t* msg_off /* n+1 */, const uint8_t* extras,
                                const uint64_t* extra_off /* n+1 or NULL */, size_t n, uint64_t* out_xy /* n x 12 */, uint8_t* attempts /* n */);
/* The try-and-increment loop of the CIP22 hashers (crates/bls-crypto/src/hash_to_curve/try_and_increment_cip22.rs:81-134), n
 * messages per launch: the caller computes the inner CRH of each message once (for the composite hasher: hash_crh of
 * include/celo_bls_snark_sys.h, 48 bytes), this entry point runs candidate = xof(domain, counter || extra_data || inner) ->
 * curve point -> cofactor for every message.  Same layout and result conventions as hash_to_g1_direct_bls12_377. */
int hash_to_g1_cip22_tail_bls12_377(const uint8_t domain[8], const uint8_t* inner, const uint64_t* inner_off /* n+1 */, const uint8_t* extras,
                                    const uint64_t* extra_off /* n+1 or NULL */, size_t n, uint64_t* out_xy /* n x 12 */, uint8_t* attempts /* n */);
/* Batched hash-to-G1 with the COMPOSITE hasher (Pedersen CRH + Blake2Xs XOF), n messages per call: cip22 == 0:
 * TryAndIncrement<CompositeHasher, G1>::hash_with_attempt (try_and_increment.rs:87-139: a CRH of counter || extra || message per
 * attempt); cip22 != 0: the CIP22 form (try_and_increment_cip22.rs:81-134: one CRH per message, then
 * hash_to_g1_cip22_tail_bls12_377).  What hash_composite / hash_composite_cip22 of the bls-snark-sys ABI compute for one
 * message (signatures.rs:143,215).  Layout and results as hash_to_g1_direct_bls12_377. */
int hash_to_g1_composite_bls12_377(const uint8_t domain[8], const uint8_t* msgs, const uint64_t* msg_off /* n+1 */, const uint8_t* extras,
                                   const uint64_t* extra_off /* n+1 or NULL */, size_t n, int cip22, uint64_t* out_xy /* n x 12 */, uint8_t* attempts /* n */);
/* The composite hasher's CRH for n messages in one launch: the Bowe-Hopwood-Pedersen hash over ed-on-BW6-761 that
 * CompositeHasher::crh evaluates (crates/bls-crypto/src/hashers/composite.rs:79-86; hash_crh of the bls-snark-sys ABI,
 * signatures.rs:169, is the one-message form).  out48: n x 48 bytes, the affine x coordinate little-endian.  A message longer
 * than 93 * 560 * 3 bits is an error for the whole call (the reference panics). */
int composite_crh_bls12_377(const uint8_t* msgs, const uint64_t* msg_off /* n+1 */, size_t n, uint8_t* out48 /* n x 48 */);
/* The device-resident forms of the four entries above, for a caller whose messages are made on the GPU and whose rows are read there (the
 * chain check below is one): d_msgs / d_inner, d_extras, d_out48, d_out_xy and d_attempts are DEVICE pointers; the offsets stay HOST arrays,
 * because they size the call and are checked before the device is used.  The work is enqueued on hip_stream (NULL: the null stream), behind
 * whatever the caller has enqueued there, and the call returns after it has drained.  Results, refusals and return codes are those of the
 * host forms, byte for byte; a CIP22 call (cip22 != 0) keeps its 48-byte CRH rows on the device between its two steps, and
 * d_out48 of composite_crh_bls12_377_dev can be handed to hash_to_g1_cip22_tail_bls12_377_dev as d_inner with inner_off[i] = 48 i.
 * A message whose cofactor multiple is the identity (probability 2^-125) is finished by the host's serial loop: that message alone is
 * fetched, and its row and counter are written back. */
int composite_crh_bls12_377_dev(const void* d_msgs, const uint64_t* msg_off /* n+1, host */, size_t n, void* d_out48 /* n x 48 */, void* hip_stream);
int hash_to_g1_direct_bls12_377_dev(const uint8_t domain[8], const void* d_msgs, const uint64_t* msg_off /* n+1, host */, const void* d_extras,
                                    const uint64_t* extra_off /* n+1 or NULL, host */, size_t n, void* d_out_xy /* n x 12 u64 */, void* d_attempts /* n */,
                                    void* hip_stream);
int hash_to_g1_cip22_tail_bls12_377_dev(const uint8_t domain[8], const void* d_inner, const uint64_t* inner_off /* n+1, host */, const void* d_extras,
                                        const uint64_t* extra_off /* n+1 or NULL, host */, size_t n, void* d_out_xy /* n x 12 u64 */, void* d_attempts /* n */,
                                        void* hip_stream);
int hash_to_g1_composite_bls12_377_dev(const uint8_t domain[8], const void* d_msgs, const uint64_t* msg_off /* n+1, host */, const void* d_extras,
                                       const uint64_t* extra_off /* n+1 or NULL, host */, size_t n, int cip22, void* d_out_xy /* n x 12 u64 */,
                                       void* d_attempts /* n */, void* hip_stream);
/* ---- batched hash-to-G2: the same hashers and loops onto the twist over Fq2 - TryAndIncrement<H, G2> / TryAndIncrementCIP22<H, G2>
 * (try_and_increment.rs:63-140, try_and_increment_cip22.rs:75-135; the reference pins ten outputs, hash_to_curve/mod.rs:490-513).  A candidate
 * is 96 XOF bytes (hash_length(96) = 96: every node offset carries 96); the winning point is multiplied by the 502-bit cofactor of the twist.
 * Arguments, layouts and return codes are those of the hash_to_g1_* entries, except: out_xy is n x 24 u64 (x.c0, x.c1, y.c0, y.c1 in arkworks
 * Montgomery limbs, the G2 layout of the MSM / pairing entry points), and compat selects the flag logic: 0 = the y-sign flag is bit 7 of byte
 * 95 as the XOF gives it (the reference's vectors), 1 = the deployed remap, bit 1 of byte 95 copied into bit 7 first
 * (try_and_increment.rs:107-120).  Any other compat value returns 2. */
int hash_to_g2_direct_bls12_377(const uint8_t domain[8], const uint8_t* msgs, const uint64_t* msg_off /* n+1 */, const uint8_t* extras,
                                const uint64_t* extra_off /* n+1 or NULL */, size_t n, int compat, uint64_t* out_xy /* n x 24 */, uint8_t* attempts /* n */);
int hash_to_g2_cip22_tail_bls12_377(const uint8_t domain[8], const uint8_t* inner, const uint64_t* inner_off /* n+1 */, const uint8_t* extras,
                                    const uint64_t* extra_off /* n+1 or NULL */, size_t n, int compat, uint64_t* out_xy /* n x 24 */, uint8_t* attempts /* n */);
int hash_to_g2_composite_bls12_377(const uint8_t domain[8], const uint8_t* msgs, const uint64_t* msg_off /* n+1 */, const uint8_t* extras,
                                   const uint64_t* extra_off /* n+1 or NULL */, size_t n, int cip22, int compat, uint64_t* out_xy /* n x 24 */,
                                   uint8_t* attempts /* n */);
/* One message through the serial loop on the HOST: no device is touched, so it works on a machine without a GPU.  mode: 0 direct, 1 the
 * CIP22 tail (msg is the inner CRH), 2 composite, 3 composite CIP22.  *attempt = 255 and a zero row when no counter below 255 gives a point. */
int hash_to_g2_one_bls12_377(const uint8_t domain[8], const uint8_t* msg, size_t mlen, const uint8_t* extra, size_t elen, int mode, int compat,
                             uint64_t out_xy[24], int* attempt);
/* The lane budget of the hash_to_g2_* rounds: every round gives each open message the widest power of two of counters, at most 16, with
 * open * width <= 2^log.  Default 17 (what hash_to_g1_* uses); 4 ... 17 accepted, anything else returns 2.  A test hook: at 8 the widths
 * 16 / 8 / 4 / 2 / 1 are reached at 16 / 32 / 64 / 128 / 129+ messages. */
int celo_amd_hash_g2_set_lane_budget_log(int log);
/* the last hash_to_g2_* call's kernel time in two parts: ms[0] the candidate rounds (with the host's round trips between them), ms[1] the
 * cofactor kernel */
int celo_amd_hash_g2_last_split(float ms[2]);
/* kernel time (HIP events) of the last hash_to_g1_* or hash_to_g2_* call */
int celo_amd_hash_last_ms(float* ms);
/* candidate rounds (launches of the try-and-increment kernel) of the last hash_to_g1_* or hash_to_g2_* call that hashed at least one
 * message: each round gives every message still open 1, 2, 4, 8 or 16 adjacent counters, the width chosen from how many are open */
int celo_amd_hash_last_rounds(int* rounds);
/* Lanes per message of the CRH kernel behind composite_crh_bls12_377[_dev], the CIP22 composite entries of both groups and every pipeline
 * that hashes through them (signing, aggregated seals, chains of epoch transitions): lane l of L sums the chunks l (mod L) of its message
 * and the L partial sums are folded in the workgroup; the hash is the x of a sum in a group, so every width gives the same 48 bytes.
 * 0 (the default) = the rule: L = min(smallest power of two >= chunks of the longest message / 32, largest power of two <= 2^16 / n),
 * one width per call; a call of 2^16 messages or more runs one lane per message.  1, 2, 4 ... 256 force a width (halved while n x L
 * lanes exceed a 31-bit grid of workgroups); anything else returns 2 and changes nothing.  Needs no device.  Not used by the per-attempt
 * CRH of the composite mode without CIP22, which stays one lane per attempt. */
int celo_amd_crh_set_lanes(int lanes);
/* the width the last CRH kernel of this process ran with (0 before the first); NULL returns 2.  Needs no device. */
int celo_amd_crh_last_lanes(int* lanes);

/* ---- plain sums of k Jacobian points (host pointers, arkworks layout; host-side, for small k): the fold of per-GPU
 * partial MSM results and small aggregates — Signature::aggregate / PublicKey::aggregate
 * (crates/bls-crypto/src/bls/signature.rs:61-67, public.rs:38-44). */
int celo_amd_sum_jacobian_bls12_377_g1(const uint64_t* jac /* k*18 */, size_t k, uint64_t out_xyz[18]);
int celo_amd_sum_jacobian_bls12_377_g2(const uint64_t* jac /* k*36 */, size_t k, uint64_t out_xyz[36]);
int celo_amd_sum_jacobian_bw6_761(const uint64_t* jac /* k*36 */, size_t k, uint64_t out_xyz[36]);

/* ---- instrumentation (bench.py / tests).  group: 0 = bls12_377_g1, 1 = bls12_377_g2, 2 = bw6_761.
 * ms[5] = {convert, sort, accumulate, reduce, total} of the last MSM on that engine, from HIP events recorded on the
 * MSM's own stream; cfg[3] = {window bits c, windows, buckets}. */
int celo_amd_msm_last_timings(int group, float ms[5], int cfg[3]);
/* Self-test of the bucket-accumulation kernels the library runs (tests/test_msm_gpu.py): `runs` runs of `len` random signed multiples of the
 * affine generator gen_xy (HOST pointer, arkworks layout) through k_accumulate<group> (chunked = 0) or through the host-pointer pipeline's
 * k_accumulate_chunk<group> twice, the second launch continuing the first's carried sums (chunked = 1); the first `check` partial sums are
 * compared limb for limb with the same formulas run on the host.  *differ = the number of runs that disagree (0 expected). */
int celo_amd_selftest_accumulate(int group, const uint64_t* gen_xy, uint32_t runs, uint32_t len, uint32_t seed, uint32_t check, int chunked, uint32_t* differ);
/* The multiplier roofline of THIS device in THIS process (bench.py's valu_roofline.peak): chip-wide rate of the library's own field-product
 * bodies in register-resident loops (csrc/unit_ubench.hip; ~0.3 s).  out[0..3] = 1e9 products/s: Fq(BLS12-377) mul, sqr, Fq(BW6-761) mul,
 * sqr; out[4] = shader clock in MHz during the first loop (s_memtime against the 100 MHz s_memrealtime); out[5..8] = the loops' kernel ms. */
int celo_amd_ubench_fp(float out[9]);
/* Forces the Pippenger window size (0 = automatic) — tuning and test hook.  c = 4..16 for the large pipeline; the batched kernels
 * (msm_batch_*) clamp it to their 3..7, and c = 3 applies to them alone (the large pipeline stays automatic). */
int celo_amd_msm_set_window_bits(int group, int c);
/* Host-pointer entry points (msm_<group>, from 2^18 terms - 2^17 when the count is set here): the number of index chunks in which scalars and bases cross PCIe while the
 * chunks already on the device are sorted and accumulated (csrc/msm.h HostIn).  0 = the unpipelined form (three transfers, then
 * the resident pipeline; 1 = one chunk: the sort runs beside the bases' transfer), -1 = the default (CELO_HOST_CHUNKS, else n / 2^18 within [4, 16] - [8, 16] for BW6-761, n / 2^19 within [4, 8] for G2 of BLS12-377).  The first chunk is cut
 * in halves once where the halves keep 2^17 points (else not at all), the last one never; `chunks | (h + 1) << 8 | (t + 1) << 12`
 * sets those counts to h and t (0 <= h, t <= 8) as well.  Process-wide — tuning and test hook. */
int celo_amd_msm_set_host_chunks(int chunks);
/* The BW6-761 bucket accumulation of the resident entry points (msm_bw6_761_*_dev, and msm_bw6_761_* below 2^18 terms): 1 = three batched-affine
 * tree levels before the XYZZ chain (csrc/msm_ba.h), 0 = the XYZZ chain alone, -1 = the default (CELO_BA, else 0: the two measure alike on
 * config 4, profiles/r6_ba_ab.txt).  Same group element either way.  Process-wide - test and measurement hook; 1 for an argument out of range. */
int celo_amd_msm_set_batched_affine(int on);
/* The chunk plan the pipelined host-pointer entry uses for n terms (pure host arithmetic, no device call - csrc/runtime.h host_chunk_plan):
 * returns the number of chunks K (<= 80) and their lengths lens[0..K) in the order they are sent, *cm = the chunk capacity (chunk k sits at
 * the virtual index k * cm on the device); -1 for arguments the entry points would not pipeline (chunks < 1 or > 64, n < chunks * 2^16, n >= 2^30; chunks = 1 is the one-chunk pipelined form celo_amd_msm_set_host_chunks(1) runs). */
int celo_amd_msm_host_chunk_plan(uint64_t n, int chunks, int head_split, int tail_split, uint32_t* cm, uint32_t lens[80]);

/* ---- synthetic-workload generators (bench / tests only): writes n affine points
 * P_i = k_i * G into DEVICE memory in the arkworks layout, k_i = 64-bit splitmix64(seed, i) | 1.
 * gen_xy: the generator G, affine, HOST pointer, arkworks layout. */
int celo_amd_gen_points_bls12_377_g1_dev(void* d_out_xy, size_t n, uint64_t seed, const uint64_t* gen_xy, void* stream);
int celo_amd_gen_points_bls12_377_g2_dev(void* d_out_xy, size_t n, uint64_t seed, const uint64_t* gen_xy, void* stream);
int celo_amd_gen_points_bw6_761_dev(void* d_out_xy, size_t n, uint64_t seed, const uint64_t* gen_xy, void* stream);
/* The same with one generator per group of `per` consecutive points: P_i = k_i * gens[i / per] (ngens >= ceil(n / per) affine
 * generators, HOST pointer).  Builds VALID Batch::verify inputs without a host big-int loop: the
 * signatures of batch b = k_{b,j} * H(m_b) with gens = the message hashes, the keys = k_{b,j} * g2 from the same seed. */
int celo_amd_gen_points_grouped_bls12_377_g1_dev(void* d_out_xy, size_t n, uint64_t seed, const uint64_t* gens_xy, size_t ngens, uint32_t per, void* stream);
int celo_amd_gen_points_grouped_bls12_377_g2_dev(void* d_out_xy, size_t n, uint64_t seed, const uint64_t* gens_xy, size_t ngens, uint32_t per, void* stream);

/* ---- batched fixed-base scalar multiplication (ark-ec FixedBaseMSM::multi_scalar_mul, the work of ark_groth16::generate_random_parameters at
 * crates/epoch-snark/src/api/setup.rs:22-46,63-105; csrc/fixed_base.h, csrc/unit_setup.hip): out_i = k_i * G for ONE
 * generator G and n scalars, n affine rows (not msm_*_fixed, which returns one sum).  The generator's table (d * 2^(c w) * G, signed digits) is
 * built on the device per call; one lane per scalar, one mixed addition per nonzero digit, a batch normalisation at the end.
 * scalars: n canonical integers below r (4 u64 BLS12-377, 6 u64 BW6-761), as msm_* take them; a scalar >= r -> 2, nothing written.
 * gen_xy: affine generator, arkworks Montgomery limbs (must not be the identity: 2).  out_xy: n affine rows; k_i = 0 -> zero row, inf[i] = 1.
 * Both BW6-761 groups share one coordinate field and group law.  The _dev forms take device scalars / rows / flags and run on hip_stream. */
int fixed_base_mul_bls12_377_g1(const uint64_t gen_xy[12], const uint64_t* scalars, size_t n, uint64_t* out_xy, uint8_t* inf);
int fixed_base_mul_bls12_377_g2(const uint64_t gen_xy[24], const uint64_t* scalars, size_t n, uint64_t* out_xy, uint8_t* inf);
int fixed_base_mul_bw6_761_g1(const uint64_t gen_xy[24], const uint64_t* scalars, size_t n, uint64_t* out_xy, uint8_t* inf);
int fixed_base_mul_bw6_761_g2(const uint64_t gen_xy[24], const uint64_t* scalars, size_t n, uint64_t* out_xy, uint8_t* inf);
int fixed_base_mul_bls12_377_g1_dev(const uint64_t* gen_xy, const void* d_scalars, size_t n, void* d_out_xy, void* d_inf, void* hip_stream);
int fixed_base_mul_bls12_377_g2_dev(const uint64_t* gen_xy, const void* d_scalars, size_t n, void* d_out_xy, void* d_inf, void* hip_stream);
int fixed_base_mul_bw6_761_g1_dev(const uint64_t* gen_xy, const void* d_scalars, size_t n, void* d_out_xy, void* d_inf, void* hip_stream);
int fixed_base_mul_bw6_761_g2_dev(const uint64_t* gen_xy, const void* d_scalars, size_t n, void* d_out_xy, void* d_inf, void* hip_stream);
/* Jacobian -> affine for n BW6-761 points (the twin of normalize_bls12_377_*): jac n x 36 u64, out_xy n x 24, identity -> zero row, inf = 1 */
int normalize_bw6_761_g1(const uint64_t* jac /* n x 36 */, size_t n, uint64_t* out_xy /* n x 24 */, uint8_t* inf /* n */);
int normalize_bw6_761_g2(const uint64_t* jac /* n x 36 */, size_t n, uint64_t* out_xy /* n x 24 */, uint8_t* inf /* n */);
/* ---- Groth16 parameter generation after the QAP evaluation at tau (ark-groth16 0.1 generate_parameters; the caller turns its R1CS into
 * data, as for the prover).  qap_a / qap_b / qap_c: a_i(tau), b_i(tau), c_i(tau) for n_vars variables (the one variable and the
 * input-consistency rows included), arkworks Montgomery Fr (6 u64 BW6-761, 4 u64 BLS12-377); n_inputs: instance variables, the one included;
 * zt = Z(tau); tau and n_h: h_query_i = zt delta^-1 tau^i for i < n_h; toxic: alpha, beta, gamma, delta (Montgomery Fr); g1_xy / g2_xy: the
 * generators (affine arkworks limbs; ark 0.1 draws them at random).  On the device:
 *   gamma_abc_i = (beta a_i + alpha b_i + c_i) gamma^-1 (i < n_inputs), l_i = (...) delta^-1 (i >= n_inputs), h_i as above,
 *   every row of the key one fixed-base multiplication (G1: a_query, b_g1_query, h_query, l_query, gamma_abc_g1, alpha, beta, delta; G2:
 *   b_g2_query, beta, gamma, delta).
 * out_vk (NULL allowed): alpha_g1, beta_g2, gamma_g2, delta_g2, then n_inputs rows of gamma_abc_g1.
 * out_rows (NULL allowed): beta_g1, delta_g1, a_query[n_vars], b_g1_query[n_vars], b_g2_query[n_vars], h_query[n_h], l_query[n_vars - n_inputs]
 * (ProvingKey field order after the vk).  Rows: G1 24 u64 (BW6-761) / 12 u64 (BLS12-377), G2 24 u64.  Identity rows are arkworks'
 * GroupAffine::zero() coordinates x = 0, y = 1 (Montgomery): the identity rule of groth16_load_key_*.
 * out_key (NULL allowed): the handle groth16_load_key_* would build from those rows with the same window_bits, built from the device-resident
 * rows (no query crosses PCIe); bound to the device, freed with groth16_free_key.
 * Returns 0; 2: n_inputs == 0, n_inputs > n_vars, gamma or delta zero, a generator that is the identity, all three outputs NULL;
 * 10: device allocation failure.  On any failure everything is freed and *out_key is not written beyond NULL. */
int groth16_setup_bw6_761(const uint64_t* qap_a, const uint64_t* qap_b, const uint64_t* qap_c /* n_vars x 6 */, size_t n_vars, size_t n_inputs,
                          const uint64_t zt[6], const uint64_t tau[6], size_t n_h, const uint64_t toxic[24] /* alpha beta gamma delta */,
                          const uint64_t g1_xy[24], const uint64_t g2_xy[24], int window_bits, uint64_t* out_vk, uint64_t* out_rows, void** out_key);
int groth16_setup_bls12_377(const uint64_t* qap_a, const uint64_t* qap_b, const uint64_t* qap_c /* n_vars x 4 */, size_t n_vars, size_t n_inputs,
                            const uint64_t zt[4], const uint64_t tau[4], size_t n_h, const uint64_t toxic[16], const uint64_t g1_xy[12],
                            const uint64_t g2_xy[24], int window_bits, uint64_t* out_vk, uint64_t* out_rows, void** out_key);
/* the generator tables' window bits c (0 = the default of DESIGN.md 6f, else 2 .. 14) and the last fixed_base_mul_* / groth16_setup_* call's
 * times in ms: [0] table build, [1] Fr preparation, [2] G1 rows, [3] G2 rows, [4] normalisation, [5] key tables, [6] wall, [7] unused */
int celo_amd_fixed_base_set_window(int window_bits);
int celo_amd_setup_last_timings(float ms[8]);

/* ---- Batched variable-base scalar multiplication out_i = [k_i] P_i: n points, each with its own scalar (PrivateKey::sign = hash * sk,
 * crates/bls-crypto/src/bls/secret.rs:65; the sign_batch / keygen_mul helpers of crates/bls-crypto/src/test_helpers.rs:20,54; re-randomising
 * points, blinding a list of keys).  csrc/var_base.h, csrc/unit_varbase.hip, DESIGN.md section 6i.
 * xy: n affine points in arkworks Montgomery limbs (12 u64 for BLS12-377 G1, 24 for the other groups); inf: n identity flags, or NULL for none.
 * P_i is ANY point of the curve, not only the prime-order subgroup (points off the curve are not validated, as elsewhere).
 * scalars: n_scalars x (4 | 6) u64, canonical and below the group order r; n_scalars is n, or 1: every row then uses scalars[0] (one key, many
 * messages) and the scalar is not copied.
 * out_xy / out_inf: the row format of fixed_base_mul_*: affine arkworks limbs, and a zero row with inf = 1 for the identity.
 * _subgroup (BLS12-377 G1 only): the CALLER vouches that every P_i lies in the prime-order subgroup - the contract of
 * msm_bls12_377_g1_subgroup.  The scalar is split k = k0 + k1 x^2 and [k]P = [k0]P + [k1](beta x, -y), the halves sharing ~127 doublings
 * instead of 253; the result is the same group element, so the same row bit for bit.  With a point outside the subgroup the result is
 * unspecified.  G2 and BW6-761 have the plain path only (their endomorphism forms are not implemented here).
 * _dev: every pointer is a DEVICE pointer, the work is enqueued on hip_stream and the call returns after it has drained.
 * Returns 0 (also for n = 0); 2 with NOTHING written: a NULL xy / scalars / output, n_scalars not in {1, n}, a scalar >= r; 1 / 10: HIP errors. */
int scalar_mul_batch_bls12_377_g1(const uint64_t* xy /* n x 12 */, const uint8_t* inf /* n or NULL */, const uint64_t* scalars /* n_scalars x 4 */,
                                  size_t n_scalars, size_t n, uint64_t* out_xy, uint8_t* out_inf);
int scalar_mul_batch_bls12_377_g1_subgroup(const uint64_t* xy /* n x 12 */, const uint8_t* inf, const uint64_t* scalars /* n_scalars x 4 */,
                                           size_t n_scalars, size_t n, uint64_t* out_xy, uint8_t* out_inf);
int scalar_mul_batch_bls12_377_g2(const uint64_t* xy /* n x 24 */, const uint8_t* inf, const uint64_t* scalars /* n_scalars x 4 */, size_t n_scalars,
                                  size_t n, uint64_t* out_xy, uint8_t* out_inf);
int scalar_mul_batch_bw6_761_g1(const uint64_t* xy /* n x 24 */, const uint8_t* inf, const uint64_t* scalars /* n_scalars x 6 */, size_t n_scalars,
                                size_t n, uint64_t* out_xy, uint8_t* out_inf);
int scalar_mul_batch_bw6_761_g2(const uint64_t* xy /* n x 24 */, const uint8_t* inf, const uint64_t* scalars /* n_scalars x 6 */, size_t n_scalars,
                                size_t n, uint64_t* out_xy, uint8_t* out_inf);
int scalar_mul_batch_bls12_377_g1_dev(const void* d_xy, const void* d_inf, const void* d_scalars, size_t n_scalars, size_t n, void* d_out_xy,
                                      void* d_out_inf, void* hip_stream);
int scalar_mul_batch_bls12_377_g1_subgroup_dev(const void* d_xy, const void* d_inf, const void* d_scalars, size_t n_scalars, size_t n, void* d_out_xy,
                                               void* d_out_inf, void* hip_stream);
int scalar_mul_batch_bls12_377_g2_dev(const void* d_xy, const void* d_inf, const void* d_scalars, size_t n_scalars, size_t n, void* d_out_xy,
                                      void* d_out_inf, void* hip_stream);
int scalar_mul_batch_bw6_761_g1_dev(const void* d_xy, const void* d_inf, const void* d_scalars, size_t n_scalars, size_t n, void* d_out_xy,
                                    void* d_out_inf, void* hip_stream);
int scalar_mul_batch_bw6_761_g2_dev(const void* d_xy, const void* d_inf, const void* d_scalars, size_t n_scalars, size_t n, void* d_out_xy,
                                    void* d_out_inf, void* hip_stream);
/* Batched signing, sig_i = [sk_i] H(msg_i): the hash of hash_to_g1_* (mode 0 direct, 2 composite, 3 composite CIP22 - the numbering of
 * hash_to_g2_one_bls12_377; 1 is not a mode here), the subgroup path above (a hash is cofactor-cleared) and compress_bls12_377_g1.
 * sk: n_sk x 4 u64 canonical, the 32 bytes of serialize_private_key; n_sk is 1 (one key signs every message) or n.  domain: SIG_DOMAIN for
 * signatures, POP_DOMAIN for proofs of possession, as sign_message / sign_pop pass them.  msgs / msg_off / extras / extra_off: as
 * hash_to_g1_direct_bls12_377 (extras and extra_off may be NULL).  out_sig48: n x 48 bytes as serialize_signature writes them; attempts: n
 * counters.  A message whose hash found no counter (attempts[i] == 255) gets 48 zero bytes; the call still returns 0.
 * Returns 0 (also for n = 0); 2 with nothing written: a NULL argument, n_sk not in {1, n}, a key >= r, an unknown mode. */
int sign_batch_bls12_377(const uint64_t* sk /* n_sk x 4 */, size_t n_sk /* 1 or n */, const uint8_t domain[8], const uint8_t* msgs, const uint64_t* msg_off,
                         const uint8_t* extras, const uint64_t* extra_off, size_t n, int mode, uint8_t* out_sig48 /* n x 48 */, uint8_t* attempts /* n */);
/* test and A/B hooks: the ladder's window bits c (0 = the default of DESIGN.md 6i, else 2 .. 8: a table of 2^(c-1) entries per row); the rows
 * per chunk of the per-call workspace (0 = the default, which keeps the workspace below 256 MiB; at most 2^24); and the last
 * scalar_mul_batch_* / sign_batch_* call's times in ms: [0] table build, [1] ladder, [2] normalisation, [3] the whole call (wall; for
 * sign_batch_* the hash included, whose kernel time celo_amd_hash_last_ms reports).  The setters return 2 for a value outside the range. */
int celo_amd_scalar_mul_set_window(int c);
int celo_amd_scalar_mul_set_chunk_rows(uint32_t rows);
int celo_amd_scalar_mul_last_ms(float ms[4]);

/* ---- Masked segmented point sums: the aggregated key of every seal of a batch from its signer bitmap (PublicKeyCache::aggregate,
 * crates/bls-crypto/src/bls/cache.rs:65-87; the native twin of BlsGadget::enforce_bitmap, crates/epoch-snark/src/gadgets/single_update.rs:71-117;
 * the G1 form is Signature::aggregate over a bitmap).  csrc/aggregate.h, csrc/unit_seals.hip, DESIGN.md section 6j.
 *   out_i = sum { P_j : bits_i[j] != 0 }        out_count[i] = the number of non-zero bytes of bits_i
 * Rows are those of fixed_base_mul_* / scalar_mul_batch_*: affine arkworks Montgomery limbs (12 u64 for G1, 24 for G2), a zero row with
 * inf = 1 for the identity.  P_j is ANY point of the curve (not validated, as elsewhere): duplicate keys, a key and its negative and sums
 * that are the identity are legal.  A selected row flagged in pk_inf adds nothing but still counts.
 * Two forms.  n_sets == m, per-seal sets: seal i owns rows [offsets[i], offsets[i+1]) of pk_xy / pk_inf and the bytes of `bits` at the same
 * indices (one byte per row; offsets[n_sets] rows and bytes in all).  n_sets == 1, the shared set: every seal reads rows
 * [offsets[0], offsets[1]), n of them, and bits is m x n bytes, row-major - one validator set, one bitmap per block.
 * The shared-set form computes the set's total T once per call, and a seal with strictly fewer zeros than ones is summed as T plus the
 * NEGATED keys at its zero bytes (the reference's cache: "the previous total minus the few who are absent"); a tie sums the ones.  The
 * result is the same group element, so the same row bit for bit.
 * L lanes cooperate on one sum (L a power of two, 1 .. 64): each adds the selected rows j = lane (mod L) by mixed additions, then the L
 * partials are folded pairwise through LDS by full additions.  L per call, from a = the largest number of rows a seal adds after the side
 * choice and m:  L = min(smallest power of two >= a / 4, largest power of two <= 2^16 / m), at least 1 (csrc/aggregate.h agg_pick_lanes).
 * _dev: every pointer but offsets is a DEVICE pointer (d_out_count may be NULL); the work is enqueued on hip_stream and the call returns
 * after it has drained.
 * Returns 0 (also for m = 0, which touches nothing); 2 with NOTHING written and before any use of the device: a NULL pk_xy / offsets / bits /
 * out_xy / out_inf, n_sets not in {1, m}, decreasing offsets, m > 2^24; 100: no device; 1 / 10: HIP errors. */
int aggregate_by_bitmap_bls12_377_g2(const uint64_t* pk_xy /* rows x 24 */, const uint8_t* pk_inf /* rows or NULL */, const uint32_t* offsets /* n_sets + 1 */,
                                     size_t n_sets /* 1 or m */, const uint8_t* bits, size_t m, uint64_t* out_xy /* m x 24 */, uint8_t* out_inf /* m */,
                                     uint32_t* out_count /* m, may be NULL */);
int aggregate_by_bitmap_bls12_377_g1(const uint64_t* pk_xy /* rows x 12 */, const uint8_t* pk_inf, const uint32_t* offsets, size_t n_sets, const uint8_t* bits, size_t m,
                                     uint64_t* out_xy /* m x 12 */, uint8_t* out_inf, uint32_t* out_count);
int aggregate_by_bitmap_bls12_377_g2_dev(const void* d_pk_xy, const void* d_pk_inf, const uint32_t* offsets, size_t n_sets, const void* d_bits, size_t m,
                                         void* d_out_xy, void* d_out_inf, void* d_out_count, void* hip_stream);
int aggregate_by_bitmap_bls12_377_g1_dev(const void* d_pk_xy, const void* d_pk_inf, const uint32_t* offsets, size_t n_sets, const void* d_bits, size_t m,
                                         void* d_out_xy, void* d_out_inf, void* d_out_count, void* hip_stream);
/* Aggregated seals to verdicts, chained on the device: the check a node makes once per block and the epoch prover once per transition
 * (EpochTransition { block, aggregate_signature, bitmap }, crates/epoch-snark/src/epoch_block.rs:19-30; the minimum-signers rule of
 * gadgets/single_update.rs:71-117):  apk_i = the masked sum above, count_i >= min_signers[i], e(sig_i, -g2) e(H(m_i), apk_i) == 1.
 * One call: count + sums; the m signatures (serialize_signature form, 48 B) decoded and subgroup-checked on the device; the message hashes of
 * hash_to_g1_* (hash_mode 0 direct, 2 composite, 3 composite CIP22: sign_batch's numbering; messages and extras packed as there; the hash
 * rows pass through the host, as in sign_batch); a pack kernel writes the pairs into the pairing engine's slots; the engine's products.
 * Nothing but verdicts and statuses returns.  out_status[i], the first that applies, out_ok[i] = 1 iff it is 0:
 *   0 clean and the product is one      1 count < min_signers[i], or count == 0 (a seal by nobody is not a seal)
 *   2 the signature does not decode or lies outside G1      3 the hash found no counter      4 the product is not one
 * A seal with status 1 - 3 takes no part in any product.  An apk that is the identity with count > 0 follows the pairing engine: that pair
 * contributes 1.  Precondition as for batch_verify_bls12_377: the keys are elements of G2.
 * mode 0 "each": m products of two pairs.  mode 1 "combined", contract and fallback of groth16_verify_batch_*: with the exponents r_i of
 * celo_amd_groth16_draw_exponents under `key` (8 words; NULL = 32 bytes from the OS), e(sum r_i sig_i, -g2) prod e([r_i] H(m_i), apk_i) == 1
 * over the clean seals - one m-term G1 MSM, one scalar_mul_batch on the subgroup path, one product of m + 1 pairs; if it holds every clean
 * seal is accepted, if not the call runs mode 0 and returns its verdicts.  Measured: a product of two pairs is cheap next to
 * the ladder and the MSM, so combined never won - 1.05 x the time of each at 17 280 seals, 1.23 x at 4 096, 1.45 x at 64: call mode 0 unless a
 * caller wants the single combined product for its own sake.
 * Returns 0 (also for m = 0); 2 with nothing written and before any use of the device: a NULL required pointer (pk_inf, min_signers, extras,
 * extra_off, key and out_status may be NULL), hash_mode not in {0, 2, 3}, mode not in {0, 1}, n_sets not in {1, m}, decreasing offsets, m > 2^24. */
int verify_aggregated_seals_bls12_377(const uint64_t* pk_xy, const uint8_t* pk_inf, const uint32_t* offsets, size_t n_sets, const uint8_t* bits,
                                      const uint32_t* min_signers /* m, or NULL: no threshold */, const uint8_t domain[8], const uint8_t* msgs,
                                      const uint64_t* msg_off, const uint8_t* extras, const uint64_t* extra_off, int hash_mode, const uint8_t* sig48 /* m x 48 */,
                                      const uint64_t neg_g2_xy[24], size_t m, int mode /* 0 each, 1 combined */, const uint32_t* key /* 8, or NULL */,
                                      uint8_t* out_ok /* m */, uint8_t* out_status /* m, may be NULL */);
/* test and A/B hooks: the lane width (0 = the rule above, else 1, 2, 4, .. 64) and the complement (-1 = the rule above, 0 = never, 1 = for
 * every seal of a shared-set call); anything else returns 2.  celo_amd_seals_last: the last call's record - path (-1 a bare sum; 0 each,
 * 1 combined accepted, 2 combined rejected then each), the lane width used, and times in ms: [0] count + sums + normalisation (kernel time),
 * [1] signature decoding, [2] hash kernels, [3] exponents + ladder + MSM (wall), [4] products, [5] transfers, [6] the whole call (wall),
 * [7] the count kernel alone (its share of [0]). */
int celo_amd_aggregate_set_lanes(int lanes);
int celo_amd_aggregate_set_complement(int mode);
int celo_amd_seals_last(int* path, int* lanes, float ms[8]);

/* ---- Epoch blocks to bytes, to the Groth16 public inputs of the epoch proof and to verdicts: what epoch_snark::verify
 * (crates/epoch-snark/src/api/verifier.rs:23-40) does per proof on the host, for many proofs on the device.  A light client holds a first and a
 * last EpochBlock per proof (EpochBlockFFI: index, entropies, maximum_non_signers, maximum_validators, compressed keys), not Fr elements; the
 * steps from one to the other - decode and subgroup-check every key, sum the last block's keys, bit-encode both blocks (epoch_block.rs:117-140,
 * 174-181, encoding.rs:23-47), Blake2s under "ULforout", pack the 512 bits as 376 | 136 - run here as kernels.  csrc/epoch.h,
 * csrc/unit_epoch.hip, DESIGN.md section 6k.
 *
 * celo_epoch_blocks: nb blocks.  index, round, max_non_signers, max_validators and key_off (nb + 1 offsets into keys: block i owns keys
 * [key_off[i], key_off[i+1])) are HOST arrays in every form - they size the call.  round is read by kind 2 only and may be NULL otherwise.
 * epoch_entropy / parent_entropy: nb x 16 bytes, or NULL.  A NULL array, an absent entropy and sixteen zero bytes encode to the same 128 zero
 * bits (encode_entropy_cip22), so there is no per-block flag.  keys_form 0: keys = 96-byte compressed G2 keys as in EpochBlockFFI.pubkeys,
 * decoded and subgroup-checked on the device; keys_form 1: affine rows of 24 u64 (arkworks Montgomery limbs) with keys_inf flags or NULL,
 * TRUSTED as the MSM entries trust theirs (neither the curve nor the subgroup is looked at).  An identity key is accepted: it encodes as
 * arkworks' zero() = (0, 1) and adds nothing to the sum, as Seam A `verify` treats it.  In the _dev forms keys, keys_inf and the entropies
 * are DEVICE pointers, like the outputs.
 *
 * epoch_encoded_size (host code): kind 0 first-epoch form, 176 + 755 K bits; 1 last-epoch form with the aggregated key appended,
 * 176 + 755 (K + 1); 2 inner CIP22 (the message validators sign), 256 + 755 K with 7 bytes of extra data; 3 pre-CIP22 encode_to_bytes,
 * 48 + 755 n_keys.  K = max(n_keys, max_validators); bytes = ceil(bits / 8).
 * epoch_encode_blocks_bls12_377: block i's bytes at out + out_off[i]; out_off (nb + 1, a host array, out_off[0] = 0) must be the running sum
 * of epoch_encoded_size.  Kind 2 also writes extras (nb x 7 bytes): out / out_off / extras are the msgs / msg_off / extras of hash_to_g1_* and
 * verify_aggregated_seals_bls12_377 (extra_off[i] = 7 i).  status[i]: 0 clean; 1 a key does not decode or lies outside G2 - that block's
 * bytes are zero.
 * epoch_public_inputs_bw6_761: out_inputs = m x 2 x 6 u64, canonical (what groth16_verify_batch_bw6_761 takes); out_status[i] 0, 1 a bad first
 * block, 2 a bad last block (the inputs of such a proof are not meaningful).
 * verify_epoch_proofs_bw6_761: the inputs above, then groth16_verify_batch_bw6_761_serialized on proofs (m x 288 bytes, A | B | C) under vk - the
 * inputs and block statuses are read by the verifier where they lie.  out_status[i] (may be NULL), the first that applies; out_ok[i] = 1 iff 0:
 *   0 accepted    1 / 2 as above    3 a proof point does not decode or is outside its subgroup    4 the product is not one
 * A proof with status 1 - 3 takes part in no product and no combination, like a malformed serialized proof of the batch verifier.  mode, key,
 * limits and the precondition handling are groth16_verify_batch_bw6_761_serialized's; celo_amd_groth16_verify_last describes the verifier's part.
 *
 * Returns 0 (also for nb / m = 0); 2 with NOTHING written and before any use of the device: a NULL required pointer, decreasing offsets, out_off
 * not the sizes' running sum, nb or m above 2^24, kind or keys_form out of range, mode not in {0, 1}, a block with n_keys or max_validators above
 * 65 536 (a limit the reference does not have: no single maximum_validators sizes a buffer here), more than 2^31 - 1 keys, vk not a live BW6-761
 * handle with exactly two inputs; 100: no device; 1 / 10: HIP errors.
 * celo_amd_epoch_last: the last call's times in ms: [0] key decoding, [1] key sums + normalisation, [2] records + pack, [3] Blake2s + input
 * packing, [4] transfers, [5] the verifier (wall), [6] the whole call (wall), [7] unused. */
typedef struct celo_epoch_blocks {
  const uint16_t* index;           /* nb */
  const uint8_t* round;            /* nb, or NULL unless kind 2 */
  const uint32_t* max_non_signers; /* nb */
  const uint32_t* max_validators;  /* nb */
  const uint8_t* epoch_entropy;    /* nb x 16, or NULL */
  const uint8_t* parent_entropy;   /* nb x 16, or NULL */
  const void* keys;                /* key_off[nb] x 96 bytes (keys_form 0) or x 24 u64 (keys_form 1) */
  const uint8_t* keys_inf;         /* keys_form 1: key_off[nb] flags, or NULL */
  const uint32_t* key_off;         /* nb + 1 */
  int keys_form;
} celo_epoch_blocks;
int epoch_encoded_size(int kind, uint64_t n_keys, uint64_t max_validators, uint64_t* bytes);
int epoch_encode_blocks_bls12_377(const celo_epoch_blocks* blocks, size_t nb, int kind, const uint64_t* out_off /* nb + 1 */, uint8_t* out, uint8_t* extras /* nb x 7, kind 2 */,
                                  uint8_t* status /* nb */);
int epoch_encode_blocks_bls12_377_dev(const celo_epoch_blocks* blocks, size_t nb, int kind, const uint64_t* out_off, void* d_out, void* d_extras, void* d_status,
                                      void* hip_stream);
int epoch_public_inputs_bw6_761(const celo_epoch_blocks* first, const celo_epoch_blocks* last, size_t m, uint64_t* out_inputs /* m x 12 */, uint8_t* out_status /* m */);
int epoch_public_inputs_bw6_761_dev(const celo_epoch_blocks* first, const celo_epoch_blocks* last, size_t m, void* d_out_inputs, void* d_out_status, void* hip_stream);
int verify_epoch_proofs_bw6_761(const void* vk, const uint8_t* proofs /* m x 288 */, const celo_epoch_blocks* first, const celo_epoch_blocks* last, size_t m,
                                int mode /* 0 each, 1 combined */, const uint32_t* key /* 8, or NULL */, uint8_t* out_ok /* m */, uint8_t* out_status /* m, may be NULL */);
int celo_amd_epoch_last(float ms[8]);

/* ---- chains of epoch transitions to verdicts: what epoch_snark::prove holds (crates/epoch-snark/src/api/prover.rs:22-82: an initial EpochBlock
 * and a list of EpochTransition { block, aggregate_signature, bitmap }), checked against what the circuit ValidatorSetUpdate enforces
 * (gadgets/epochs.rs:97-283, single_update.rs:79-135, epoch_data.rs:223-233, bls-gadgets/src/bls.rs:138-191) BEFORE a proof is made -
 * create_proof_no_zk does not check satisfaction, and a full node runs the same check over every epoch header it syncs.  One call: keys
 * decoded once, blocks encoded in the inner CIP22 form, CRH, CIP22 tail, masked key sums, signatures and products all stay on the device.
 *
 * Layout: everything is indexed by block.  Chain c owns blocks [chain_off[c], chain_off[c+1]); the first is its initial epoch, every other
 * block b is a transition with predecessor p = b - 1.  bits[key_off[p] + j] != 0: key j of block p signed block p + 1 (any non-zero byte; the
 * bytes under the last block of a chain are ignored).  sig48[b]: the aggregate signature over block b, compressed (rows of initial blocks are
 * ignored).  blocks: celo_epoch_blocks as above, either keys_form, `round` required.  domain: the 8 bytes of the hasher's personalisation;
 * neg_g2_xy: -g2 as for verify_aggregated_seals_bls12_377.
 *
 * out_status[b], the first that applies (out_ok[b] = 1 iff it is 0; an initial block can only get 0 or 1):
 *    0  accepted
 *    1  a key of block b does not decode or lies outside G2 (epoch_encode_blocks status 1)
 *    2  block p has status 1: the signing set is unknown
 *    3  index[b] != index[p] + 1, compared as integers, no wrap; a transition with index 0 always lands here (the circuit's dummy padding is
 *       the prover's business, not an input)                                                     epoch_data.rs:223-233
 *    4  n_keys(b) != n_keys(p): the circuit's num_validators is fixed                            single_update.rs:92
 *    5  the chain's INITIAL block has a non-zero epoch_entropy and parent_entropy[b] != epoch_entropy[p] (16 bytes; a NULL array is all zero)
 *                                                                                                epochs.rs:193, single_update.rs:104-107
 *    6  signers < n_keys(p) - max_non_signers[p] (saturating at 0), or no signer at all          bls.rs:187
 *    7  a SELECTED key of block p equals the padding key, the G2 generator (an unselected one is legal)    bls.rs:147-148, epoch_block.rs:94-96
 *    8  the signature does not decode or lies outside G1
 *    9  the hash found no counter
 *   10  the product is not one
 *
 * mode 0, "is every seal genuine": one two-pair product per clean transition, e(sig_b, -g2) e(H_b, apk_b); out_chain_ok[c] is the AND over
 * the chain's blocks.
 * mode 1, "will the proof verify": the circuit's own statement (epochs.rs verify_signature, unweighted aggregation).  Every chain whose
 * blocks are all free of statuses 1 to 9 is ONE product, e(sum_b sig_b, -g2) prod_b e(H_b, apk_b), all chains in one ragged call of the
 * pairing engine.  A chain whose product holds has status 0 throughout and out_chain_ok[c] = 1; one whose product fails has its transitions
 * run as in mode 0 to place status 10.  A chain with a status in 1 to 9 is not multiplied: its clean blocks are checked as in mode 0.
 * THE CONSEQUENCE: mode 1 accepts a chain whose signatures are individually wrong but sum correctly (sig_a + D and sig_b - D), because the
 * circuit does too.  It does not say that every seal is genuine; mode 0 does.
 *
 * Optional outputs (NULL to skip), what the prover takes away: out_crh[b] the 48-byte CRH of block b's inner encoding (the message_bits of
 * the hash helper, prover.rs:92-106); out_attempts[b] the hash counter (the hash-to-group gadget's witness); out_asig_xy[c] / out_asig_inf[c]
 * the sum of the chain's signatures that decoded into G1 (prover.rs:62), an affine row of 12 u64 and an identity flag (the row is zero when
 * the flag is set).  Rows of initial blocks are zero.
 *
 * Returns 0, also for nb == 0; 2, with nothing written and before any use of the device, for a NULL required pointer, chain_off not
 * increasing from 0 to nb (an empty chain included), mode not in {0, 1}, the refusals of epoch_encode_blocks (key counts, nb > 2^24), or a
 * block whose inner encoding + 8 bytes exceeds the Pedersen table of 93 * 560 * 3 bits (max(n_keys, max_validators) <= 206 fits; the reference
 * panics); 100 / 1 / 10 as elsewhere.  Calls from several threads are serialised.  Not covered by tests: more than one device; a hash that
 * exhausts its counters (no such input is known). */
int verify_epoch_transitions_bls12_377(const celo_epoch_blocks* blocks, size_t nb, const uint32_t* chain_off /* n_chains + 1 */, size_t n_chains,
                                       const uint8_t* bits /* key_off[nb] bytes */, const uint8_t* sig48 /* nb x 48 */, const uint8_t domain[8],
                                       const uint64_t neg_g2_xy[24], int mode /* 0 each, 1 chain product */, uint8_t* out_ok /* nb */,
                                       uint8_t* out_status /* nb or NULL */, uint8_t* out_chain_ok /* n_chains or NULL */, uint8_t* out_crh /* nb x 48 or NULL */,
                                       uint8_t* out_attempts /* nb or NULL */, uint64_t* out_asig_xy /* n_chains x 12 or NULL */,
                                       uint8_t* out_asig_inf /* n_chains or NULL */);
/* the last verify_epoch_transitions call: *path 0 = each, 1 = chain products and every one held, 2 = at least one chain fell back to its
 * transitions (-1 before any call); ms in the slots of celo_amd_epoch_last: [0] key decoding, [1] masked sums (keys, then signatures), [2]
 * packing, [3] CRH + CIP22 tail, [4] transfers, [5] the products, [6] wall time of the call, [7] signature decoding and the status kernel */
int celo_amd_transitions_last(int* path, float ms[8]);

/* ---- R1CS matrices on the device: the step of ark-groth16 0.1 between cs.to_matrices() and the entry points above - the constraint evaluation
 * of R1CStoQAP::witness_map (prover) and R1CStoQAP::instance_map_with_evaluation (setup).  Synthesis (running the gadgets) stays with the caller
 * for every circuit but HashToBits (hash_to_bits_* below); its result is data: three sparse matrices of n_constraints rows and the full assignment.
 *
 * One matrix = CSR: row_ptr (n_constraints + 1 offsets, row_ptr[0] = 0, row_ptr[n_constraints] = nnz), col (nnz variable indices: the instance
 * variables first, index 0 the constant one, then the witness), val (nnz x 6 | 4 u64, arkworks Montgomery Fr), nnz (the length of col and val).
 * Rows may be empty, repeat a column or hold a zero coefficient.
 *
 * groth16_r1cs_load_*: validates on the host, copies the matrices to the device and builds their transposes and the work lists of both
 * products, once.  Returns 0; 2: n_inputs == 0, n_inputs > n_vars, n_vars, n_constraints or an nnz >= 2^32, a NULL array; 34: a matrix is
 * malformed - *first_bad (may be NULL) = matrix index (0 a, 1 b, 2 c) << 60 | the row whose end lies before its start (row 0: row_ptr[0] != 0,
 * row n_constraints: row_ptr[n_constraints] != nnz), or | the entry whose col >= n_vars or whose val >= the modulus; 10: device allocation
 * failure.  On any failure everything is freed and *out_r1cs is NULL.  A handle is bound to its device (101 from another), is read-only after
 * the load and may be used from several threads; groth16_r1cs_free releases it.
 * groth16_r1cs_info: out = curve (0 BW6-761, 1 BLS12-377), n_constraints, n_vars, n_inputs, nnz of a, b, c, device bytes held.
 *
 * groth16_r1cs_rows: the witness map's inputs from the assignment z (n_vars x 6 | 4 u64 Montgomery, below the modulus, z[0] = 1):
 * out_a[j] = sum_k A[j][k] z_k for j < n_constraints, likewise out_b, out_c; out_a[n_constraints + i] = z_i for i < n_inputs (the
 * input-consistency rows); every other row up to 2^log_n zero.  2: 2^log_n < n_constraints + n_inputs or log_n > 28.  _dev: z and the outputs
 * are device pointers, the work runs on hip_stream and is complete on return.
 * groth16_r1cs_check: (A z)_j (B z)_j == (C z)_j for every constraint; *first_unsatisfied = the smallest failing j, or -1.
 *
 * groth16_r1cs_qap_at_tau: the four inputs of groth16_setup_*.  L_j = Z(tau) / n * omega^j / (tau - omega^j) over the n = 2^log_n domain points
 * (omega = the domain's group_gen, from the caller; for tau = omega^k: L_j = [j == k], Z(tau) = 0); out_a[i] = sum_j A[j][i] L_j
 * (+ L_(n_constraints + i) for i < n_inputs), out_b, out_c without the extra term (n_vars x 6 | 4 u64 each), out_zt = tau^n - 1 (one element, a
 * HOST pointer in both forms).  _dev: out_a / out_b / out_c are device pointers. */
int groth16_r1cs_load_bw6_761(size_t n_constraints, size_t n_vars, size_t n_inputs, const uint64_t* a_row_ptr, const uint32_t* a_col, const uint64_t* a_val, size_t a_nnz,
                              const uint64_t* b_row_ptr, const uint32_t* b_col, const uint64_t* b_val, size_t b_nnz, const uint64_t* c_row_ptr, const uint32_t* c_col,
                              const uint64_t* c_val, size_t c_nnz, void** out_r1cs, uint64_t* first_bad);
int groth16_r1cs_load_bls12_377(size_t n_constraints, size_t n_vars, size_t n_inputs, const uint64_t* a_row_ptr, const uint32_t* a_col, const uint64_t* a_val, size_t a_nnz,
                                const uint64_t* b_row_ptr, const uint32_t* b_col, const uint64_t* b_val, size_t b_nnz, const uint64_t* c_row_ptr, const uint32_t* c_col,
                                const uint64_t* c_val, size_t c_nnz, void** out_r1cs, uint64_t* first_bad);
int groth16_r1cs_info(const void* r1cs, uint64_t out[8]);
int groth16_r1cs_free(void* r1cs);
int groth16_r1cs_rows(const void* r1cs, const uint64_t* z, unsigned log_n, uint64_t* out_a, uint64_t* out_b, uint64_t* out_c /* 2^log_n x 6 | 4 each */);
int groth16_r1cs_rows_dev(const void* r1cs, const uint64_t* d_z, unsigned log_n, uint64_t* d_out_a, uint64_t* d_out_b, uint64_t* d_out_c, void* hip_stream);
int groth16_r1cs_check(const void* r1cs, const uint64_t* z, int64_t* first_unsatisfied);
int groth16_r1cs_qap_at_tau(const void* r1cs, unsigned log_n, const uint64_t* omega, const uint64_t* tau, uint64_t* out_a, uint64_t* out_b, uint64_t* out_c,
                            uint64_t* out_zt);
int groth16_r1cs_qap_at_tau_dev(const void* r1cs, unsigned log_n, const uint64_t* omega, const uint64_t* tau, uint64_t* d_out_a, uint64_t* d_out_b, uint64_t* d_out_c,
                                uint64_t* out_zt, void* hip_stream);
/* matrices + assignment -> proof: z goes to the device once; groth16_r1cs_rows_dev, the witness map (canonical h) and the canonical assignment
 * z[1..] are made there, and the four fixed-base MSMs of groth16_prove_with_key read them where they lie.  Domain constants as for
 * groth16_witness_map_*.  Same results, identity-row rule and error codes as the piecewise calls; 2 also for a key and a circuit of different
 * curves, 101 for a key or circuit of another device. */
int groth16_prove_r1cs_with_key(const void* key, const void* r1cs, const uint64_t* z, unsigned log_n, const uint64_t* omega, const uint64_t* omega_inv,
                                const uint64_t* coset, const uint64_t* coset_inv, const uint64_t* size_inv, const uint64_t* vanishing_inv, uint64_t* out_a,
                                uint64_t* out_b, uint64_t* out_c);
/* matrices + toxic waste -> parameters: groth16_r1cs_qap_at_tau_dev, then groth16_setup_* on the vectors where they lie, with
 * n_h = 2^log_n - 1.  Outputs and codes as groth16_setup_*; 2 also for a circuit of the other curve or 2^log_n < n_constraints + n_inputs. */
int groth16_setup_r1cs_bw6_761(const void* r1cs, unsigned log_n, const uint64_t omega[6], const uint64_t tau[6], const uint64_t toxic[24], const uint64_t g1_xy[24],
                               const uint64_t g2_xy[24], int window_bits, uint64_t* out_vk, uint64_t* out_rows, void** out_key);
int groth16_setup_r1cs_bls12_377(const void* r1cs, unsigned log_n, const uint64_t omega[4], const uint64_t tau[4], const uint64_t toxic[16], const uint64_t g1_xy[12],
                                 const uint64_t g2_xy[24], int window_bits, uint64_t* out_vk, uint64_t* out_rows, void** out_key);
/* the last calls' times in ms: [0] load (host wall: validation, transposition, copies), [1] rows kernels, [2] Lagrange kernel, [3] columns kernels,
 * [4] groth16_prove_r1cs_with_key wall, [5] groth16_setup_r1cs_* wall, [6..7] unused */
int celo_amd_r1cs_last_timings(float ms[8]);
/* groth16_prove_r1cs_with_key with z as a DEVICE pointer (n_vars x 6 | 4 u64, complete before the call; it is read, not written): the copy of z
 * to the device is skipped and everything else is the same: the same three points (their Jacobian representatives are not fixed from call to call in
 * either entry: the MSMs' summation order is not), the same bytes from groth16_serialize_proof_*. */
int groth16_prove_r1cs_with_key_dev(const void* key, const void* r1cs, const uint64_t* d_z, unsigned log_n, const uint64_t* omega, const uint64_t* omega_inv,
                                    const uint64_t* coset, const uint64_t* coset_inv, const uint64_t* size_inv, const uint64_t* vanishing_inv, uint64_t* out_a,
                                    uint64_t* out_b, uint64_t* out_c);

/* ---- The one circuit the library synthesizes itself: HashToBits, the circuit of the hash-helper proof over BLS12-377
 * (crates/epoch-snark/src/gadgets/hash_to_bits.rs; generate_hash_helper, api/prover.rs:85-118).  For n_epochs messages of 384 bits it states
 * that the 512 XOF bits of every message are Blake2Xs (two single-block Blake2s compressions under SIG_DOMAIN, DirectHasher::xof(.., 64)) of
 * its bits.  The instance vector is the reference's:  [1] ++ pack(all message bits) ++ pack(all XOF bits), pack = 252-bit (Fr::CAPACITY)
 * chunks running across epoch borders, the first bit of a chunk the most significant, a short last chunk:
 * n_inputs = 1 + ceil(384 n_epochs / 252) + ceil(512 n_epochs / 252).
 * The LAYOUT is not the reference's: the order of its variables and constraints comes from the arkworks gadgets and is not reproduced, so keys
 * made for this system and the reference's ceremony keys do not fit each other.  What holds is the same relation over the same instance vector
 * (the row kinds, the counts and the soundness argument).
 *
 * rows48: n_epochs rows of 48 bytes, e.g. out_crh of verify_epoch_transitions_bls12_377 as it lies.  bit_order 0: message bit j = bit j % 8 of
 * byte j / 8 of the row (bytes_le_to_bits_le, the reference's own test); 1: the 384-bit reversal of that (bytes_le_to_bits_be(row, 384), what
 * prover.rs:101 feeds from the CRH bytes: the order for out_crh rows).
 *
 * hash_to_bits_r1cs_size_*: host only.  out = n_constraints, n_vars, n_inputs, nnz of a, b, c, the smallest log_n (2^log_n >= n_constraints +
 * n_inputs), the variables per epoch (epoch e's witness lies at n_inputs + e * that).  2: n_epochs == 0, out NULL, or the circuit exceeds the
 * R1CS limits (n_vars or an nnz >= 2^32, log_n > 28).
 * hash_to_bits_r1cs_*: host only.  Writes the three matrices into caller-owned arrays of those sizes (row_ptr: n_constraints + 1, col: nnz,
 * val: 4 nnz u64) - with the nnz, the arguments of groth16_r1cs_load_bls12_377.  2 as above or for a NULL array.
 * hash_to_bits_r1cs_load_*: both in one; *out_r1cs is an ordinary R1CS handle of curve 1 (groth16_r1cs_free), codes of groth16_r1cs_load_*.
 * hash_to_bits_assignment_*: the full assignment z (n_vars x 4 u64 Montgomery, z[0] = 1) of the messages.  _dev: rows48 and z are device
 * pointers, the work runs on hip_stream and is complete on return.  celo_amd_hash_to_bits_assignment_host: the same on the host, from the
 * same templates (no device needed).  2: a NULL pointer, bit_order not 0 / 1, n_epochs refused by the size query.
 * hash_to_bits_public_inputs_*: the verifier's side, for n_proofs proofs of n_epochs epochs each (proof p takes rows [p n_epochs,
 * (p + 1) n_epochs)): out = n_proofs x (n_inputs - 1) x 4 u64 CANONICAL, the constant left out - the inputs of
 * groth16_verify_batch_bls12_377.  2 as above, or n_proofs == 0 or n_proofs * n_epochs > 2^24.
 * groth16_hash_helper_prove_*: generate_hash_helper in one call.  The rows go to the device, the assignment is made there, the proof is
 * groth16_prove_r1cs_with_key's from the device-resident z (A, B, C Jacobian; create_proof_no_zk, no randomisation), and out_inputs receives the
 * n_inputs - 1 canonical instance rows.  key / r1cs: a BLS12-377 key and the handle of hash_to_bits_r1cs_load_* for the same n_epochs and
 * log_n (2: another curve, a circuit of another size, a key whose queries are not n_vars, n_vars, n_vars - n_inputs and 2^log_n - 1 rows long;
 * 101: another device).  Domain constants as for groth16_prove_r1cs_with_key.
 * celo_amd_hash_helper_last: the last such call in ms: [0] trace, [1] expand, [2] pack kernels, [3] the proof (wall), [4] the call (wall); a
 * hash_to_bits_assignment_* call leaves its three kernel times in [0..2] and zeroes the rest.
 *
 * groth16_hash_helper_verify_*: the verifier's side of generate_hash_helper in one call, for n_proofs serialized proofs (192 B each; proof p
 * over rows [p n_epochs, (p + 1) n_epochs)).  The rows go to the device, the canonical inputs are written there and the verifier of
 * groth16_verify_batch_bls12_377_serialized reads them where they lie; mode, key and out_ok (n_proofs verdicts) are that entry's.  vk: a
 * BLS12-377 handle of n_inputs - 1 public inputs.  2, before any device use: a NULL pointer (key may be NULL), bit_order or mode not 0 / 1,
 * n_proofs or n_epochs refused by hash_to_bits_public_inputs_*, a handle that is not a live BLS12-377 one or whose input count is not
 * n_inputs(n_epochs) - 1.  Otherwise the verifier's codes.
 *
 * Limit: a key from groth16_vk_load_bls12_377[_serialized] takes at most 64 public inputs (code 36): helper proofs of at most 17 epochs (61
 * inputs; 18 epochs have 65).  A key from groth16_vk_load_bls12_377_wide[_serialized] takes 1024: up to 287 epochs, the production size of
 * 143 (509 inputs) among them.  Everything else here works at any n_epochs within the R1CS limits; 143 epochs make a domain of 2^23. */
int hash_to_bits_r1cs_size_bls12_377(size_t n_epochs, uint64_t out[8]);
int hash_to_bits_r1cs_bls12_377(size_t n_epochs, uint64_t* a_row_ptr, uint32_t* a_col, uint64_t* a_val, uint64_t* b_row_ptr, uint32_t* b_col, uint64_t* b_val,
                                uint64_t* c_row_ptr, uint32_t* c_col, uint64_t* c_val);
int hash_to_bits_r1cs_load_bls12_377(size_t n_epochs, void** out_r1cs);
int hash_to_bits_assignment_bls12_377(const uint8_t* rows48, size_t n_epochs, int bit_order, uint64_t* z);
int hash_to_bits_assignment_bls12_377_dev(const uint8_t* d_rows48, size_t n_epochs, int bit_order, uint64_t* d_z, void* hip_stream);
int celo_amd_hash_to_bits_assignment_host(const uint8_t* rows48, size_t n_epochs, int bit_order, uint64_t* z);
int hash_to_bits_public_inputs_bls12_377(const uint8_t* rows48, size_t n_proofs, size_t n_epochs, int bit_order, uint64_t* out);
int hash_to_bits_public_inputs_bls12_377_dev(const uint8_t* d_rows48, size_t n_proofs, size_t n_epochs, int bit_order, uint64_t* d_out, void* hip_stream);
int groth16_hash_helper_prove_bls12_377(const void* key, const void* r1cs, const uint8_t* rows48, size_t n_epochs, int bit_order, unsigned log_n, const uint64_t* omega,
                                        const uint64_t* omega_inv, const uint64_t* coset, const uint64_t* coset_inv, const uint64_t* size_inv,
                                        const uint64_t* vanishing_inv, uint64_t* out_a, uint64_t* out_b, uint64_t* out_c, uint64_t* out_inputs);
int celo_amd_hash_helper_last(float ms[8]);
int groth16_hash_helper_verify_bls12_377(const void* vk, const uint8_t* rows48 /* n_proofs x n_epochs x 48 */, size_t n_proofs, size_t n_epochs, int bit_order,
                                         const uint8_t* proofs /* n_proofs x 192 */, int mode, const uint32_t* key /* 8, or NULL */, uint8_t* out_ok /* n_proofs */);

#ifdef __cplusplus
}
#endif
#endif
