// Translation unit: the Groth16 prover's device work - what ark_groth16::create_proof_no_zk does after
// R1CS synthesis, for BOTH proofs of an epoch: the epoch proof over BW6-761 (crates/epoch-snark/src/api/prover.rs:78 ->
// generate_epoch_proof) and the hash-helper proof over BLS12-377 (prover.rs:83-118, create_proof_no_zk::<BLSCurve, _> at :112):
//   1. witness map (ark-groth16 r1cs_to_qap.rs R1CStoQAP::witness_map): the QAP evaluations a, b, c over the domain
//        ifft(a), ifft(b), ifft(c); coset_fft(a), coset_fft(b), coset_fft(c); ab = (a o b - c) / Z(coset); coset_ifft(ab) = h
//      seven radix-2 transforms over the curve's scalar field (ntt.h: Fr(BW6-761) = 377 bits, Fr(BLS12-377) = 253 bits) and one
//      pointwise kernel; Z is constant on the coset: g^n - 1.
//   2. the proof (create_proof with r = s = 0):
//        A = a_query[0] + MSM(a_query[1..], assignment) + alpha_g1
//        B = b_g2_query[0] + MSM(b_g2_query[1..], assignment) + beta_g2
//        C = MSM(l_query, aux_assignment) + MSM(h_query, h)
//      the four MSMs run concurrently on four engines (msm.h); the handful of point additions around them on the host.
// R1CS synthesis (running the gadgets) is the circuit's business and stays with the caller (but for HashToBits: unit_hashbits.hip).  Evaluating the constraint matrices on the
// assignment is unit_r1cs.hip: groth16_prove_r1cs below starts from matrices + assignment, the entry points above it from a, b, c.
#include <hip/hip_runtime.h>
#include <cstdio>
#include "fp.h"
#include "runtime.h"
#include "units.h"
#include <algorithm>
#include <thread>
#include <vector>
#include <cstring>

namespace celo {
// a[i] <- (a[i] b[i] - c[i]) z   (arkworks Montgomery limbs in and out; optionally the canonical integer: Fr::into_repr())
template <class FR>
__global__ void __launch_bounds__(256) k_qap_combine(uint64_t* __restrict__ a, const uint64_t* __restrict__ b, const uint64_t* __restrict__ c, uint32_t n,
                                                     const uint32_t* __restrict__ z_dev) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int A = FR::ARK64;
  const FR x = FR::from_ark(a + (size_t)i * A), y = FR::from_ark(b + (size_t)i * A), w = FR::from_ark(c + (size_t)i * A);
  const FR z = FR::load(z_dev);
  const FR t = FR::norm(FR::template sub<4, 1>(FR::mul(x, y), w));
  FR::mul(t, z).to_ark(a + (size_t)i * A);
}
template <class FR>
__global__ void __launch_bounds__(256) k_to_canonical(uint64_t* __restrict__ a, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  FR::from_ark(a + (size_t)i * FR::ARK64).to_canonical(a + (size_t)i * FR::ARK64);
}

// a, b, c: host or device pointers (runtime.h, the call frame; on the caller's stream in both forms).  a is overwritten with h; as device
// pointers b and c are overwritten with intermediate values.
template <class FR>
int witness_map_run(uint64_t* a, uint64_t* b, uint64_t* c, unsigned log_n, const uint64_t* omega, const uint64_t* omega_inv, const uint64_t* coset,
                    const uint64_t* coset_inv, const uint64_t* n_inv, const uint64_t* z_inv, int out_canonical, int dev, void* stream_) {
  if (int rc0 = api_enter()) return rc0;
  if (!a || !b || !c || !omega || !omega_inv || !coset || !coset_inv || !n_inv || !z_inv || log_n > 28) return 2;
  const size_t n = size_t(1) << log_n, bytes = n * FR::ARK64 * 8;
  CallScope cs((hipStream_t)stream_);
  const hipStream_t stream = cs.stream();
  uint64_t *da, *db, *dc;
  uint32_t zw[FR::WORDS];
  {
    FR v = FR::wred(FR::from_ark(z_inv));
    memset(zw, 0, sizeof zw);
    v.store(zw);
  }
  HIP_TRY(cs.inout(&da, a, bytes, dev), 10);
  HIP_TRY(cs.in(&db, b, bytes, dev), 10);
  HIP_TRY(cs.in(&dc, c, bytes, dev), 10);
  uint32_t* d_z;
  HIP_TRY(cs.in(&d_z, zw, sizeof zw, 0), 10);
  // an NTT engine keeps the twiddle table of its last (omega, n) and the pool hands the same engine back to a serial caller: the
  // table is rebuilt three times per witness map (inverse, forward, inverse: ~20 us each at 2^20), not seven
  for (uint64_t* p : {da, db, dc}) if (int rc = ntt_run<FR>(p, log_n, omega_inv, nullptr, 0, n_inv, 1, stream)) return rc;        // ifft
  for (uint64_t* p : {da, db, dc}) if (int rc = ntt_run<FR>(p, log_n, omega, coset, 0, nullptr, 1, stream)) return rc;             // coset_fft
  hipLaunchKernelGGL((k_qap_combine<FR>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, da, db, dc, (uint32_t)n, d_z);
  if (int rc = ntt_run<FR>(da, log_n, omega_inv, coset_inv, 1, n_inv, 1, stream)) return rc;                                          // coset_ifft
  if (out_canonical) hipLaunchKernelGGL((k_to_canonical<FR>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, da, (uint32_t)n);
  HIP_TRY(hipGetLastError(), 10);
  HIP_TRY(cs.copy_back(), 10);
  HIP_TRY(hipStreamSynchronize(stream), 10);
  return 0;
}

template int witness_map_run<Fr761>(uint64_t*, uint64_t*, uint64_t*, unsigned, const uint64_t*, const uint64_t*, const uint64_t*, const uint64_t*, const uint64_t*,
                                    const uint64_t*, int, int, void*);
template int witness_map_run<Fr377>(uint64_t*, uint64_t*, uint64_t*, unsigned, const uint64_t*, const uint64_t*, const uint64_t*, const uint64_t*, const uint64_t*,
                                    const uint64_t*, int, int, void*);

// ---- the proof composition, once for both curves.  A curve: its two MSM groups, its scalar field and the sizes in u64 - a coordinate of a G1 /
// G2 point (affine rows are 2, Jacobian points 3 coordinates) and a scalar.  Fq: the field whose 1 is a coordinate's "one" (Fq2: (1, 0)).
// HOST_FLAGS (MsmApi::host): 2 = a query row (0, 1) is arkworks' identity (msm.h k_flag_ark_zero); 1 = a proving key's BLS12-377 queries are
// elements of G1 / G2 (the GLV split applies, msm.h k_glv_expand).
struct Bw6 {          // the epoch proof: every point has 12-u64 coordinates
  typedef G_761 G1; typedef G_761 G2; typedef Fr761 FR; typedef Fq761d Fq;
  static constexpr int CURVE = 0, Q1 = 12, Q2 = 12, S = 6, HOST_FLAGS = 2;
};
// the hash-helper proof (prover.rs:112): A, C and the a / h / l queries live in G1, B and the b_g2 query in G2.  (create_proof also accumulates B
// in G1 - g_b_g1 - for the r B term of C; with r = s = 0 that term vanishes whatever B's G1 image is, so it is not computed.)
struct Bls12 {
  typedef G1_377 G1; typedef G2_377 G2; typedef Fr377 FR; typedef Fq377d Fq;
  static constexpr int CURVE = 1, Q1 = 6, Q2 = 12, S = 4, HOST_FLAGS = 3;
};

// The arkworks limbs of a coordinate's 1 (a Montgomery product to make: built once per key load or proof, not per row), and what is decided by it.
// arkworks' GroupAffine::zero() handed over as coordinates is x = 0, y = 1 (never an element of a prime-order group here: msm.h)
template <class Fq, int Q> struct ArkOne {
  uint64_t v[Q];
  ArkOne() { memset(v, 0, sizeof v); Fq::one().to_ark(v); }
  bool is_zero(const uint64_t* xy) const {
    uint64_t o = 0;
    for (int k = 0; k < Q; k++) o |= xy[k] | (xy[Q + k] ^ v[k]);
    return o == 0;
  }
  // affine (x, y) -> Jacobian (x, y, 1), or Z = 0 for the identity encoding (query[0] or a key element may be given so)
  void as_jac(const uint64_t* xy, uint64_t* j) const {
    memcpy(j, xy, 2 * Q * 8);
    memset(j + 2 * Q, 0, Q * 8);
    if (!is_zero(xy)) memcpy(j + 2 * Q, v, Q * 8);
  }
};
// The four MSMs of a proof, each a callable (scalars, n, out Jacobian) -> rc that holds its own bases: the variable-base MSM over a caller's
// query, or the fixed-base MSM over a loaded key's table.
template <class G> static auto host_msm(const uint64_t* bases, int flags) {
  return [=](const uint64_t* sc, size_t n, uint64_t* out) { return MsmApi<G>::host(bases, nullptr, sc, n, flags, out); };
}
// resident = 0: the scalars are host pointers; 1: device pointers whose producing stream has been synchronised (the four engine threads read
// them on their own streams).  A query without rows has no table: the identity
template <class G, class Fq, int Q> static auto fixed_msm(const FixedTable* t, int resident) {
  return [=](const uint64_t* sc, size_t n, uint64_t* out) {
    if (t && n) return MsmApi<G>::fixed_run(t, sc, n, resident, out, nullptr);
    memset(out, 0, 3 * Q * 8);
    Fq::one().to_ark(out + Q);
    return 0;
  };
}
// what a proof takes from its key beside the MSM bases: the rows of the four queries (a and b counted WITH their row 0, which is a0 / b0 and
// not among the MSM's bases), row 0 of a and b and the two key elements (affine arkworks limbs)
struct KeySide {
  size_t na, nb, nl, nh;
  const uint64_t *a0, *b0, *alpha_g1, *beta_g2;
};
// assignment: n_assign canonical scalars (public inputs without the leading one, then the witness); aux = its last n_aux entries; h: n_h canonical scalars
// (the witness map's output).  Results: Jacobian.  The four MSMs run concurrently on four engines, three threads and the caller's.
template <class C, class MsmA, class MsmB, class MsmL, class MsmH>
static int compose(MsmA msm_a, MsmB msm_b, MsmL msm_l, MsmH msm_h, const KeySide& key, const uint64_t* assignment, size_t n_assign, size_t n_aux, const uint64_t* h,
                   size_t n_h, uint64_t* out_a, uint64_t* out_b, uint64_t* out_c) {
  typedef typename C::Fq Fq;
  constexpr int Q1 = C::Q1, Q2 = C::Q2, J1 = 3 * Q1, J2 = 3 * Q2;
  // VariableBaseMSM::multi_scalar_mul zips bases with scalars: the shorter side decides (ark-ec msm/variable_base.rs)
  const size_t ka = std::min(key.na - 1, n_assign), kb = std::min(key.nb - 1, n_assign), kl = std::min(key.nl, n_aux), kh = std::min(key.nh, n_h);
  const uint64_t* aux = assignment + (n_assign - n_aux) * C::S;
  // calculate_coeff(initial = 0, query, vk_param, assignment): A = a0 + MSM_a + alpha, B = b0 + MSM_b + beta;  C = MSM_l + MSM_h
  uint64_t ta[3 * J1], tb[3 * J2], tc[2 * J1];
  int rcs[4] = {0, 0, 0, 0};
  const int dev = api_device();
  auto run = [&](int i, auto& msm, const uint64_t* sc, size_t n, uint64_t* out) {
    rcs[i] = api_bind_thread(dev);
    if (!rcs[i]) rcs[i] = msm(sc, n, out);
  };
  {
    std::thread t0([&] { run(0, msm_a, assignment, ka, ta + J1); }), t1([&] { run(1, msm_b, assignment, kb, tb + J2); }), t2([&] { run(2, msm_l, aux, kl, tc); });
    run(3, msm_h, h, kh, tc + J1);
    t0.join(); t1.join(); t2.join();
  }
  for (int r : rcs) if (r) return r;
  const ArkOne<Fq, Q1> one1;
  const ArkOne<Fq, Q2> one2;
  one1.as_jac(key.a0, ta); one1.as_jac(key.alpha_g1, ta + 2 * J1);
  if (int rc = MsmAuxApi<typename C::G1>::sum_jac(ta, 3, out_a)) return rc;
  one2.as_jac(key.b0, tb); one2.as_jac(key.beta_g2, tb + 2 * J2);
  if (int rc = MsmAuxApi<typename C::G2>::sum_jac(tb, 3, out_b)) return rc;
  return MsmAuxApi<typename C::G1>::sum_jac(tc, 2, out_c);
}

// all pointers HOST.  Queries: affine points, arkworks layout
template <class C>
static int prove_host(const uint64_t* a_query, size_t na, const uint64_t* b_g2_query, size_t nb, const uint64_t* h_query, size_t nh, const uint64_t* l_query, size_t nl,
                      const uint64_t* alpha_g1, const uint64_t* beta_g2, const uint64_t* assignment, size_t n_assign, size_t n_aux, const uint64_t* h, size_t n_h,
                      uint64_t* out_a, uint64_t* out_b, uint64_t* out_c) {
  if (int rc0 = api_enter()) return rc0;
  if (!a_query || !b_g2_query || !alpha_g1 || !beta_g2 || !out_a || !out_b || !out_c || na == 0 || nb == 0) return 2;
  if ((n_assign && !assignment) || n_aux > n_assign || (n_h && !h) || (nh && !h_query) || (nl && !l_query)) return 2;
  typedef typename C::G1 G1;
  return compose<C>(host_msm<G1>(a_query + 2 * C::Q1, C::HOST_FLAGS), host_msm<typename C::G2>(b_g2_query + 2 * C::Q2, C::HOST_FLAGS), host_msm<G1>(l_query, C::HOST_FLAGS),
                    host_msm<G1>(h_query, C::HOST_FLAGS), KeySide{na, nb, nl, nh, a_query, b_g2_query, alpha_g1, beta_g2}, assignment, n_assign, n_aux, h, n_h, out_a,
                    out_b, out_c);
}
int groth16_prove_761_run(const uint64_t* a_query, size_t na, const uint64_t* b_g2_query, size_t nb, const uint64_t* h_query, size_t nh, const uint64_t* l_query, size_t nl,
                          const uint64_t* alpha_g1, const uint64_t* beta_g2, const uint64_t* assignment, size_t n_assign, size_t n_aux, const uint64_t* h, size_t n_h,
                          uint64_t* out_a, uint64_t* out_b, uint64_t* out_c) {
  return prove_host<Bw6>(a_query, na, b_g2_query, nb, h_query, nh, l_query, nl, alpha_g1, beta_g2, assignment, n_assign, n_aux, h, n_h, out_a, out_b, out_c);
}
int groth16_prove_377_run(const uint64_t* a_query, size_t na, const uint64_t* b_g2_query, size_t nb, const uint64_t* h_query, size_t nh, const uint64_t* l_query, size_t nl,
                          const uint64_t* alpha_g1, const uint64_t* beta_g2, const uint64_t* assignment, size_t n_assign, size_t n_aux, const uint64_t* h, size_t n_h,
                          uint64_t* out_a, uint64_t* out_b, uint64_t* out_c) {
  return prove_host<Bls12>(a_query, na, b_g2_query, nb, h_query, nh, l_query, nl, alpha_g1, beta_g2, assignment, n_assign, n_aux, h, n_h, out_a, out_b, out_c);
}

// ---- the same composition against a LOADED proving key: the queries' fixed-base tables are built once (msm.h FixedTable) and every proof is
// four fixed-base MSMs - the reference creates its Parameters once (crates/epoch-snark/src/api/setup.rs:63-105) and hands the same ones to
// every create_proof_no_zk (prover.rs:78,112).
struct ProvingKey {
  int curve = 0;                                                          // Bw6::CURVE / Bls12::CURVE
  FixedTable *a = nullptr, *b = nullptr, *l = nullptr, *h = nullptr;      // over a_query[1..], b_g2_query[1..], l_query, h_query
  size_t na = 0, nb = 0, nl = 0, nh = 0;
  std::vector<uint64_t> a0, b0, alpha, beta;                              // query[0] and the key elements, affine arkworks limbs
  int device = 0;
};
void groth16_key_free(ProvingKey* k) {
  if (!k) return;
  for (FixedTable* t : {k->a, k->b, k->l, k->h}) if (t) (void)fixed_table_release(t);
  delete k;
}
// one query's table.  resident = 0: host rows, their identity bytes computed here (inf is not read); 1: device rows with the bytes given
template <class G, class Fq, int Q> static int key_table(const uint64_t* rows, const uint8_t* inf, size_t n, int resident, int window_bits, FixedTable** t) {
  if (n == 0) return 0;
  std::vector<uint8_t> f;
  if (!resident) {
    const ArkOne<Fq, Q> one;
    f.resize(n);
    for (size_t i = 0; i < n; i++) f[i] = one.is_zero(rows + i * 2 * Q) ? 1 : 0;
    inf = f.data();
  }
  return MsmApi<G>::fixed_build(rows, inf, n, resident, window_bits, t);
}
// the four queries as they lie (affine arkworks rows, row 0 of a / b included, and for device rows the identity byte of every row), the four
// key elements as host rows.  The tables are built where the rows lie.
template <class C>
static int key_load(int resident, const uint64_t* a, const uint8_t* ainf, size_t na, const uint64_t* b, const uint8_t* binf, size_t nb, const uint64_t* h,
                    const uint8_t* hinf, size_t nh, const uint64_t* l, const uint8_t* linf, size_t nl, const uint64_t* a0, const uint64_t* b0,
                    const uint64_t* alpha_g1, const uint64_t* beta_g2, int window_bits, ProvingKey** out) {
  typedef typename C::G1 G1;
  typedef typename C::Fq Fq;
  constexpr int Q1 = C::Q1, Q2 = C::Q2;
  ProvingKey* k = new ProvingKey();
  k->curve = C::CURVE; k->na = na; k->nb = nb; k->nl = nl; k->nh = nh; k->device = api_device();
  k->a0.assign(a0, a0 + 2 * Q1); k->b0.assign(b0, b0 + 2 * Q2); k->alpha.assign(alpha_g1, alpha_g1 + 2 * Q1); k->beta.assign(beta_g2, beta_g2 + 2 * Q2);
  int rc = key_table<G1, Fq, Q1>(a + 2 * Q1, resident ? ainf + 1 : nullptr, na - 1, resident, window_bits, &k->a);
  if (!rc) rc = key_table<typename C::G2, Fq, Q2>(b + 2 * Q2, resident ? binf + 1 : nullptr, nb - 1, resident, window_bits, &k->b);
  if (!rc) rc = key_table<G1, Fq, Q1>(l, linf, nl, resident, window_bits, &k->l);
  if (!rc) rc = key_table<G1, Fq, Q1>(h, hinf, nh, resident, window_bits, &k->h);
  if (rc) { groth16_key_free(k); return rc; }
  *out = k;
  return 0;
}
int groth16_key_load(int curve, const uint64_t* a_query, size_t na, const uint64_t* b_g2_query, size_t nb, const uint64_t* h_query, size_t nh, const uint64_t* l_query,
                     size_t nl, const uint64_t* alpha_g1, const uint64_t* beta_g2, int window_bits, ProvingKey** out) {
  if (int rc0 = api_enter()) return rc0;
  if (!a_query || !b_g2_query || !alpha_g1 || !beta_g2 || !out || na == 0 || nb == 0 || (nh && !h_query) || (nl && !l_query) || curve < 0 || curve > 1) return 2;
  return (curve ? key_load<Bls12> : key_load<Bw6>)(0, a_query, nullptr, na, b_g2_query, nullptr, nb, h_query, nullptr, nh, l_query, nullptr, nl, a_query, b_g2_query,
                                                   alpha_g1, beta_g2, window_bits, out);
}
// The same key from DEVICE rows (wire_key_load, unit_wire761.hip; groth16_setup, unit_setup.hip)
int groth16_key_load_dev(int curve, const uint64_t* d_a, const uint8_t* d_ainf, size_t na, const uint64_t* d_b, const uint8_t* d_binf, size_t nb,
                         const uint64_t* d_h, const uint8_t* d_hinf, size_t nh, const uint64_t* d_l, const uint8_t* d_linf, size_t nl,
                         const uint64_t* a0, const uint64_t* b0, const uint64_t* alpha_g1, const uint64_t* beta_g2, int window_bits, ProvingKey** out) {
  if (int rc0 = api_enter()) return rc0;
  if (!d_a || !d_b || !a0 || !b0 || !alpha_g1 || !beta_g2 || !out || na == 0 || nb == 0 || (nh && !d_h) || (nl && !d_l) || curve < 0 || curve > 1) return 2;
  return (curve ? key_load<Bls12> : key_load<Bw6>)(1, d_a, d_ainf, na, d_b, d_binf, nb, d_h, d_hinf, nh, d_l, d_linf, nl, a0, b0, alpha_g1, beta_g2, window_bits, out);
}
template <class C>
static int prove_keyed(const ProvingKey* k, const uint64_t* assignment, size_t n_assign, size_t n_aux, const uint64_t* h, size_t n_h, int resident, uint64_t* out_a,
                       uint64_t* out_b, uint64_t* out_c) {
  if (int rc0 = api_enter()) return rc0;
  if (!k || !out_a || !out_b || !out_c || (n_assign && !assignment) || n_aux > n_assign || (n_h && !h)) return 2;
  if (k->device != api_device()) return 101;
  typedef typename C::G1 G1;
  typedef typename C::Fq Fq;
  return compose<C>(fixed_msm<G1, Fq, C::Q1>(k->a, resident), fixed_msm<typename C::G2, Fq, C::Q2>(k->b, resident), fixed_msm<G1, Fq, C::Q1>(k->l, resident),
                    fixed_msm<G1, Fq, C::Q1>(k->h, resident), KeySide{k->na, k->nb, k->nl, k->nh, k->a0.data(), k->b0.data(), k->alpha.data(), k->beta.data()},
                    assignment, n_assign, n_aux, h, n_h, out_a, out_b, out_c);
}
int groth16_prove_keyed(const ProvingKey* k, const uint64_t* assignment, size_t n_assign, size_t n_aux, const uint64_t* h, size_t n_h, uint64_t* out_a, uint64_t* out_b,
                        uint64_t* out_c) {
  // (a null key takes either branch: the checks above refuse it after api_enter, as every entry point does)
  return (k && k->curve ? prove_keyed<Bls12> : prove_keyed<Bw6>)(k, assignment, n_assign, n_aux, h, n_h, 0, out_a, out_b, out_c);
}

// ---- matrices + assignment -> proof (groth16_prove_r1cs_with_key): z goes up once; the constraint rows (unit_r1cs.hip), the witness map and the
// canonical assignment are made on the device and the four fixed-base MSMs read them where they lie.
// z_mode 0: a host pointer; 1: a device pointer, complete before the call, left as it is (the call works on a device copy: its z becomes
// canonical in place); 2: a device pointer the call may overwrite (groth16_hash_helper_prove's own buffer).
template <class C>
static int prove_r1cs_t(const ProvingKey* k, const R1cs* r, size_t n_vars, size_t n_inputs, const uint64_t* z, int z_mode, unsigned log_n, const uint64_t* omega,
                        const uint64_t* omega_inv, const uint64_t* coset, const uint64_t* coset_inv, const uint64_t* n_inv, const uint64_t* z_inv, uint64_t* out_a,
                        uint64_t* out_b, uint64_t* out_c) {
  typedef typename C::FR FR;
  constexpr int A = C::S;
  const size_t n = size_t(1) << log_n;
  CallScope cs;
  HIP_TRY(cs.open(0, nullptr), 10);
  const hipStream_t s = cs.stream();
  uint64_t *d_z, *d_a, *d_b, *d_c;
  if (z_mode == 1) {
    HIP_TRY(cs.alloc(&d_z, n_vars * A * 8), 10);
    HIP_TRY(hipMemcpyAsync(d_z, z, n_vars * A * 8, hipMemcpyDeviceToDevice, s), 10);
  } else {
    HIP_TRY(cs.in(&d_z, z, n_vars * A * 8, z_mode), 10);
  }
  HIP_TRY(cs.alloc(&d_a, n * A * 8), 10); HIP_TRY(cs.alloc(&d_b, n * A * 8), 10); HIP_TRY(cs.alloc(&d_c, n * A * 8), 10);
  if (int rc = r1cs_rows(r, d_z, log_n, d_a, d_b, d_c, 1, s)) return rc;
  if (int rc = witness_map_run<FR>(d_a, d_b, d_c, log_n, omega, omega_inv, coset, coset_inv, n_inv, z_inv, 1, 1, s)) return rc;
  if (n_vars > 1) hipLaunchKernelGGL((k_to_canonical<FR>), dim3((unsigned)((n_vars - 1 + 255) / 256)), dim3(256), 0, s, d_z + A, (uint32_t)(n_vars - 1));
  HIP_TRY(hipGetLastError(), 10);
  HIP_TRY(hipStreamSynchronize(s), 10);
  return prove_keyed<C>(k, d_z + A, n_vars - 1, n_vars - n_inputs, d_a, n, 1, out_a, out_b, out_c);
}
int groth16_prove_r1cs(const ProvingKey* k, const R1cs* r, const uint64_t* z, int z_mode, unsigned log_n, const uint64_t* omega, const uint64_t* omega_inv,
                       const uint64_t* coset, const uint64_t* coset_inv, const uint64_t* n_inv, const uint64_t* z_inv, uint64_t* out_a, uint64_t* out_b, uint64_t* out_c) {
  if (int rc0 = api_enter()) return rc0;
  if (!k || !r || !z || z_mode < 0 || z_mode > 2 || !omega || !omega_inv || !coset || !coset_inv || !n_inv || !z_inv || !out_a || !out_b || !out_c) return 2;
  int curve, device;
  size_t m, n_vars, n_inputs;
  r1cs_shape(r, &curve, &device, &m, &n_vars, &n_inputs);
  if (curve != k->curve) return 2;
  if (k->device != api_device() || device != api_device()) return 101;
  if (log_n > 28 || (size_t(1) << log_n) < m + n_inputs) return 2;
  const WallMs wall;
  const int rc = curve ? prove_r1cs_t<Bls12>(k, r, n_vars, n_inputs, z, z_mode, log_n, omega, omega_inv, coset, coset_inv, n_inv, z_inv, out_a, out_b, out_c)
                       : prove_r1cs_t<Bw6>(k, r, n_vars, n_inputs, z, z_mode, log_n, omega, omega_inv, coset, coset_inv, n_inv, z_inv, out_a, out_b, out_c);
  r1cs_note_ms(4, wall.ms());
  return rc;
}
// the curve and the rows of the four queries (a and b with their row 0, l, h) of a loaded key
void groth16_key_shape(const ProvingKey* k, int* curve, size_t rows[4]) {
  *curve = k->curve;
  rows[0] = k->na; rows[1] = k->nb; rows[2] = k->nl; rows[3] = k->nh;
}
}  // namespace celo
