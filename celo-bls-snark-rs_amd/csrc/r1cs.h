// R1CS matrices as data: the two sparse matrix-vector products over the curve's scalar field that ark-groth16 0.1 runs between synthesis and
// the entry points of unit_prover.hip / unit_setup.hip (r1cs_to_qap.rs), and the Lagrange basis at tau.
//   prover  (R1CStoQAP::witness_map, constraint evaluation):        (A z)_j = sum_k A[j][k] z_k          the matrices with the assignment
//   setup   (R1CStoQAP::instance_map_with_evaluation):              a_i(tau) = sum_j A[j][i] L_j(tau)    their transposes with L(tau)
// One matrix = CSR: row_ptr (u64[rows + 1]), col (u32[nnz]), val (nnz x N64 arkworks Montgomery limbs).  Every routine here is HD or plain
// host code: the kernels of unit_r1cs.hip and the host twins of host_test.cpp (-DCELO_FP_TRACK) run the same bodies.
//
// The running sum.  A term is mul(repack(val), repack(vec[col])) of the two arkworks forms AS THEY LIE (x R_a, R_a = 2^(64 N64)): the product
// x y R_a^2 / R_d, one Montgomery pass per non-zero and no conversion of either operand; the sum of a row is turned into the arkworks form
// of the result by ONE more product with C_IN = R_d^2 / R_a (r1cs_finish), in place of two from_ark and one to_ark per term.
// Bound (fp.h contract, checked by the tracker on every twin run): a product has lb 1, vb < 2; add() admits lb <= 15.  A sum that starts
// from a weakly reduced value (wred: lb 1, vb 3) therefore takes R1CS_LAZY = 14 products (lb 15, vb 31 <= wred's 300) before the next
// wred.  Partial sums (lanes of a chunk, chunks of a row) are stored weakly reduced and added under the same rule (14 x vb 3 + 3 = 45).
#pragma once
#include <vector>
#include "fixed_base.h"

namespace celo {

constexpr uint32_t R1CS_LAZY = 14;        // products (or stored partial sums) added between two weak reductions
constexpr uint32_t R1CS_LONG = 128;       // a list of more entries than this is cut into chunks
constexpr uint32_t R1CS_CHUNK = 1024;     // entries per chunk: one wave, lane t takes entries t, t + 64, ...
constexpr uint32_t R1CS_WAVE = 64;
constexpr uint32_t R1CS_LAG_BLOCK = 8;    // domain points per lane of the Lagrange kernel (one inversion per lane)
constexpr int R1CS_ERR_MATRIX = 34;       // a matrix failed validation (30-33: the serialized key's codes)

struct R1csCsr { const uint64_t* row_ptr; const uint32_t* col; const uint64_t* val; uint64_t nnz; };

// ---- validation (host).  0; 2 for a bad shape (n_inputs == 0, n_inputs > n_vars, n_vars, rows or nnz >= 2^32, a NULL array);
// R1CS_ERR_MATRIX with *first_bad = matrix index << 60 | row index (row_ptr faults: a row whose end lies before its start, row 0 for
// row_ptr[0] != 0, row `rows` for row_ptr[rows] != nnz) or entry index (col >= n_vars, val >= the modulus).
template <int N64>
inline int r1cs_validate(size_t rows, size_t n_vars, size_t n_inputs, const R1csCsr* mats, const uint64_t* modulus, uint64_t* first_bad) {
  if (n_inputs == 0 || n_inputs > n_vars || n_vars >> 32 || rows >> 32 || !mats) return 2;
  for (int k = 0; k < 3; k++) {
    const R1csCsr& M = mats[k];
    if (!M.row_ptr || M.nnz >> 32 || (M.nnz && (!M.col || !M.val))) return 2;
  }
  auto bad = [&](int k, uint64_t i) { if (first_bad) *first_bad = ((uint64_t)k << 60) | i; return R1CS_ERR_MATRIX; };
  for (int k = 0; k < 3; k++) {
    const R1csCsr& M = mats[k];
    if (M.row_ptr[0] != 0) return bad(k, 0);
    for (size_t j = 0; j < rows; j++) if (M.row_ptr[j + 1] < M.row_ptr[j]) return bad(k, j);
    if (M.row_ptr[rows] != M.nnz) return bad(k, rows);
    for (uint64_t e = 0; e < M.nnz; e++) {
      if (M.col[e] >= n_vars) return bad(k, e);
      if (!fb_below<N64>(M.val + e * N64, modulus)) return bad(k, e);
    }
  }
  return 0;
}

// ---- the transpose of a matrix (host, once per load): column-major lists in row order within a column (a counting sort), the row index
// where the matrix held the column index
template <int N64>
inline void r1cs_transpose(size_t rows, size_t n_vars, const R1csCsr& M, std::vector<uint64_t>& t_ptr, std::vector<uint32_t>& t_idx, std::vector<uint64_t>& t_val) {
  t_ptr.assign(n_vars + 1, 0);
  t_idx.resize(M.nnz);
  t_val.resize(M.nnz * N64);
  for (uint64_t e = 0; e < M.nnz; e++) t_ptr[M.col[e] + 1]++;
  for (size_t i = 0; i < n_vars; i++) t_ptr[i + 1] += t_ptr[i];
  std::vector<uint64_t> at(t_ptr.begin(), t_ptr.end() - 1);
  for (size_t j = 0; j < rows; j++) {
    for (uint64_t e = M.row_ptr[j]; e < M.row_ptr[j + 1]; e++) {
      const uint64_t d = at[M.col[e]]++;
      t_idx[d] = (uint32_t)j;
      for (int k = 0; k < N64; k++) t_val[d * N64 + k] = M.val[e * N64 + k];
    }
  }
}

// ---- the binning (host, once per load): the lists above R1CS_LONG entries and their chunks.  Chunk c belongs to long list li = chunk_li[c]
// (row long_rows[li]) and is its (c - long_first[li])-th piece of R1CS_CHUNK entries; long_first has n_long + 1 entries.
struct R1csBins { std::vector<uint32_t> long_rows, long_first, chunk_li; };
inline R1csBins r1cs_bin(const uint64_t* row_ptr, size_t rows) {
  R1csBins b;
  b.long_first.push_back(0);
  for (size_t r = 0; r < rows; r++) {
    const uint64_t len = row_ptr[r + 1] - row_ptr[r];
    if (len <= R1CS_LONG) continue;
    const uint32_t nch = (uint32_t)((len + R1CS_CHUNK - 1) / R1CS_CHUNK);
    for (uint32_t k = 0; k < nch; k++) b.chunk_li.push_back((uint32_t)b.long_rows.size());
    b.long_rows.push_back((uint32_t)r);
    b.long_first.push_back((uint32_t)b.chunk_li.size());
  }
  return b;
}

// ---- the sums
// entries lo, lo + step, ... below hi of one list: weakly reduced on return (lb 1, vb 3)
template <class FR>
HD FR r1cs_sum(const uint32_t* __restrict__ col, const uint64_t* __restrict__ val, const uint64_t* __restrict__ vec, uint64_t lo, uint64_t hi, uint32_t step) {
  constexpr int A = FR::ARK64;
  FR acc = FR::zero();
  uint32_t pend = 0;
  for (uint64_t e = lo; e < hi; e += step) {
    acc = FR::add(acc, FR::mul(FR::repack_from64(val + e * A), FR::repack_from64(vec + (size_t)col[e] * A)));
    if (++pend == R1CS_LAZY) { acc = FR::wred(acc); pend = 0; }
  }
  return FR::wred(acc);
}
// a stored partial sum: weakly reduced when it was written, and loaded with that bound (F::load alone declares vb 64)
template <class FR> HD FR r1cs_load_part(const uint32_t* p) { FR r = FR::load(p); TRK(r.lb = 1; r.vb = 3;) return r; }
// stored partial sums lo, lo + step, ... below hi, in that order: weakly reduced on return
template <class FR> HD FR r1cs_combine(const uint32_t* parts, uint32_t lo, uint32_t hi, uint32_t step) {
  FR acc = FR::zero();
  uint32_t pend = 0;
  for (uint32_t k = lo; k < hi; k += step) {
    acc = FR::add(acc, r1cs_load_part<FR>(parts + (size_t)k * FR::WORDS));
    if (++pend == R1CS_LAZY) { acc = FR::wred(acc); pend = 0; }
  }
  return FR::wred(acc);
}
// a row's sum of products -> the arkworks form of the result (header comment)
template <class P> HD void r1cs_finish(const Fp<P>& acc, uint64_t* out) {
  Fp<P>::reduce(Fp<P>::mul(acc, Fp<P>::from_limbs(P::C_IN))).repack_to64(out);
}
// the piece of chunk k of a list [lo, hi)
HD void r1cs_chunk_range(uint64_t lo, uint64_t hi, uint32_t k, uint64_t& c_lo, uint64_t& c_hi) {
  c_lo = lo + (uint64_t)k * R1CS_CHUNK;
  c_hi = c_lo + R1CS_CHUNK < hi ? c_lo + R1CS_CHUNK : hi;
}

// The whole product in the kernels' order, on the host (the twin of k_r1cs_short / k_r1cs_chunk / k_r1cs_long): out = rows x N64.  A long list:
// a wave per chunk (lane t the entries t, t + 64, ...; the 64 lane sums added in lane order), then a wave per list over the chunk sums in the
// same two steps - a list of 2 400 chunks (column 0 of a 2^22-constraint matrix) is not one lane's serial loop.
template <class FR>
inline void r1cs_matvec_host(const uint64_t* row_ptr, const uint32_t* col, const uint64_t* val, size_t rows, const uint64_t* vec, uint64_t* out) {
  constexpr int A = FR::ARK64, FW = FR::WORDS;
  std::vector<uint32_t> lanes(R1CS_WAVE * FW), parts;
  for (size_t r = 0; r < rows; r++) {
    const uint64_t lo = row_ptr[r], hi = row_ptr[r + 1];
    if (hi - lo <= R1CS_LONG) { r1cs_finish(r1cs_sum<FR>(col, val, vec, lo, hi, 1), out + r * A); continue; }
    const uint32_t nch = (uint32_t)((hi - lo + R1CS_CHUNK - 1) / R1CS_CHUNK);
    parts.assign((size_t)nch * FW, 0);
    for (uint32_t k = 0; k < nch; k++) {
      uint64_t c_lo, c_hi;
      r1cs_chunk_range(lo, hi, k, c_lo, c_hi);
      for (uint32_t t = 0; t < R1CS_WAVE; t++) r1cs_sum<FR>(col, val, vec, c_lo + t, c_hi, R1CS_WAVE).store(lanes.data() + (size_t)t * FW);
      r1cs_combine<FR>(lanes.data(), 0, R1CS_WAVE, 1).store(parts.data() + (size_t)k * FW);
    }
    for (uint32_t t = 0; t < R1CS_WAVE; t++) r1cs_combine<FR>(parts.data(), t, nch, R1CS_WAVE).store(lanes.data() + (size_t)t * FW);
    r1cs_finish(r1cs_combine<FR>(lanes.data(), 0, R1CS_WAVE, 1), out + r * A);
  }
}

// ---- the Lagrange basis at tau over the domain {omega^j}, j < n:  L_j = c omega^j / (tau - omega^j),  c = Z(tau) / n.
// One lane takes cnt <= R1CS_LAG_BLOCK consecutive points: the powers forwards from omega^j0, the prefix products of the denominators, ONE
// inversion (Montgomery's trick), then backwards with omega^-1.  A denominator of zero (tau = omega^j, where Z(tau) = c = 0) stands in the
// products as one and its L_j is one: the basis' definition, L_j(omega^k) = [j == k]; every other L of such a tau is c (...) = 0.
// c, tau, omega, omega_inv: device form, normalised.  out: arkworks limbs.
template <class P>
HD void r1cs_lagrange_block(const Fp<P>& c, const Fp<P>& tau, const Fp<P>& omega, const Fp<P>& omega_inv, uint64_t j0, uint32_t cnt, uint64_t* out) {
  typedef Fp<P> FR;
  constexpr int A = FR::ARK64;
  FR pre[R1CS_LAG_BLOCK];
  FR w = FR::norm(FR::pow64(omega, &j0, 1)), run = FR::one();
  uint32_t zero = 0;
#pragma unroll
  for (uint32_t k = 0; k < R1CS_LAG_BLOCK; k++) {
    if (k < cnt) {
      if (k) w = FR::mul(w, omega);
      FR d = FR::norm(FR::template sub<4, 1>(tau, w));
      if (d.is_zero_mod_p()) { zero |= 1u << k; d = FR::one(); }
      pre[k] = run;
      run = FR::mul(run, d);
    }
  }
  FR inv = FR::norm(FR::inv(run));
#pragma unroll
  for (uint32_t kk = 0; kk < R1CS_LAG_BLOCK; kk++) {
    const uint32_t k = R1CS_LAG_BLOCK - 1 - kk;
    if (k < cnt) {
      const bool z = (zero >> k) & 1u;
      const FR d = z ? FR::one() : FR::norm(FR::template sub<4, 1>(tau, w));
      const FR lk = z ? FR::one() : FR::mul(FR::mul(c, w), FR::mul(inv, pre[k]));
      lk.to_ark(out + (j0 + k) * A);
      inv = FR::mul(inv, d);
      w = FR::mul(w, omega_inv);
    }
  }
}
// the constants of the Lagrange step from arkworks limbs (host): zt = tau^n - 1 (written to zt_ark), c = zt / n, omega^-1
template <class FR> struct R1csLagConsts { FR c, tau, omega, omega_inv; };
template <class FR> inline R1csLagConsts<FR> r1cs_lagrange_consts(unsigned log_n, const uint64_t* omega_ark, const uint64_t* tau_ark, uint64_t* zt_ark) {
  R1csLagConsts<FR> k;
  k.tau = FR::norm(FR::from_ark(tau_ark));
  k.omega = FR::norm(FR::from_ark(omega_ark));
  k.omega_inv = FR::norm(FR::inv(k.omega));
  FR t = k.tau;
  for (unsigned i = 0; i < log_n; i++) t = FR::sqr(t);
  const FR zt = FR::norm(FR::template sub<4, 1>(t, FR::one()));
  zt.to_ark(zt_ark);
  uint64_t nn[FR::ARK64] = {};
  nn[0] = uint64_t(1) << log_n;
  k.c = FR::norm(FR::mul(zt, FR::inv(FR::from_canonical(nn))));
  return k;
}
// a_i += L_(rows + i) for the instance variables (both arkworks limbs)
template <class FR> HD void r1cs_add_input(uint64_t* a, const uint64_t* l) {
  FR::add(FR::from_ark(a), FR::from_ark(l)).to_ark(a);
}
// (A z)_j (B z)_j == (C z)_j
template <class FR> HD bool r1cs_row_holds(const uint64_t* a, const uint64_t* b, const uint64_t* c) {
  return FR::eq_mod_p(FR::mul(FR::from_ark(a), FR::from_ark(b)), FR::from_ark(c));
}

}  // namespace celo
