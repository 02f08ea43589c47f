// Translation unit: chains of epoch transitions to verdicts (transitions.h holds the rule; include/celo_bls_amd.h the contract).  One call,
// one frame, nothing but the outputs crosses back:
//   keys decoded and subgroup-checked once, blocks packed in the inner CIP22 form (unit_epoch.hip) -> CRH -> CIP22 tail, on the device
//   (unit_hash.hip) -> masked key sums, seal b over the rows of block b - 1 (unit_seals.hip) -> signatures decoded (unit_wire.hip) ->
//   k_transition_status -> two-pair products per transition, or one ragged product per chain (the pairing engine).
// DESIGN.md section 6l.
#include "transitions.h"
#include "epoch.h"
#include "pedersen.h"
#include <hip/hip_runtime.h>
#include <cstring>
#include <mutex>
#include <vector>
#include "runtime.h"
#include "units.h"

namespace celo {

// bulk calls, serialised per process (one fills the GPU).  The lock guards nothing else: serialisation only
static std::mutex trans_mu;
static Last<CallTimes> g_trans_last;          // tag[0]: the path; published on every exit of a call that has entered
// the slots of celo_amd_epoch_last, with the products where the proofs are there and the signatures in the spare slot
enum { TR_MS_DECODE = 0, TR_MS_SUMS = 1, TR_MS_PACK = 2, TR_MS_HASH = 3, TR_MS_XFER = 4, TR_MS_PAIR = 5, TR_MS_WALL = 6, TR_MS_SIGS = 7 };

struct TrNegG2 { uint64_t xy[24]; };         // -g2, or the generator's row: affine, arkworks Montgomery limbs
constexpr uint32_t TR_NONE = 0xffffffffu;

// per block, on the device: cid its chain, tidx its place among the transitions (TR_NONE for an initial block)
struct TrIndex { const uint32_t* chain_off; const uint32_t* cid; const uint32_t* tidx; };

// the 7 bytes of extra data of every transition, in the order of the hashes
__global__ void __launch_bounds__(256) k_transition_extras(EpochStaged e, TrIndex x, uint32_t nb, uint8_t* __restrict__ extras) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nb || x.tidx[b] == TR_NONE) return;
  uint8_t o[7];
  epoch_extra(e.index[b], e.round[b], e.mns[b], o);
  for (int i = 0; i < 7; i++) extras[(size_t)x.tidx[b] * 7 + i] = o[i];
}

// lane b -> block b: the facts of transitions.h, the rule, and what the products and the signature sums read: siginf (the signature is the
// identity), sigsel (a transition's signature that decoded into G1) and its complement signot (the flags of the rows the signature sums skip)
__global__ void __launch_bounds__(256) k_transition_status(EpochStaged e, TrIndex x, const uint8_t* __restrict__ bits, const uint32_t* __restrict__ count,
                                                           const uint8_t* __restrict__ wire, const uint8_t* __restrict__ attempts, TrNegG2 gen, uint32_t nb,
                                                           uint8_t* __restrict__ status, uint8_t* __restrict__ siginf, uint8_t* __restrict__ sigsel, uint8_t* __restrict__ signot) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nb) return;
  TransitionFacts f = {};
  f.initial = x.tidx[b] == TR_NONE;
  f.bad_key = e.status[b] != 0;
  if (!f.initial) {
    const uint32_t p = b - 1, first = x.chain_off[x.cid[b]];
    f.pred_bad_key = e.status[p] != 0;
    f.index = e.index[b]; f.pred_index = e.index[p];
    f.n_keys = e.key_off[b + 1] - e.key_off[b]; f.pred_n_keys = e.key_off[b] - e.key_off[p];
    f.entropy_live = transition_entropy_nonzero(e.ee, first);
    f.entropy_equal = transition_entropy_equal(e.pe, b, e.ee, p);
    f.signers = count[p];
    f.pred_max_non_signers = e.mns[p];
    // (read only where the rule gets that far: a set that did not decode has no rows to compare)
    f.padding_selected = !f.bad_key && !f.pred_bad_key && transition_padding_selected(e.rows, e.inf, bits, e.key_off[p], e.key_off[b], gen.xy);
    f.sig_wire = wire[b];
    f.attempt = attempts[x.tidx[b]];
  }
  status[b] = transition_status(f);
  siginf[b] = !f.initial && wire[b] == 1 ? 1 : 0;
  sigsel[b] = !f.initial && wire[b] == 0 ? 1 : 0;
  signot[b] = sigsel[b] ^ 1;
}

// "each": product b = (sig_b, -g2), (H_b, apk_{b-1}); one lane per (block, u64 of a G2 row).  A block with skip set has both G1 sides flagged:
// its pairs contribute 1 and none is evaluated.
__global__ void __launch_bounds__(256) k_pack_transition_pairs(const uint64_t* __restrict__ sig, const uint8_t* __restrict__ siginf, const uint64_t* __restrict__ hash,
                                                               const uint64_t* __restrict__ apk, const uint8_t* __restrict__ apkinf, const uint8_t* __restrict__ skip,
                                                               const uint32_t* __restrict__ tidx, TrNegG2 ng2, uint32_t nb, uint64_t* __restrict__ g1,
                                                               uint64_t* __restrict__ g2, uint8_t* __restrict__ i1, uint8_t* __restrict__ i2) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t b = t / 24;
  const uint32_t w = (uint32_t)(t % 24);
  if (b >= nb) return;
  const bool off = skip[b] != 0 || tidx[b] == TR_NONE;
  const size_t h = off ? 0 : tidx[b], p = off ? 0 : b - 1;
  if (w < 12) { g1[(2 * b) * 12 + w] = off ? 0 : sig[b * 12 + w]; g1[(2 * b + 1) * 12 + w] = off ? 0 : hash[h * 12 + w]; }
  g2[(2 * b) * 24 + w] = ng2.xy[w];
  g2[(2 * b + 1) * 24 + w] = off ? ng2.xy[w] : apk[p * 24 + w];
  if (w == 0) {
    i1[2 * b] = off ? 1 : siginf[b]; i1[2 * b + 1] = off ? 1 : 0;
    i2[2 * b] = 0; i2[2 * b + 1] = off ? 0 : apkinf[p];
  }
}
// "chain": pair b of product cid[b] is (sum of the chain's signatures, -g2) at the chain's initial block and (H_b, apk_{b-1}) at a transition,
// so the products' offsets are chain_off.  skip: per chain.
__global__ void __launch_bounds__(256) k_pack_chain_pairs(const uint64_t* __restrict__ asig, const uint8_t* __restrict__ asiginf, const uint64_t* __restrict__ hash,
                                                          const uint64_t* __restrict__ apk, const uint8_t* __restrict__ apkinf, const uint8_t* __restrict__ skip,
                                                          TrIndex x, TrNegG2 ng2, uint32_t nb, uint64_t* __restrict__ g1, uint64_t* __restrict__ g2,
                                                          uint8_t* __restrict__ i1, uint8_t* __restrict__ i2) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t b = t / 24;
  const uint32_t w = (uint32_t)(t % 24);
  if (b >= nb) return;
  const uint32_t c = x.cid[b];
  const bool off = skip[c] != 0, head = x.tidx[b] == TR_NONE;
  const size_t h = head ? 0 : x.tidx[b], p = head ? 0 : b - 1;
  if (w < 12) g1[b * 12 + w] = off ? 0 : head ? asig[(size_t)c * 12 + w] : hash[h * 12 + w];
  g2[b * 24 + w] = off || head ? ng2.xy[w] : apk[p * 24 + w];
  if (w == 0) {
    i1[b] = off ? 1 : head ? asiginf[c] : 0;
    i2[b] = off || head ? 0 : apkinf[p];
  }
}

static TrNegG2 transitions_generator_row() {
  TrNegG2 g;
  Fq::from_limbs(T377::G2_GEN_X0).to_ark(g.xy); Fq::from_limbs(T377::G2_GEN_X1).to_ark(g.xy + 6);
  Fq::from_limbs(T377::G2_GEN_Y0).to_ark(g.xy + 12); Fq::from_limbs(T377::G2_GEN_Y1).to_ark(g.xy + 18);
  return g;
}

int verify_epoch_transitions(const EpochBlocks* blocks, size_t nb, const uint32_t* chain_off, size_t n_chains, const uint8_t* bits, const uint8_t* sig48,
                             const uint8_t* domain, const uint64_t neg_g2_xy[24], int mode, uint8_t* out_ok, uint8_t* out_status, uint8_t* out_chain_ok, uint8_t* out_crh,
                             uint8_t* out_attempts, uint64_t* out_asig_xy, uint8_t* out_asig_inf) {
  if (nb == 0) return 0;
  // ---- what needs no device
  if (!blocks || !chain_off || !bits || !sig48 || !domain || !neg_g2_xy || !out_ok || (mode != 0 && mode != 1)) return 2;
  if (n_chains == 0 || n_chains > nb || chain_off[0] != 0 || chain_off[n_chains] != nb) return 2;
  for (size_t c = 0; c < n_chains; c++) if (chain_off[c + 1] <= chain_off[c]) return 2;
  if (int rc = epoch_refuse_blocks(*blocks, nb, true)) return rc;
  const EpochBlocks& B = *blocks;
  std::vector<uint32_t> cid(nb), tidx(nb);
  std::vector<uint64_t> out_off(nb + 1), msg_off, seven, fortyeight;
  out_off[0] = 0;
  size_t T = 0;
  for (size_t c = 0; c < n_chains; c++)
    for (size_t b = chain_off[c]; b < chain_off[c + 1]; b++) {
      const uint64_t bytes = (epoch_encoded_bits(2, B.key_off[b + 1] - B.key_off[b], B.max_validators[b]) + 7) / 8;
      if ((bytes + 8) * 8 > PEDERSEN_MAX_BITS) return 2;           // counter || extra || encoding past the generator table: the reference panics
      const bool initial = b == chain_off[c];
      cid[b] = (uint32_t)c;
      tidx[b] = initial ? TR_NONE : (uint32_t)T++;
      out_off[b + 1] = out_off[b] + (initial ? 0 : bytes);
      if (!initial) msg_off.push_back(out_off[b]);
    }
  msg_off.push_back(out_off[nb]);
  seven.resize(T + 1); fortyeight.resize(T + 1);
  for (size_t t = 0; t <= T; t++) { seven[t] = 7 * t; fortyeight[t] = 48 * t; }
  if (int rc0 = api_enter()) return rc0;
  std::lock_guard<std::mutex> lk(trans_mu);
  TimedCall call(g_trans_last, TR_MS_WALL);
  float* const ms = call.t.ms;
  TrNegG2 ng2;
  for (int q = 0; q < 24; q++) ng2.xy[q] = neg_g2_xy[q];
  static const TrNegG2 gen = transitions_generator_row();
  const uint32_t nb32 = (uint32_t)nb, nc32 = (uint32_t)n_chains;
  std::vector<uint8_t> h_status(nb), h_crh, h_att, h_ainf(n_chains, 1);
  std::vector<uint8_t> each(nb, 0);        // verdicts of the two-pair products, where one was run
  int path = mode;
  CallScope cs;
  HIP_TRY(cs.open(0, nullptr), 10);
  const hipStream_t s = cs.stream();
  EvLog log(s);
  // ---- 1, 2: the keys once, the inner encodings of the transitions
  EpochStaged E;
  if (int rc = epoch_stage_bytes(cs, log, B, nb, 2, out_off.data(), &E)) return rc;
  TrIndex X;
  uint32_t *d_chain_off, *d_cid, *d_tidx, *d_count;
  uint8_t *d_bits, *d_sig48, *d_extras, *d_crh, *d_att, *d_wire, *d_status, *d_siginf, *d_sigsel, *d_signot, *d_apkinf, *d_asiginf, *d_skip;
  uint64_t *d_hash, *d_apk, *d_sig, *d_asig;
  hipEvent_t e0 = log.open();
  HIP_TRY(cs.in(&d_chain_off, chain_off, (n_chains + 1) * 4, 0), 10);
  HIP_TRY(cs.in(&d_cid, cid.data(), nb * 4, 0), 10);
  HIP_TRY(cs.in(&d_tidx, tidx.data(), nb * 4, 0), 10);
  HIP_TRY(cs.in(&d_bits, bits, B.key_off[nb], 0, 8), 10);
  HIP_TRY(cs.in(&d_sig48, sig48, nb * 48, 0), 10);
  log.close(TR_MS_XFER, e0);
  X = {d_chain_off, d_cid, d_tidx};
  HIP_TRY(cs.alloc(&d_extras, T * 7 + 8), 10);
  HIP_TRY(cs.alloc(&d_crh, T * 48 + 8), 10);
  HIP_TRY(cs.alloc(&d_att, T + 8), 10);
  HIP_TRY(cs.alloc(&d_hash, T * 96 + 8), 10);
  HIP_TRY(cs.alloc(&d_count, nb * 4), 10);
  HIP_TRY(cs.alloc(&d_apk, nb * 192), 10);
  HIP_TRY(cs.alloc(&d_apkinf, nb), 10);
  HIP_TRY(cs.alloc(&d_sig, nb * 96), 10);
  HIP_TRY(cs.alloc(&d_wire, nb), 10);
  HIP_TRY(cs.alloc(&d_status, nb), 10);
  HIP_TRY(cs.alloc(&d_siginf, nb), 10);
  HIP_TRY(cs.alloc(&d_sigsel, nb + 8), 10);
  HIP_TRY(cs.alloc(&d_signot, nb + 8), 10);
  HIP_TRY(cs.alloc(&d_asig, n_chains * 96), 10);
  HIP_TRY(cs.alloc(&d_asiginf, n_chains), 10);
  HIP_TRY(cs.alloc(&d_skip, nb), 10);
  // ---- 3: CRH -> CIP22 tail; the bytes, the rows and the counters stay on the device (the hash unit runs on this call's stream)
  if (T) {
    e0 = log.open();
    hipLaunchKernelGGL(k_transition_extras, dim3((nb32 + 255) / 256), dim3(256), 0, s, E, X, nb32, d_extras);
    log.close(TR_MS_PACK, e0);
    HIP_TRY(hipGetLastError(), 10);
    float ms_crh = 0.f;
    if (int rc = pedersen_crh_run(E.bytes, msg_off.data(), T, d_crh, 1, s, &ms_crh)) return rc;
    if (int rc = hash_to_g1_direct_run(domain, d_crh, fortyeight.data(), d_extras, seven.data(), T, d_hash, d_att, 1, 1, s, &ms[TR_MS_HASH])) return rc;
    ms[TR_MS_HASH] += ms_crh;
  }
  // ---- 4: seal p = the keys of block p under the bytes below them: the aggregated key of transition p + 1 (the last of a chain signs nothing here)
  e0 = log.open();
  if (int rc = aggregate_by_bitmap(1, E.rows, E.inf, B.key_off, nb, d_bits, nb, d_apk, d_apkinf, d_count, 1, s)) return rc;
  log.close(TR_MS_SUMS, e0);
  // ---- 5, 6: signatures, statuses
  if (int rc = wire_decompress(0, d_sig48, nb, 1, d_sig, d_wire, 1, s, &ms[TR_MS_SIGS])) return rc;
  e0 = log.open();
  hipLaunchKernelGGL(k_transition_status, dim3((nb32 + 255) / 256), dim3(256), 0, s, E, X, d_bits, d_count, d_wire, d_att, gen, nb32, d_status, d_siginf, d_sigsel, d_signot);
  log.close(TR_MS_SIGS, e0);
  HIP_TRY(hipGetLastError(), 10);
  // the sum of every chain's decoded signatures: the masked sums again, chains as sets
  const bool want_asig = out_asig_xy || out_asig_inf;
  if (T && (mode == 1 || want_asig)) {
    e0 = log.open();
    if (int rc = aggregate_by_bitmap(0, d_sig, d_signot, chain_off, n_chains, d_sigsel, n_chains, d_asig, d_asiginf, nullptr, 1, s)) return rc;
    log.close(TR_MS_SUMS, e0);
  }
  e0 = log.open();
  HIP_TRY(hipMemcpyAsync(h_status.data(), d_status, nb, hipMemcpyDeviceToHost, s), 10);
  if (T && out_crh) { h_crh.resize(T * 48); HIP_TRY(hipMemcpyAsync(h_crh.data(), d_crh, T * 48, hipMemcpyDeviceToHost, s), 10); }
  if (T && out_attempts) { h_att.resize(T); HIP_TRY(hipMemcpyAsync(h_att.data(), d_att, T, hipMemcpyDeviceToHost, s), 10); }
  if (T && out_asig_xy) HIP_TRY(hipMemcpyAsync(out_asig_xy, d_asig, n_chains * 96, hipMemcpyDeviceToHost, s), 10);
  if (T && want_asig) HIP_TRY(hipMemcpyAsync(h_ainf.data(), d_asiginf, n_chains, hipMemcpyDeviceToHost, s), 10);
  log.close(TR_MS_XFER, e0);
  HIP_TRY(hipStreamSynchronize(s), 10);
  // ---- 7: products
  std::vector<uint8_t> chain_clean(n_chains), chain_held(n_chains, 0), skip(nb, 0);
  size_t clean = 0;
  for (size_t c = 0; c < n_chains; c++) {
    bool all = true;
    for (size_t b = chain_off[c]; b < chain_off[c + 1]; b++) {
      all = all && h_status[b] == 0;
      clean += h_status[b] == 0 && b != chain_off[c];
    }
    chain_clean[c] = all;
  }
  if (mode == 1 && clean) {
    std::vector<uint8_t> cskip(n_chains), v(n_chains, 0);
    size_t run = 0;
    for (size_t c = 0; c < n_chains; c++) {
      cskip[c] = !(chain_clean[c] && chain_off[c + 1] - chain_off[c] > 1);
      run += !cskip[c];
    }
    if (run) {
      HIP_TRY(hipMemcpyAsync(d_skip, cskip.data(), n_chains, hipMemcpyHostToDevice, s), 10);
      StagedProduct<Pairing377> g;
      if (int rc = g.stage(nb32, n_chains)) return rc;
      if (int rc = g.after(cs)) return rc;
      hipLaunchKernelGGL(k_pack_chain_pairs, dim3((unsigned)((nb * 24 + 255) / 256)), dim3(256), 0, g.ps.stream, d_asig, d_asiginf, d_hash, d_apk, d_apkinf, d_skip, X, ng2, nb32,
                         g.ps.d_g1, g.ps.d_g2, g.ps.d_i1, g.ps.d_i2);
      HIP_TRY(hipGetLastError(), 10);
      if (int rc = g.run(chain_off, n_chains, v.data(), &ms[TR_MS_PAIR])) return rc;
      HIP_TRY(hipStreamSynchronize(s), 10);
    }
    for (size_t c = 0; c < n_chains; c++) {
      if (!cskip[c] && v[c]) {
        chain_held[c] = 1;
        for (size_t b = chain_off[c]; b < chain_off[c + 1]; b++) { skip[b] = 1; clean -= b != chain_off[c]; }
      } else if (!cskip[c]) path = 2;
    }
  }
  if (clean) {
    for (size_t b = 0; b < nb; b++) skip[b] = skip[b] || h_status[b] != 0;
    HIP_TRY(hipMemcpyAsync(d_skip, skip.data(), nb, hipMemcpyHostToDevice, s), 10);
    StagedProduct<Pairing377> g;
    if (int rc = g.stage(2 * nb32, nb)) return rc;
    if (int rc = g.after(cs)) return rc;
    hipLaunchKernelGGL(k_pack_transition_pairs, dim3((unsigned)((nb * 24 + 255) / 256)), dim3(256), 0, g.ps.stream, d_sig, d_siginf, d_hash, d_apk, d_apkinf, d_skip, d_tidx, ng2,
                       nb32, g.ps.d_g1, g.ps.d_g2, g.ps.d_i1, g.ps.d_i2);
    HIP_TRY(hipGetLastError(), 10);
    std::vector<uint32_t> off(nb + 1);
    for (size_t p = 0; p <= nb; p++) off[p] = (uint32_t)(2 * p);
    if (int rc = g.run(off.data(), nb, each.data(), &ms[TR_MS_PAIR])) return rc;
    HIP_TRY(hipStreamSynchronize(s), 10);
  }
  log.sum(ms);
  call.t.tag[0] = path;
  // ---- the outputs
  for (size_t c = 0; c < n_chains; c++) {
    bool all = true;
    for (size_t b = chain_off[c]; b < chain_off[c + 1]; b++) {
      const bool initial = b == chain_off[c];
      uint8_t st = h_status[b];
      if (st == 0 && !initial && !chain_held[c] && !each[b]) st = TR_PRODUCT;
      out_ok[b] = st == 0 ? 1 : 0;
      if (out_status) out_status[b] = st;
      all = all && st == 0;
      if (out_crh) { if (initial) memset(out_crh + b * 48, 0, 48); else memcpy(out_crh + b * 48, h_crh.data() + (size_t)tidx[b] * 48, 48); }
      if (out_attempts) out_attempts[b] = initial ? 0 : h_att[tidx[b]];
    }
    if (out_chain_ok) out_chain_ok[c] = all ? 1 : 0;
    if (out_asig_inf) out_asig_inf[c] = h_ainf[c];
    if (out_asig_xy && (h_ainf[c] || !T)) memset(out_asig_xy + c * 12, 0, 96);
  }
  return 0;
}

void transitions_last(int* path, float ms[8]) {
  const CallTimes t = g_trans_last.read();
  *path = t.tag[0];
  for (int i = 0; i < 8; i++) ms[i] = t.ms[i];
}

}  // namespace celo
