// Translation unit: epoch blocks to bytes, to the two Groth16 public inputs of the epoch proof, and to verdicts (epoch.h; what
// epoch_snark::verify does per proof on the host, crates/epoch-snark/src/api/verifier.rs:23-40, for m proofs on the device):
//   keys decoded and subgroup-checked (unit_wire.hip) -> the last blocks' key sums (unit_seals.hip) -> one 755-bit record per key ->
//   the byte streams gathered word by word into 64-byte-aligned slots -> Blake2s per slot -> 376 | 136 bit inputs -> the batch verifier
//   (groth16_verify_unit.h), which reads the inputs and the block statuses where they lie.
// DESIGN.md section 6k.
#include "epoch.h"
#include <hip/hip_runtime.h>
#include <cstring>
#include <mutex>
#include <vector>
#include "runtime.h"
#include "units.h"

namespace celo {

// bulk calls, serialised per process like the decoders' (one fills the GPU).  The lock guards nothing else: serialisation only
static std::mutex epoch_mu;
static Last<CallTimes> g_epoch_last;          // published on every exit of a call that has entered
enum { EP_DECODE = 0, EP_SUMS = 1, EP_PACK = 2, EP_HASH = 3, EP_XFER = 4, EP_VERIFY = 5, EP_WALL = 6 };

// the per-block fields on the device
struct EpochFields {
  const uint16_t* index; const uint8_t* round; const uint32_t* mns; const uint32_t* maxv; const uint8_t* ee; const uint8_t* pe; const uint32_t* key_off;
};

// lane b -> block b: a key that is the identity (or did not decode) is flagged for the sums; a key that does not decode or lies outside G2
// spoils its block.  kst: the decoder's statuses (keys_form 0) or null; inf_in: the caller's flags (keys_form 1) or null
__global__ void __launch_bounds__(256) k_epoch_block_status(const uint32_t* __restrict__ key_off, const uint8_t* __restrict__ kst, const uint8_t* __restrict__ inf_in,
                                                            uint32_t nb, uint8_t* __restrict__ inf_out, uint8_t* __restrict__ status) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nb) return;
  uint8_t bad = 0;
  for (uint32_t k = key_off[b]; k < key_off[b + 1]; k++) {
    const uint8_t s = kst ? kst[k] : 0;
    inf_out[k] = (s != WIRE_OK || (inf_in && inf_in[k])) ? 1 : 0;
    if (s >= WIRE_INVALID) bad = 1;
  }
  status[b] = bad;
}
// one lane per key: its record (epoch.h)
__global__ void __launch_bounds__(64) k_epoch_key_record(const uint64_t* __restrict__ rows, const uint8_t* __restrict__ inf, uint32_t n, uint32_t* __restrict__ recs) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t rec[EPOCH_REC_WORDS];
  epoch_key_record(rows + (size_t)i * 24, inf && inf[i], rec);
  uint32_t* o = recs + (size_t)i * EPOCH_REC_WORDS;
#pragma unroll
  for (int j = 0; j < (int)EPOCH_REC_WORDS; j++) o[j] = rec[j];
}
// A gather, one lane per 32-bit word of the slots: slot b holds block b's bytes from word slot_off[b] on and zeros up to slot_off[b + 1], a
// multiple of 16 words - every word of the slots is written here, so the hash kernel reads nothing else.  recs: the key records, the
// generator's behind the last key (index key_off[nb]); sums: one record per block (kind 1) or null.  A spoiled block is zero-filled.
__global__ void __launch_bounds__(256) k_epoch_pack(EpochFields f, int kind, uint32_t nb, const uint64_t* __restrict__ slot_off, const uint32_t* __restrict__ recs,
                                                    const uint32_t* __restrict__ sums, const uint8_t* __restrict__ status, uint32_t* __restrict__ slots) {
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= slot_off[nb]) return;
  const uint32_t b = epoch_find_block<uint64_t>(slot_off, nb, g);
  if (status[b]) { slots[g] = 0; return; }
  const uint32_t k0 = f.key_off[b], n_keys = f.key_off[b + 1] - k0, nk = epoch_key_slots(kind, n_keys, f.maxv[b]);
  const uint64_t w = g - slot_off[b];
  uint32_t hd[EPOCH_HDR_WORDS] = {};
  if (32 * (w + 1) > (uint64_t)EPOCH_KEY_BITS * nk)
    epoch_header(kind, f.index[b], f.mns[b], f.ee ? f.ee + (size_t)b * 16 : nullptr, f.pe ? f.pe + (size_t)b * 16 : nullptr, hd);
  slots[g] = epoch_pack_word(kind, w, n_keys, nk, hd, recs + (size_t)k0 * EPOCH_REC_WORDS, recs + (size_t)f.key_off[nb] * EPOCH_REC_WORDS,
                             sums ? sums + (size_t)b * EPOCH_REC_WORDS : nullptr);
}
// one lane per message (epoch.h epoch_blake2s): digest b = 8 words
__global__ void __launch_bounds__(64) k_epoch_blake2s(EpochFields f, int kind, uint32_t nb, const uint64_t* __restrict__ slot_off, const uint32_t* __restrict__ slots,
                                                      uint32_t* __restrict__ digests) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nb) return;
  const uint64_t len = (epoch_encoded_bits(kind, f.key_off[b + 1] - f.key_off[b], f.maxv[b]) + 7) / 8;
  uint32_t h[8];
  epoch_blake2s(slots + slot_off[b], len, h);
#pragma unroll
  for (int i = 0; i < 8; i++) digests[(size_t)b * 8 + i] = h[i];
}
// one lane per proof: two digests -> two canonical inputs; status 1 a spoiled first block, 2 a spoiled last block
__global__ void __launch_bounds__(256) k_epoch_inputs(const uint32_t* __restrict__ dig_first, const uint32_t* __restrict__ dig_last, const uint8_t* __restrict__ st_first,
                                                      const uint8_t* __restrict__ st_last, uint32_t m, uint64_t* __restrict__ inputs, uint8_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  uint32_t a[8], b[8];
  uint64_t o[12];
#pragma unroll
  for (int j = 0; j < 8; j++) { a[j] = dig_first[(size_t)i * 8 + j]; b[j] = dig_last[(size_t)i * 8 + j]; }
  epoch_inputs(a, b, o);
#pragma unroll
  for (int j = 0; j < 12; j++) inputs[(size_t)i * 12 + j] = o[j];
  status[i] = st_first[i] ? 1 : st_last[i] ? 2 : 0;
}
// the slots -> the caller's packed bytes (block b at out_off[b]); one lane per byte
__global__ void __launch_bounds__(256) k_epoch_compact(const uint32_t* __restrict__ slots, const uint64_t* __restrict__ slot_off, const uint64_t* __restrict__ out_off,
                                                       uint32_t nb, uint8_t* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= out_off[nb]) return;
  const uint32_t b = epoch_find_block<uint64_t>(out_off, nb, t);
  const uint64_t j = t - out_off[b];
  out[t] = (uint8_t)(slots[slot_off[b] + j / 4] >> (8 * (j % 4)));
}
__global__ void __launch_bounds__(256) k_epoch_extras(EpochFields f, uint32_t nb, uint8_t* __restrict__ extras) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nb) return;
  uint8_t e[7];
  epoch_extra(f.index[b], f.round[b], f.mns[b], e);
  for (int i = 0; i < 7; i++) extras[(size_t)b * 7 + i] = e[i];
}

// what needs no device: 2 for a refused set of blocks
static int epoch_refuse(const EpochBlocks& b, size_t nb, bool need_round) {
  if (nb > EPOCH_MAX_BLOCKS || !b.index || !b.max_non_signers || !b.max_validators || !b.key_off || (need_round && !b.round)) return 2;
  if (b.keys_form != 0 && b.keys_form != 1) return 2;
  for (size_t i = 0; i < nb; i++) {
    if (b.key_off[i + 1] < b.key_off[i]) return 2;
    if (!epoch_block_ok(b.key_off[i + 1] - b.key_off[i], b.max_validators[i])) return 2;
  }
  if (b.key_off[nb] > 0x7fffffffu || (b.key_off[nb] && !b.keys)) return 2;
  return 0;
}

// the padding generator's record, from the same template the kernel runs
static EpochRecord epoch_generator_record() {
  uint64_t gen[24];
  EpochRecord r;
  Fq::from_limbs(T377::G2_GEN_X0).to_ark(gen); Fq::from_limbs(T377::G2_GEN_X1).to_ark(gen + 6);
  Fq::from_limbs(T377::G2_GEN_Y0).to_ark(gen + 12); Fq::from_limbs(T377::G2_GEN_Y1).to_ark(gen + 18);
  epoch_key_record(gen, false, r.w);
  return r;
}

// CallScope::in for a field the kernels only read
template <class T> static hipError_t epoch_in(CallScope& cs, const T** d, const void* p, size_t bytes, int dev) {
  T* q = nullptr;
  const hipError_t e = cs.in(&q, p, bytes, dev);
  *d = q;
  return e;
}

// one set of nb blocks on the device, up to its records
struct EpochDev {
  EpochFields f = {};
  const uint64_t* rows = nullptr;   // key_off[nb] decoded keys
  const uint8_t* inf = nullptr;     // ... and their flags: the identity, or a key that did not decode
  uint32_t* recs = nullptr;     // key_off[nb] key records, then the generator's
  uint32_t* sums = nullptr;     // nb records: the aggregated keys (with_sums)
  uint8_t* status = nullptr;    // nb
  uint64_t* slot_off = nullptr; // nb + 1, in words
  uint32_t* slots = nullptr;
  uint64_t slot_words = 0;
};

static int epoch_stage(CallScope& cs, EvLog& log, const EpochBlocks& b, size_t nb, int dev, bool with_sums, EpochDev& d) {
  const hipStream_t s = cs.stream();
  const uint32_t nb32 = (uint32_t)nb, nkeys = b.key_off[nb];
  uint64_t* d_rows;
  uint8_t *d_kst = nullptr, *d_inf_in = nullptr, *d_inf;
  hipEvent_t e0 = log.open();
  // the fields that size the call are host arrays in both forms
  HIP_TRY(epoch_in(cs, &d.f.index, b.index, nb * 2, 0), 10);
  HIP_TRY(epoch_in(cs, &d.f.round, b.round, nb, 0), 10);
  HIP_TRY(epoch_in(cs, &d.f.mns, b.max_non_signers, nb * 4, 0), 10);
  HIP_TRY(epoch_in(cs, &d.f.maxv, b.max_validators, nb * 4, 0), 10);
  HIP_TRY(epoch_in(cs, &d.f.key_off, b.key_off, (nb + 1) * 4, 0), 10);
  HIP_TRY(epoch_in(cs, &d.f.ee, b.epoch_entropy, nb * 16, dev), 10);
  HIP_TRY(epoch_in(cs, &d.f.pe, b.parent_entropy, nb * 16, dev), 10);
  HIP_TRY(cs.alloc(&d_inf, (size_t)nkeys + 8), 10);
  HIP_TRY(cs.alloc(&d.status, nb), 10);
  HIP_TRY(cs.alloc(&d.recs, ((size_t)nkeys + 1) * EPOCH_REC_WORDS * 4), 10);
  if (b.keys_form == 0) {
    uint8_t* d_k96 = nullptr;
    if (nkeys) HIP_TRY(cs.in(&d_k96, b.keys, (size_t)nkeys * 96, dev), 10);
    HIP_TRY(cs.alloc(&d_rows, (size_t)nkeys * 192 + 8), 10);
    HIP_TRY(cs.alloc(&d_kst, (size_t)nkeys + 8), 10);
    log.close(EP_XFER, e0);
    e0 = log.open();
    // a validator set changes by a handful of keys per epoch: when the switch says so (celo_amd_key_dedup_set), each distinct key is decoded once
    if (nkeys) {
      const int rc = key_dedup_use(nkeys) ? wire_decompress_dedup(1, d_k96, nkeys, 1, d_rows, d_kst, nullptr, nullptr, 1, s)
                                          : wire_decompress(1, d_k96, nkeys, 1, d_rows, d_kst, 1, s);
      if (rc) return rc;
    }
    log.close(EP_DECODE, e0);
  } else {
    if (nkeys) {
      HIP_TRY(cs.in(&d_rows, b.keys, (size_t)nkeys * 192, dev, 8), 10);
      HIP_TRY(cs.in(&d_inf_in, b.keys_inf, nkeys, dev, 8), 10);
    } else {
      HIP_TRY(cs.alloc(&d_rows, 8), 10);                 // (a pointer for the sums: no row is read)
    }
    log.close(EP_XFER, e0);
  }
  static const EpochRecord grec = epoch_generator_record();
  HIP_TRY(hipMemcpyAsync(d.recs + (size_t)nkeys * EPOCH_REC_WORDS, grec.w, sizeof grec.w, hipMemcpyHostToDevice, s), 10);
  hipLaunchKernelGGL(k_epoch_block_status, dim3((nb32 + 255) / 256), dim3(256), 0, s, d.f.key_off, d_kst, d_inf_in, nb32, d_inf, d.status);
  HIP_TRY(hipGetLastError(), 10);
  d.rows = d_rows;
  d.inf = d_inf;
  uint64_t* d_sum = nullptr;
  uint8_t* d_suminf = nullptr;
  if (with_sums) {
    // the unmasked sum of every block's keys: the masked segmented sums under a bitmap of ones (identity keys and keys that did not decode
    // are flagged, and add nothing)
    uint8_t* d_ones;
    HIP_TRY(cs.alloc(&d_ones, (size_t)nkeys + 8), 10);
    HIP_TRY(cs.alloc(&d_sum, nb * 192), 10);
    HIP_TRY(cs.alloc(&d_suminf, nb), 10);
    HIP_TRY(cs.alloc(&d.sums, nb * EPOCH_REC_WORDS * 4), 10);
    HIP_TRY(hipMemsetAsync(d_ones, 1, (size_t)nkeys + 8, s), 10);
    e0 = log.open();
    if (int rc = aggregate_by_bitmap(1, d_rows, d_inf, b.key_off, nb, d_ones, nb, d_sum, d_suminf, nullptr, 1, s)) return rc;
    log.close(EP_SUMS, e0);
  }
  e0 = log.open();
  if (nkeys) hipLaunchKernelGGL(k_epoch_key_record, dim3((nkeys + 63) / 64), dim3(64), 0, s, d_rows, d_inf, nkeys, d.recs);
  if (with_sums) hipLaunchKernelGGL(k_epoch_key_record, dim3((nb32 + 63) / 64), dim3(64), 0, s, d_sum, d_suminf, nb32, d.sums);
  log.close(EP_PACK, e0);
  HIP_TRY(hipGetLastError(), 10);
  return 0;
}

// the byte streams of kind `kind` into 64-byte-aligned slots
static int epoch_pack(CallScope& cs, EvLog& log, const EpochBlocks& b, size_t nb, int kind, EpochDev& d) {
  const hipStream_t s = cs.stream();
  std::vector<uint64_t> off(nb + 1);
  off[0] = 0;
  for (size_t i = 0; i < nb; i++) {
    const uint64_t bytes = (epoch_encoded_bits(kind, b.key_off[i + 1] - b.key_off[i], b.max_validators[i]) + 7) / 8;
    off[i + 1] = off[i] + (bytes + 63) / 64 * 16;
  }
  d.slot_words = off[nb];
  if (d.slot_words >= (uint64_t(1) << 38)) return 2;       // (2^24 blocks of 2^16 keys: past any device, and past the grid)
  hipEvent_t e0 = log.open();
  HIP_TRY(cs.in(&d.slot_off, off.data(), (nb + 1) * 8, 0), 10);
  HIP_TRY(hipStreamSynchronize(s), 10);                     // (off is a local)
  log.close(EP_XFER, e0);
  HIP_TRY(cs.alloc(&d.slots, d.slot_words * 4), 10);
  e0 = log.open();
  hipLaunchKernelGGL(k_epoch_pack, dim3((unsigned)((d.slot_words + 255) / 256)), dim3(256), 0, s, d.f, kind, (uint32_t)nb, d.slot_off, d.recs, d.sums, d.status, d.slots);
  log.close(EP_PACK, e0);
  HIP_TRY(hipGetLastError(), 10);
  return 0;
}

int epoch_refuse_blocks(const EpochBlocks& b, size_t nb, bool need_round) { return epoch_refuse(b, nb, need_round); }
// host pointers throughout (the caller's frame stages what it adds); no record of its own: the times go to the caller's log
int epoch_stage_bytes(CallScope& cs, EvLog& log, const EpochBlocks& b, size_t nb, int kind, const uint64_t* out_off, EpochStaged* out) {
  EpochDev d;
  if (int rc = epoch_stage(cs, log, b, nb, 0, kind == 1, d)) return rc;
  if (int rc = epoch_pack(cs, log, b, nb, kind, d)) return rc;
  uint64_t* d_out_off;
  uint8_t* d_bytes;
  HIP_TRY(cs.in(&d_out_off, out_off, (nb + 1) * 8, 0), 10);
  HIP_TRY(cs.alloc(&d_bytes, out_off[nb] + 8), 10);
  hipEvent_t e0 = log.open();
  if (out_off[nb]) hipLaunchKernelGGL(k_epoch_compact, dim3((unsigned)((out_off[nb] + 255) / 256)), dim3(256), 0, cs.stream(), d.slots, d.slot_off, d_out_off, (uint32_t)nb, d_bytes);
  log.close(EP_PACK, e0);
  HIP_TRY(hipGetLastError(), 10);
  *out = {d.f.index, d.f.round, d.f.mns, d.f.key_off, d.f.ee, d.f.pe, d.rows, d.inf, d.status, d_bytes};
  return 0;
}

int epoch_encoded_size(int kind, uint64_t n_keys, uint64_t max_validators, uint64_t* bytes) {
  if (!bytes || kind < 0 || kind >= EPOCH_KINDS || n_keys > EPOCH_MAX_KEYS || max_validators > EPOCH_MAX_KEYS) return 2;
  *bytes = (epoch_encoded_bits(kind, (uint32_t)n_keys, (uint32_t)max_validators) + 7) / 8;
  return 0;
}

int epoch_encode_blocks(const EpochBlocks* b, size_t nb, int kind, const uint64_t* out_off, void* out, void* extras, void* status, int dev, void* stream) {
  if (nb == 0) return 0;
  if (!b || kind < 0 || kind >= EPOCH_KINDS || !out_off || !out || !status || (kind == 2 && !extras)) return 2;
  if (int rc = epoch_refuse(*b, nb, kind == 2)) return rc;
  if (out_off[0] != 0) return 2;
  for (size_t i = 0; i < nb; i++)
    if (out_off[i + 1] < out_off[i] || out_off[i + 1] - out_off[i] != (epoch_encoded_bits(kind, b->key_off[i + 1] - b->key_off[i], b->max_validators[i]) + 7) / 8) return 2;
  if (int rc0 = api_enter()) return rc0;
  std::lock_guard<std::mutex> lk(epoch_mu);
  TimedCall call(g_epoch_last, EP_WALL);
  CallScope cs;
  HIP_TRY(cs.open(dev, stream), 10);
  EvLog log(cs.stream());
  const uint32_t nb32 = (uint32_t)nb;
  EpochDev d;
  if (int rc = epoch_stage(cs, log, *b, nb, dev, kind == 1, d)) return rc;
  if (int rc = epoch_pack(cs, log, *b, nb, kind, d)) return rc;
  uint8_t *d_out, *d_extras, *d_status;
  uint64_t* d_out_off;
  HIP_TRY(cs.in(&d_out_off, out_off, (nb + 1) * 8, 0), 10);
  HIP_TRY(cs.out(&d_out, out, out_off[nb], dev), 10);
  HIP_TRY(cs.out(&d_extras, kind == 2 ? extras : nullptr, nb * 7, dev), 10);
  HIP_TRY(cs.out(&d_status, status, nb, dev), 10);
  hipEvent_t e0 = log.open();
  hipLaunchKernelGGL(k_epoch_compact, dim3((unsigned)((out_off[nb] + 255) / 256)), dim3(256), 0, cs.stream(), d.slots, d.slot_off, d_out_off, nb32, d_out);
  if (kind == 2) hipLaunchKernelGGL(k_epoch_extras, dim3((nb32 + 255) / 256), dim3(256), 0, cs.stream(), d.f, nb32, d_extras);
  log.close(EP_PACK, e0);
  HIP_TRY(hipGetLastError(), 10);
  e0 = log.open();
  HIP_TRY(hipMemcpyAsync(d_status, d.status, nb, hipMemcpyDeviceToDevice, cs.stream()), 10);
  HIP_TRY(cs.copy_back(), 10);
  log.close(EP_XFER, e0);
  HIP_TRY(hipStreamSynchronize(cs.stream()), 10);
  log.sum(call.t.ms);
  return 0;
}

// first and last blocks of m proofs -> d_inputs (m x 12 u64) and d_status (m), enqueued on cs.stream()
static int epoch_inputs_stage(CallScope& cs, EvLog& log, const EpochBlocks& first, const EpochBlocks& last, size_t m, int dev, uint64_t* d_inputs, uint8_t* d_status) {
  const hipStream_t s = cs.stream();
  const uint32_t m32 = (uint32_t)m;
  EpochDev df, dl;
  uint32_t* d_dig;
  HIP_TRY(cs.alloc(&d_dig, 2 * m * 32), 10);
  if (int rc = epoch_stage(cs, log, first, m, dev, false, df)) return rc;
  if (int rc = epoch_pack(cs, log, first, m, 0, df)) return rc;
  if (int rc = epoch_stage(cs, log, last, m, dev, true, dl)) return rc;
  if (int rc = epoch_pack(cs, log, last, m, 1, dl)) return rc;
  hipEvent_t e0 = log.open();
  hipLaunchKernelGGL(k_epoch_blake2s, dim3((m32 + 63) / 64), dim3(64), 0, s, df.f, 0, m32, df.slot_off, df.slots, d_dig);
  hipLaunchKernelGGL(k_epoch_blake2s, dim3((m32 + 63) / 64), dim3(64), 0, s, dl.f, 1, m32, dl.slot_off, dl.slots, d_dig + m * 8);
  hipLaunchKernelGGL(k_epoch_inputs, dim3((m32 + 255) / 256), dim3(256), 0, s, d_dig, d_dig + m * 8, df.status, dl.status, m32, d_inputs, d_status);
  log.close(EP_HASH, e0);
  HIP_TRY(hipGetLastError(), 10);
  return 0;
}

int epoch_public_inputs(const EpochBlocks* first, const EpochBlocks* last, size_t m, void* out_inputs, void* out_status, int dev, void* stream) {
  if (m == 0) return 0;
  if (!first || !last || !out_inputs || !out_status) return 2;
  if (int rc = epoch_refuse(*first, m, false)) return rc;
  if (int rc = epoch_refuse(*last, m, false)) return rc;
  if (int rc0 = api_enter()) return rc0;
  std::lock_guard<std::mutex> lk(epoch_mu);
  TimedCall call(g_epoch_last, EP_WALL);
  CallScope cs;
  HIP_TRY(cs.open(dev, stream), 10);
  EvLog log(cs.stream());
  uint64_t* d_inputs;
  uint8_t* d_status;
  HIP_TRY(cs.out(&d_inputs, out_inputs, m * 96, dev), 10);
  HIP_TRY(cs.out(&d_status, out_status, m, dev), 10);
  if (int rc = epoch_inputs_stage(cs, log, *first, *last, m, dev, d_inputs, d_status)) return rc;
  hipEvent_t e0 = log.open();
  HIP_TRY(cs.copy_back(), 10);
  log.close(EP_XFER, e0);
  HIP_TRY(hipStreamSynchronize(cs.stream()), 10);
  log.sum(call.t.ms);
  return 0;
}

int verify_epoch_proofs(const VerifyingKey* vk, const uint8_t* proofs, const EpochBlocks* first, const EpochBlocks* last, size_t m, int mode, const uint32_t* key,
                        uint8_t* out_ok, uint8_t* out_status) {
  if (m == 0) return 0;
  if (!vk || !proofs || !first || !last || !out_ok || (mode != 0 && mode != 1)) return 2;
  if (int rc = epoch_refuse(*first, m, false)) return rc;
  if (int rc = epoch_refuse(*last, m, false)) return rc;
  if (groth16_vk_inputs(vk, 0) != 2) return 2;             // a live BW6-761 handle with exactly the two inputs of the epoch circuit
  if (int rc0 = api_enter()) return rc0;
  std::lock_guard<std::mutex> lk(epoch_mu);
  TimedCall call(g_epoch_last, EP_WALL);
  std::vector<uint8_t> pre(m), refused(m), ok(m);
  CallScope cs;
  HIP_TRY(cs.open(0, nullptr), 10);
  EvLog log(cs.stream());
  uint64_t* d_inputs;
  uint8_t* d_status;
  HIP_TRY(cs.alloc(&d_inputs, m * 96), 10);
  HIP_TRY(cs.alloc(&d_status, m), 10);
  if (int rc = epoch_inputs_stage(cs, log, *first, *last, m, 0, d_inputs, d_status)) return rc;
  hipEvent_t e0 = log.open();
  HIP_TRY(hipMemcpyAsync(pre.data(), d_status, m, hipMemcpyDeviceToHost, cs.stream()), 10);
  log.close(EP_XFER, e0);
  HIP_TRY(hipStreamSynchronize(cs.stream()), 10);          // the verifier runs on a stream of its own
  {
    const WallMs wall_v(&call.t.ms[EP_VERIFY]);
    if (int rc = G16Api<G16Bw6>::verify_staged(vk, proofs, d_inputs, d_status, m, mode, key, ok.data(), refused.data())) return rc;
  }
  log.sum(call.t.ms);
  for (size_t i = 0; i < m; i++) {
    const uint8_t st = pre[i] ? pre[i] : refused[i] ? 3 : ok[i] ? 0 : 4;
    out_ok[i] = st == 0 ? 1 : 0;
    if (out_status) out_status[i] = st;
  }
  return 0;
}

void epoch_last(float ms[8]) {
  const CallTimes t = g_epoch_last.read();
  for (int i = 0; i < 8; i++) ms[i] = t.ms[i];
}

}  // namespace celo
