"""ctypes binding of the gfx950 C-ABI library (include/celo_bls_amd.h).

There is NO CPU fallback: if build/libcelo_bls_amd.so is missing, import of `lib()` raises.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "build", "libcelo_bls_amd.so")

GROUP_ID = {"bls12_377_g1": 0, "bls12_377_g2": 1, "bw6_761_g1": 2, "bw6_761_g2": 2}
# (u64 limbs per affine point, u64 limbs per scalar, u64 limbs of the Jacobian result)
GROUP_SHAPE = {"bls12_377_g1": (12, 4, 18), "bls12_377_g2": (24, 4, 36), "bw6_761_g1": (24, 6, 36), "bw6_761_g2": (24, 6, 36)}

EXPORTS = [
    "celo_amd_init", "celo_amd_use_device", "celo_amd_device_count", "celo_amd_device_name",
    "msm_bls12_377_g1_multi", "msm_bls12_377_g2_multi", "msm_bw6_761_g1_multi", "msm_bw6_761_g2_multi",
    "msm_bls12_377_g1_multi_dev", "msm_bls12_377_g2_multi_dev", "msm_bw6_761_g1_multi_dev", "msm_bw6_761_g2_multi_dev",
    "msm_bls12_377_g1_multi_windows", "msm_bls12_377_g2_multi_windows", "msm_bw6_761_g1_multi_windows", "msm_bw6_761_g2_multi_windows",
    "msm_bls12_377_g1_subgroup_multi_windows", "msm_bls12_377_g2_subgroup_multi_windows",
    "msm_bls12_377_g1_multi_windows_dev", "msm_bls12_377_g2_multi_windows_dev", "msm_bw6_761_g1_multi_windows_dev", "msm_bw6_761_g2_multi_windows_dev",
    "msm_bls12_377_g1_subgroup_multi_windows_dev", "msm_bls12_377_g2_subgroup_multi_windows_dev",
    "msm_bls12_377_g1_window_shard_dev", "msm_bls12_377_g2_window_shard_dev", "msm_bw6_761_window_shard_dev",
    "msm_bls12_377_g1_join_windows", "msm_bls12_377_g2_join_windows", "msm_bw6_761_join_windows",
    "msm_bls12_377_g1_precompute", "msm_bls12_377_g2_precompute", "msm_bw6_761_g1_precompute", "msm_bw6_761_g2_precompute",
    "msm_bls12_377_g1_precompute_dev", "msm_bls12_377_g2_precompute_dev", "msm_bw6_761_g1_precompute_dev", "msm_bw6_761_g2_precompute_dev",
    "msm_bls12_377_g1_fixed", "msm_bls12_377_g2_fixed", "msm_bw6_761_g1_fixed", "msm_bw6_761_g2_fixed",
    "msm_bls12_377_g1_fixed_dev", "msm_bls12_377_g2_fixed_dev", "msm_bw6_761_g1_fixed_dev", "msm_bw6_761_g2_fixed_dev",
    "celo_amd_msm_fixed_release", "celo_amd_msm_fixed_info",
    "groth16_load_key_bw6_761", "groth16_load_key_bls12_377", "groth16_prove_with_key", "groth16_free_key",
    "msm_bls12_377_g1", "msm_bls12_377_g2", "msm_bw6_761_g1", "msm_bw6_761_g2",
    "msm_batch_bls12_377_g1", "msm_batch_bls12_377_g2", "msm_batch_bw6_761_g1", "msm_batch_bw6_761_g2",
    "msm_bls12_377_g1_dev", "msm_bls12_377_g2_dev", "msm_bw6_761_g1_dev", "msm_bw6_761_g2_dev",
    "pairing_product_is_one_bls12_377", "pairing_product_is_one_batch_bls12_377", "celo_amd_pairing_gt_bls12_377",
    "celo_amd_pairing_last_timings", "pairing_product_is_one_bw6_761", "pairing_product_is_one_batch_bw6_761", "celo_amd_pairing_gt_bw6_761",
    "celo_amd_sum_jacobian_bls12_377_g1", "celo_amd_sum_jacobian_bls12_377_g2", "celo_amd_sum_jacobian_bw6_761",
    "celo_amd_msm_last_timings", "celo_amd_msm_set_window_bits", "celo_amd_msm_set_host_chunks", "celo_amd_msm_set_batched_affine", "celo_amd_msm_host_chunk_plan", "celo_amd_host_alloc", "celo_amd_host_free", "celo_amd_ubench_fp", "celo_amd_selftest_accumulate",
    "celo_amd_gen_points_bls12_377_g1_dev", "celo_amd_gen_points_bls12_377_g2_dev", "celo_amd_gen_points_bw6_761_dev",
    "celo_amd_gen_points_grouped_bls12_377_g1_dev", "celo_amd_gen_points_grouped_bls12_377_g2_dev",
    "batch_verify_bls12_377", "batch_verify_bls12_377_dev", "celo_amd_draw_batch_exponents",
    "ntt_bw6_761_fr", "ntt_bw6_761_fr_dev",
    "groth16_witness_map_bw6_761", "groth16_witness_map_bw6_761_dev", "groth16_prove_bw6_761",
    "decompress_bls12_377_g1", "decompress_bls12_377_g2", "decompress_bls12_377_g1_dev", "decompress_bls12_377_g2_dev",
    "decompress_bw6_761_g1", "decompress_bw6_761_g2", "decompress_bw6_761_g1_dev", "decompress_bw6_761_g2_dev",
    "decode_uncompressed_bw6_761_g1", "decode_uncompressed_bw6_761_g2", "groth16_key_layout_bw6_761", "groth16_load_key_bw6_761_serialized",
    "celo_amd_wire761_last_timings",
    "decode_uncompressed_bls12_377_g1", "decode_uncompressed_bls12_377_g2", "decode_uncompressed_bls12_377_g1_dev", "decode_uncompressed_bls12_377_g2_dev",
    "groth16_key_layout_bls12_377", "groth16_load_key_bls12_377_serialized", "groth16_serialized_key_size_bls12_377", "groth16_serialize_key_bls12_377",
    "compress_bls12_377_g1", "compress_bls12_377_g2", "compress_bw6_761", "compress_bls12_377_g1_dev", "compress_bls12_377_g2_dev", "compress_bw6_761_dev",
    "encode_uncompressed_bls12_377_g1", "encode_uncompressed_bls12_377_g2", "encode_uncompressed_bw6_761",
    "encode_uncompressed_bls12_377_g1_dev", "encode_uncompressed_bls12_377_g2_dev", "encode_uncompressed_bw6_761_dev",
    "groth16_serialized_key_size_bw6_761", "groth16_serialize_key_bw6_761", "groth16_serialize_proof_bw6_761",
    "celo_amd_wire_encode_last_ms", "celo_amd_wire_encode_key_timings",
    "normalize_bls12_377_g1", "normalize_bls12_377_g2",
    "fixed_base_mul_bls12_377_g1", "fixed_base_mul_bls12_377_g2", "fixed_base_mul_bw6_761_g1", "fixed_base_mul_bw6_761_g2",
    "fixed_base_mul_bls12_377_g1_dev", "fixed_base_mul_bls12_377_g2_dev", "fixed_base_mul_bw6_761_g1_dev", "fixed_base_mul_bw6_761_g2_dev",
    "normalize_bw6_761_g1", "normalize_bw6_761_g2", "groth16_setup_bw6_761", "groth16_setup_bls12_377",
    "celo_amd_fixed_base_set_window", "celo_amd_setup_last_timings",
    "groth16_r1cs_load_bw6_761", "groth16_r1cs_load_bls12_377", "groth16_r1cs_info", "groth16_r1cs_free", "groth16_r1cs_rows", "groth16_r1cs_rows_dev",
    "groth16_r1cs_check", "groth16_r1cs_qap_at_tau", "groth16_r1cs_qap_at_tau_dev", "groth16_prove_r1cs_with_key", "groth16_setup_r1cs_bw6_761",
    "groth16_setup_r1cs_bls12_377", "celo_amd_r1cs_last_timings",
    "hash_to_g1_direct_bls12_377", "hash_to_g1_composite_bls12_377", "hash_to_g1_cip22_tail_bls12_377", "composite_crh_bls12_377",
    "hash_to_g1_direct_bls12_377_dev", "hash_to_g1_composite_bls12_377_dev", "hash_to_g1_cip22_tail_bls12_377_dev", "composite_crh_bls12_377_dev",
    "celo_amd_hash_last_ms", "celo_amd_hash_last_rounds", "celo_amd_crh_set_lanes", "celo_amd_crh_last_lanes",
    "hash_to_g2_direct_bls12_377", "hash_to_g2_cip22_tail_bls12_377", "hash_to_g2_composite_bls12_377", "hash_to_g2_one_bls12_377",
    "celo_amd_hash_g2_set_lane_budget_log", "celo_amd_hash_g2_last_split",
    "groth16_vk_load_bw6_761", "groth16_vk_load_bw6_761_serialized", "groth16_vk_free", "groth16_verify_batch_bw6_761",
    "groth16_verify_batch_bw6_761_serialized", "celo_amd_groth16_draw_exponents", "celo_amd_groth16_verify_last",
    "groth16_vk_load_bls12_377", "groth16_vk_load_bls12_377_serialized", "groth16_verify_batch_bls12_377", "groth16_verify_batch_bls12_377_serialized",
    "groth16_serialize_proof_bls12_377",
    "scalar_mul_batch_bls12_377_g1", "scalar_mul_batch_bls12_377_g1_subgroup", "scalar_mul_batch_bls12_377_g2", "scalar_mul_batch_bw6_761_g1",
    "scalar_mul_batch_bw6_761_g2", "scalar_mul_batch_bls12_377_g1_dev", "scalar_mul_batch_bls12_377_g1_subgroup_dev", "scalar_mul_batch_bls12_377_g2_dev",
    "scalar_mul_batch_bw6_761_g1_dev", "scalar_mul_batch_bw6_761_g2_dev", "sign_batch_bls12_377",
    "celo_amd_scalar_mul_set_window", "celo_amd_scalar_mul_set_chunk_rows", "celo_amd_scalar_mul_last_ms",
    "aggregate_by_bitmap_bls12_377_g1", "aggregate_by_bitmap_bls12_377_g2", "aggregate_by_bitmap_bls12_377_g1_dev", "aggregate_by_bitmap_bls12_377_g2_dev",
    "verify_aggregated_seals_bls12_377", "celo_amd_aggregate_set_lanes", "celo_amd_aggregate_set_complement", "celo_amd_seals_last",
    "epoch_encoded_size", "epoch_encode_blocks_bls12_377", "epoch_encode_blocks_bls12_377_dev", "epoch_public_inputs_bw6_761", "epoch_public_inputs_bw6_761_dev",
    "verify_epoch_proofs_bw6_761", "celo_amd_epoch_last", "verify_epoch_transitions_bls12_377", "celo_amd_transitions_last",
    "groth16_prove_r1cs_with_key_dev", "hash_to_bits_r1cs_size_bls12_377", "hash_to_bits_r1cs_bls12_377", "hash_to_bits_r1cs_load_bls12_377",
    "hash_to_bits_assignment_bls12_377", "hash_to_bits_assignment_bls12_377_dev", "celo_amd_hash_to_bits_assignment_host",
    "hash_to_bits_public_inputs_bls12_377", "hash_to_bits_public_inputs_bls12_377_dev", "groth16_hash_helper_prove_bls12_377", "celo_amd_hash_helper_last",
    "groth16_vk_load_bls12_377_wide", "groth16_vk_load_bls12_377_wide_serialized", "celo_amd_groth16_set_input_lanes", "celo_amd_groth16_inputs_last",
    "groth16_hash_helper_verify_bls12_377",
    "check_points_bls12_377_g1", "check_points_bls12_377_g2", "check_points_bw6_761_g1", "check_points_bw6_761_g2",
    "check_points_bls12_377_g1_dev", "check_points_bls12_377_g2_dev", "check_points_bw6_761_g1_dev", "check_points_bw6_761_g2_dev",
    "celo_amd_check_points_last_ms", "celo_amd_wire761_set_subgroup_test",
    "decompress_bls12_377_g1_dedup", "decompress_bls12_377_g2_dedup", "decompress_bls12_377_g1_dedup_dev", "decompress_bls12_377_g2_dedup_dev",
    "celo_amd_key_dedup_set", "celo_amd_key_dedup_get", "celo_amd_key_dedup_last",
]

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with __graft_entry__.build() "
                "(make -C celo-bls-snark-rs_amd/csrc). There is no CPU fallback for the MSM/pairing path.")
        _lib = C.CDLL(LIB_PATH)
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _rows(x, width):
    """x as a contiguous (k, width) uint64 array; k may be 0 (a query without rows, an empty h), which reshape(-1, width) refuses."""
    a = np.ascontiguousarray(x, dtype=np.uint64)
    return a.reshape(a.size // width, width)


def init(device=0):
    rc = lib().celo_amd_init(C.c_int(device))
    if rc != 0:
        raise RuntimeError(f"celo_amd_init({device}) failed rc={rc} (no gfx950 device?)")


def use_device(device):
    """Binds the CALLING thread to a device (celo_amd_use_device)."""
    rc = lib().celo_amd_use_device(C.c_int(device))
    if rc != 0:
        raise RuntimeError(f"celo_amd_use_device({device}) failed rc={rc}")


def device_count():
    n = C.c_int(0)
    rc = lib().celo_amd_device_count(C.byref(n))
    if rc != 0:
        raise RuntimeError(f"celo_amd_device_count failed rc={rc} (no gfx950 device?)")
    return n.value


def msm_multi(group, devices, bases_xy, inf, scalars):
    """One MSM sharded by index range over `devices` (list of ordinals, repeats allowed) inside this process; host buffers."""
    A, S, O = GROUP_SHAPE[group]
    bases_xy = np.ascontiguousarray(bases_xy, dtype=np.uint64)
    scalars = np.ascontiguousarray(scalars, dtype=np.uint64)
    n = bases_xy.size // A
    assert bases_xy.size == n * A and scalars.size == n * S, "bases / scalars length mismatch"
    devs = (C.c_int * len(devices))(*devices)
    out = np.zeros(O, dtype=np.uint64)
    rc = getattr(lib(), "msm_" + group + "_multi")(devs, C.c_int(len(devices)), _p(bases_xy), _p(inf), _p(scalars), C.c_size_t(n), _p(out))
    if rc != 0:
        raise RuntimeError(f"msm_{group}_multi failed rc={rc}")
    return out


def msm_multi_dev(group, devices, d_bases, d_infs, d_scalars, n_per):
    """One MSM over shards already resident on their devices: d_bases / d_scalars / d_infs (or None) are lists of integer
    device addresses, n_per the terms per shard."""
    O = GROUP_SHAPE[group][2]
    k = len(devices)
    devs = (C.c_int * k)(*devices)
    pb = (C.c_void_p * k)(*d_bases)
    ps = (C.c_void_p * k)(*d_scalars)
    pi = (C.c_void_p * k)(*[x or 0 for x in d_infs]) if d_infs is not None else None
    np_ = (C.c_size_t * k)(*n_per)
    out = np.zeros(O, dtype=np.uint64)
    rc = getattr(lib(), "msm_" + group + "_multi_dev")(devs, C.c_int(k), pb, pi, ps, np_, _p(out))
    if rc != 0:
        raise RuntimeError(f"msm_{group}_multi_dev failed rc={rc}")
    return out


def msm_multi_windows(group, devices, bases_xy, inf, scalars, subgroup=False):
    """One MSM partitioned by WINDOW over `devices` (repeats allowed): every shard stages all n terms and owns a range of the windows."""
    A, S, O = GROUP_SHAPE[group]
    bases_xy = np.ascontiguousarray(bases_xy, dtype=np.uint64)
    scalars = np.ascontiguousarray(scalars, dtype=np.uint64)
    n = bases_xy.size // A
    assert bases_xy.size == n * A and scalars.size == n * S, "bases / scalars length mismatch"
    devs = (C.c_int * len(devices))(*devices)
    out = np.zeros(O, dtype=np.uint64)
    name = "msm_" + group + ("_subgroup" if subgroup else "") + "_multi_windows"
    rc = getattr(lib(), name)(devs, C.c_int(len(devices)), _p(bases_xy), _p(inf), _p(scalars), C.c_size_t(n), _p(out))
    if rc != 0:
        raise RuntimeError(f"{name} failed rc={rc}")
    return out


def msm_multi_windows_dev(group, devices, d_bases, d_infs, d_scalars, n, subgroup=False):
    """The window partition over replicas already resident on their devices (lists of integer device addresses, n terms each)."""
    O = GROUP_SHAPE[group][2]
    k = len(devices)
    devs = (C.c_int * k)(*devices)
    pb = (C.c_void_p * k)(*d_bases)
    ps = (C.c_void_p * k)(*d_scalars)
    pi = (C.c_void_p * k)(*[x or 0 for x in d_infs]) if d_infs is not None else None
    out = np.zeros(O, dtype=np.uint64)
    name = "msm_" + group + ("_subgroup" if subgroup else "") + "_multi_windows_dev"
    rc = getattr(lib(), name)(devs, C.c_int(k), pb, pi, ps, C.c_size_t(n), _p(out))
    if rc != 0:
        raise RuntimeError(f"{name} failed rc={rc}")
    return out


_SHARD_NAME = {"bls12_377_g1": "bls12_377_g1", "bls12_377_g2": "bls12_377_g2", "bw6_761_g1": "bw6_761", "bw6_761_g2": "bw6_761"}


def msm_window_shard_dev(group, d_bases, d_inf, d_scalars, n, shard, nshards, stream=0, subgroup=False):
    """One rank's share of a window-partitioned MSM (one process per GPU): returns (record, bit_lo); record = X || Y || ZZ || ZZZ in
    arkworks limbs (uint64[4 * A / 2]).  The ranks all-gather the records and join them with join_windows()."""
    A = GROUP_SHAPE[group][0]
    rec = np.zeros(2 * A, dtype=np.uint64)
    bit = C.c_int(0)
    fn = getattr(lib(), "msm_" + _SHARD_NAME[group] + "_window_shard_dev")
    if group.startswith("bw6"):
        rc = fn(C.c_void_p(d_bases), C.c_void_p(d_inf or 0), C.c_void_p(d_scalars), C.c_size_t(n), C.c_int(shard), C.c_int(nshards), _p(rec), C.byref(bit),
                C.c_void_p(stream or 0))
    else:
        rc = fn(C.c_void_p(d_bases), C.c_void_p(d_inf or 0), C.c_void_p(d_scalars), C.c_size_t(n), C.c_int(1 if subgroup else 0), C.c_int(shard), C.c_int(nshards),
                _p(rec), C.byref(bit), C.c_void_p(stream or 0))
    if rc != 0:
        raise RuntimeError(f"msm_{group}_window_shard_dev failed rc={rc}")
    return rec, bit.value


def join_windows(group, records, bit_lo):
    """total = sum_g 2^bit_lo[g] P_g over the shards' records (shard order)."""
    A, _, O = GROUP_SHAPE[group]
    records = np.ascontiguousarray(records, dtype=np.uint64).reshape(-1)
    k = len(bit_lo)
    assert records.size == k * 2 * A
    bits = (C.c_int * k)(*[int(b) for b in bit_lo])
    out = np.zeros(O, dtype=np.uint64)
    rc = getattr(lib(), "msm_" + _SHARD_NAME[group] + "_join_windows")(_p(records), bits, C.c_int(k), _p(out))
    if rc != 0:
        raise RuntimeError(f"msm_{group}_join_windows failed rc={rc}")
    return out


class FixedBase:
    """A key's fixed-base tables (msm_*_precompute): build once, then msm() / msm_dev() for every scalar vector.  window_bits 0 = automatic."""
    def __init__(self, group, bases_xy=None, inf=None, window_bits=0, d_bases=None, d_inf=0, n=None):
        A = GROUP_SHAPE[group][0]
        self.group, self.h = group, C.c_void_p()
        if d_bases is not None:
            rc = getattr(lib(), "msm_" + group + "_precompute_dev")(C.c_void_p(d_bases), C.c_void_p(d_inf or 0), C.c_size_t(n), C.c_int(window_bits), C.byref(self.h))
        else:
            bases_xy = np.ascontiguousarray(bases_xy, dtype=np.uint64)
            n = bases_xy.size // A
            rc = getattr(lib(), "msm_" + group + "_precompute")(_p(bases_xy), _p(inf), C.c_size_t(n), C.c_int(window_bits), C.byref(self.h))
        if rc != 0:
            raise RuntimeError(f"msm_{group}_precompute failed rc={rc}")
        self.n = n

    def info(self):
        n, wb, w, by, ms = C.c_size_t(), C.c_int(), C.c_int(), C.c_size_t(), C.c_float()
        rc = lib().celo_amd_msm_fixed_info(self.h, C.byref(n), C.byref(wb), C.byref(w), C.byref(by), C.byref(ms))
        if rc != 0:
            raise RuntimeError(f"celo_amd_msm_fixed_info failed rc={rc}")
        return {"n": n.value, "window_bits": wb.value, "windows": w.value, "table_bytes": by.value, "build_ms": ms.value}

    def msm(self, scalars):
        S, O = GROUP_SHAPE[self.group][1:]
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64)
        out = np.zeros(O, dtype=np.uint64)
        rc = getattr(lib(), "msm_" + self.group + "_fixed")(self.h, _p(scalars), C.c_size_t(scalars.size // S), _p(out))
        if rc != 0:
            raise RuntimeError(f"msm_{self.group}_fixed failed rc={rc}")
        return out

    def msm_dev(self, d_scalars, n_scalars, stream=0):
        out = np.zeros(GROUP_SHAPE[self.group][2], dtype=np.uint64)
        rc = getattr(lib(), "msm_" + self.group + "_fixed_dev")(self.h, C.c_void_p(d_scalars), C.c_size_t(n_scalars), _p(out), C.c_void_p(stream or 0))
        if rc != 0:
            raise RuntimeError(f"msm_{self.group}_fixed_dev failed rc={rc}")
        return out

    def release(self):
        if self.h:
            lib().celo_amd_msm_fixed_release(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


def msm(group, bases_xy, inf, scalars, subgroup=False):
    """Host-buffer MSM. bases_xy: uint64 [n, A]; inf: uint8 [n] or None; scalars: uint64 [n, S]. Returns Jacobian limbs.
    subgroup=True (bls12_377_g1 / _g2): the bases are vouched to lie in the prime-order group (msm_bls12_377_g1_subgroup / _g2_subgroup: GLV split)."""
    A, S, O = GROUP_SHAPE[group]
    n = int(bases_xy.shape[0]) if bases_xy.ndim == 2 else int(bases_xy.size // A)
    bases_xy = np.ascontiguousarray(bases_xy, dtype=np.uint64)
    scalars = np.ascontiguousarray(scalars, dtype=np.uint64)
    assert bases_xy.size == n * A and scalars.size == n * S, "bases / scalars length mismatch"
    out = np.zeros(O, dtype=np.uint64)
    rc = getattr(lib(), "msm_" + group + ("_subgroup" if subgroup else ""))(_p(bases_xy), _p(inf), _p(scalars), C.c_size_t(n), _p(out))
    if rc != 0:
        raise RuntimeError(f"msm_{group} failed rc={rc}")
    return out


def msm_dev(group, d_bases, d_inf, d_scalars, n, stream=0, subgroup=False):
    """Device-pointer MSM: d_* are integer device addresses (e.g. torch tensor .data_ptr()).  subgroup: as for msm()."""
    O = GROUP_SHAPE[group][2]
    out = np.zeros(O, dtype=np.uint64)
    rc = getattr(lib(), "msm_" + group + ("_subgroup_dev" if subgroup else "_dev"))(C.c_void_p(d_bases), C.c_void_p(d_inf or 0), C.c_void_p(d_scalars),
                                                 C.c_size_t(n), _p(out), C.c_void_p(stream or 0))
    if rc != 0:
        raise RuntimeError(f"msm_{group}_dev failed rc={rc}")
    return out


def msm_timings(group):
    ms = (C.c_float * 5)()
    cfg = (C.c_int * 3)()
    rc = lib().celo_amd_msm_last_timings(C.c_int(GROUP_ID[group]), ms, cfg)
    assert rc == 0
    return {"convert_ms": ms[0], "sort_ms": ms[1], "accumulate_ms": ms[2], "reduce_ms": ms[3], "total_ms": ms[4],
            "window_bits": cfg[0], "windows": cfg[1], "buckets": cfg[2]}


def selftest_accumulate(group, gen_xy, runs=16384, length=24, seed=1, check=2048, chunked=False):
    """The library's own k_accumulate<group> / k_accumulate_chunk<group> against the host replay of the same templates; returns the number of
    runs whose partial sum differs (celo_amd_selftest_accumulate)."""
    gen_xy = np.ascontiguousarray(gen_xy, dtype=np.uint64)
    d = C.c_uint32(0xFFFFFFFF)
    rc = lib().celo_amd_selftest_accumulate(C.c_int(GROUP_ID[group]), _p(gen_xy), C.c_uint32(runs), C.c_uint32(length), C.c_uint32(seed), C.c_uint32(check),
                                            C.c_int(1 if chunked else 0), C.byref(d))
    if rc != 0:
        raise RuntimeError(f"celo_amd_selftest_accumulate failed rc={rc}")
    return d.value


def ubench_fp():
    """The multiplier peaks of this device, measured now (celo_amd_ubench_fp): G products/s for the 377- and 761-bit fields + the loop's clock."""
    out = (C.c_float * 9)()
    rc = lib().celo_amd_ubench_fp(out)
    if rc != 0:
        raise RuntimeError(f"celo_amd_ubench_fp failed rc={rc}")
    return {"fq377_mul_G": out[0], "fq377_sqr_G": out[1], "fq761_mul_G": out[2], "fq761_sqr_G": out[3], "clock_mhz": out[4],
            "kernel_ms": [out[5], out[6], out[7], out[8]]}


def set_batched_affine(on):
    """BW6-761 resident MSMs: 1 = batched-affine tree levels before the XYZZ chain (csrc/msm_ba.h), 0 = the chain alone, -1 = the default.  Process-wide."""
    if lib().celo_amd_msm_set_batched_affine(C.c_int(on)) != 0:
        raise ValueError(f"batched affine {on} not supported")


def set_host_chunks(chunks, head_split=None, tail_split=None):
    """Host-pointer msm(): index chunks of the pipelined transfer (0 = unpipelined, 1 = one chunk, -1 = default) and, optionally, how often the first /
    the last chunk is cut in halves (default: the library's).  Process-wide."""
    if chunks >= 0:
        if head_split is not None:
            chunks |= (head_split + 1) << 8
        if tail_split is not None:
            chunks |= (tail_split + 1) << 12
    rc = lib().celo_amd_msm_set_host_chunks(C.c_int(chunks))
    if rc != 0:
        raise ValueError(f"host chunks {chunks} not supported")


class PinnedArray:
    """A numpy array over page-locked host memory from celo_amd_host_alloc (freed with the object): `.a` is the array."""

    def __init__(self, shape, dtype):
        self.a = None
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self._p = C.c_void_p()
        rc = lib().celo_amd_host_alloc(C.c_size_t(nbytes), C.byref(self._p))
        if rc != 0 or not self._p.value:
            raise MemoryError(f"celo_amd_host_alloc({nbytes}) failed rc={rc}")
        buf = (C.c_uint8 * nbytes).from_address(self._p.value)
        self.a = np.frombuffer(buf, dtype=dtype).reshape(shape)

    def close(self):
        if getattr(self, "_p", None) is not None and self._p.value:
            self.a = None
            lib().celo_amd_host_free(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:                        # noqa: BLE001 (interpreter shutdown)
            pass


def host_chunk_plan(n, chunks, head_split=1, tail_split=0):
    """(cm, [chunk lengths]) of the pipelined host-pointer entry for n terms; None where the entry would not pipeline.  No device call."""
    cm = C.c_uint32(0)
    lens = (C.c_uint32 * 80)()
    k = lib().celo_amd_msm_host_chunk_plan(C.c_uint64(n), C.c_int(chunks), C.c_int(head_split), C.c_int(tail_split), C.byref(cm), lens)
    return None if k < 0 else (cm.value, [lens[i] for i in range(k)])


def set_window_bits(group, c):
    rc = lib().celo_amd_msm_set_window_bits(C.c_int(GROUP_ID[group]), C.c_int(c))
    if rc != 0:
        raise ValueError(f"window bits {c} not supported")


def gen_points_dev(group, d_out, n, seed, gen_xy, stream=0):
    name = {"bls12_377_g1": "celo_amd_gen_points_bls12_377_g1_dev", "bls12_377_g2": "celo_amd_gen_points_bls12_377_g2_dev",
            "bw6_761_g1": "celo_amd_gen_points_bw6_761_dev", "bw6_761_g2": "celo_amd_gen_points_bw6_761_dev"}[group]
    gen_xy = np.ascontiguousarray(gen_xy, dtype=np.uint64)
    rc = getattr(lib(), name)(C.c_void_p(d_out), C.c_size_t(n), C.c_uint64(seed), _p(gen_xy), C.c_void_p(stream or 0))
    if rc != 0:
        raise RuntimeError(f"{name} failed rc={rc}")


def gen_points_grouped_dev(group, d_out, n, seed, gens_xy, per, stream=0):
    """P_i = k_i * gens[i // per] into device memory (celo_amd_gen_points_grouped_*): gens_xy (ngens, A) uint64 host limbs."""
    name = {"bls12_377_g1": "celo_amd_gen_points_grouped_bls12_377_g1_dev", "bls12_377_g2": "celo_amd_gen_points_grouped_bls12_377_g2_dev"}[group]
    A = GROUP_SHAPE[group][0]
    gens_xy = np.ascontiguousarray(gens_xy, dtype=np.uint64).reshape(-1, A)
    rc = getattr(lib(), name)(C.c_void_p(d_out), C.c_size_t(n), C.c_uint64(seed), _p(gens_xy), C.c_size_t(gens_xy.shape[0]), C.c_uint32(per),
                              C.c_void_p(stream or 0))
    if rc != 0:
        raise RuntimeError(f"{name} failed rc={rc}")


def batch_verify(pk_xy, sig_xy, exponents, offsets, hash_xy, neg_g2_xy):
    """Batch::verify for m batches, host buffers (batch_verify_bls12_377).  Returns uint8 [m] verdicts."""
    pk_xy = np.ascontiguousarray(pk_xy, dtype=np.uint64)
    sig_xy = np.ascontiguousarray(sig_xy, dtype=np.uint64)
    exponents = np.ascontiguousarray(exponents, dtype=np.uint64)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
    hash_xy = np.ascontiguousarray(hash_xy, dtype=np.uint64)
    ng2 = np.ascontiguousarray(neg_g2_xy, dtype=np.uint64).reshape(24)
    m = offsets.size - 1
    tot = int(offsets[-1])
    assert pk_xy.size == tot * 24 and sig_xy.size == tot * 12 and exponents.size == tot * 4 and hash_xy.size == m * 12
    out = np.zeros(m, dtype=np.uint8)
    rc = lib().batch_verify_bls12_377(_p(pk_xy), None, _p(sig_xy), None, _p(exponents), _p(offsets), _p(hash_xy), None, _p(ng2), C.c_size_t(m), _p(out))
    if rc != 0:
        raise RuntimeError(f"batch_verify_bls12_377 failed rc={rc}")
    return out


def batch_verify_dev(d_pk, d_sig, d_exp, offsets, d_hash, neg_g2_xy):
    """The same on inputs resident in HBM (integer device addresses); offsets: host uint32 [m+1]."""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
    ng2 = np.ascontiguousarray(neg_g2_xy, dtype=np.uint64).reshape(24)
    m = offsets.size - 1
    out = np.zeros(m, dtype=np.uint8)
    rc = lib().batch_verify_bls12_377_dev(C.c_void_p(d_pk), None, C.c_void_p(d_sig), None, C.c_void_p(d_exp), _p(offsets), C.c_void_p(d_hash), None, _p(ng2),
                                          C.c_size_t(m), _p(out))
    if rc != 0:
        raise RuntimeError(f"batch_verify_bls12_377_dev failed rc={rc}")
    return out


def draw_batch_exponents(key, offsets):
    """The exponents batch_verify_strict's device kernel draws for one call under `key` (8 uint32): uint64 [offsets[-1], 4]."""
    key = np.ascontiguousarray(key, dtype=np.uint32).reshape(8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
    m = offsets.size - 1
    out = np.zeros((int(offsets[-1]), 4), dtype=np.uint64)
    rc = lib().celo_amd_draw_batch_exponents(_p(key), _p(offsets), C.c_size_t(m), _p(out))
    if rc != 0:
        raise RuntimeError(f"celo_amd_draw_batch_exponents failed rc={rc}")
    return out


def sum_jacobian(group, jac):
    """Plain sum of k Jacobian points (uint64 [k, O]) -> Jacobian limbs."""
    O = GROUP_SHAPE[group][2]
    jac = np.ascontiguousarray(jac, dtype=np.uint64).reshape(-1, O)
    out = np.zeros(O, dtype=np.uint64)
    name = {"bls12_377_g1": "celo_amd_sum_jacobian_bls12_377_g1", "bls12_377_g2": "celo_amd_sum_jacobian_bls12_377_g2",
            "bw6_761_g1": "celo_amd_sum_jacobian_bw6_761", "bw6_761_g2": "celo_amd_sum_jacobian_bw6_761"}[group]
    rc = getattr(lib(), name)(_p(jac), C.c_size_t(jac.shape[0]), _p(out))
    if rc != 0:
        raise RuntimeError(f"{name} failed rc={rc}")
    return out


def pairing_product_is_one(g1_xy, inf1, g2_xy, inf2):
    """One product of k pairings == 1 ?  g1_xy uint64 [k,12], g2_xy uint64 [k,24]."""
    g1_xy = np.ascontiguousarray(g1_xy, dtype=np.uint64)
    g2_xy = np.ascontiguousarray(g2_xy, dtype=np.uint64)
    k = g1_xy.size // 12
    one = C.c_int(0)
    rc = lib().pairing_product_is_one_bls12_377(_p(g1_xy), _p(inf1), _p(g2_xy), _p(inf2), C.c_size_t(k), C.byref(one))
    if rc != 0:
        raise RuntimeError(f"pairing_product_is_one_bls12_377 failed rc={rc}")
    return bool(one.value)


def pairing_product_is_one_batch(g1_xy, inf1, g2_xy, inf2, offsets):
    """m independent products; offsets uint32 [m+1]. Returns uint8 [m]."""
    g1_xy = np.ascontiguousarray(g1_xy, dtype=np.uint64)
    g2_xy = np.ascontiguousarray(g2_xy, dtype=np.uint64)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
    m = offsets.size - 1
    out = np.zeros(m, dtype=np.uint8)
    rc = lib().pairing_product_is_one_batch_bls12_377(_p(g1_xy), _p(inf1), _p(g2_xy), _p(inf2), _p(offsets), C.c_size_t(m), _p(out))
    if rc != 0:
        raise RuntimeError(f"pairing_product_is_one_batch_bls12_377 failed rc={rc}")
    return out


def pairing_gt(g1_xy, inf1, g2_xy, inf2, offsets, miller_only=False):
    g1_xy = np.ascontiguousarray(g1_xy, dtype=np.uint64)
    g2_xy = np.ascontiguousarray(g2_xy, dtype=np.uint64)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
    m = offsets.size - 1
    out = np.zeros((m, 72), dtype=np.uint64)
    rc = lib().celo_amd_pairing_gt_bls12_377(_p(g1_xy), _p(inf1), _p(g2_xy), _p(inf2), _p(offsets), C.c_size_t(m),
                                             C.c_int(1 if miller_only else 0), _p(out))
    if rc != 0:
        raise RuntimeError(f"celo_amd_pairing_gt_bls12_377 failed rc={rc}")
    return out


def ntt(data, log_n, omega6, coset6=None, coset_after=False, scale6=None):
    """In-place NTT over Fr(BW6-761) on HOST data: (n, 6) uint64 arkworks Montgomery limbs; omega6 / coset6 / scale6: (6,) uint64
    Montgomery limbs.  Returns the transformed array (a copy)."""
    out = np.ascontiguousarray(data, dtype=np.uint64).copy()
    assert out.shape == (1 << log_n, 6)
    w = np.ascontiguousarray(omega6, dtype=np.uint64)
    g = None if coset6 is None else np.ascontiguousarray(coset6, dtype=np.uint64)
    sc = None if scale6 is None else np.ascontiguousarray(scale6, dtype=np.uint64)
    rc = lib().ntt_bw6_761_fr(_p(out), C.c_uint(log_n), _p(w), _p(g), C.c_int(1 if coset_after else 0), _p(sc))
    if rc != 0:
        raise RuntimeError("ntt_bw6_761_fr failed with code %d" % rc)
    return out


def ntt_dev(d_ptr, log_n, omega6, coset6=None, coset_after=False, scale6=None, stream=0):
    w = np.ascontiguousarray(omega6, dtype=np.uint64)
    g = None if coset6 is None else np.ascontiguousarray(coset6, dtype=np.uint64)
    sc = None if scale6 is None else np.ascontiguousarray(scale6, dtype=np.uint64)
    rc = lib().ntt_bw6_761_fr_dev(C.c_void_p(d_ptr), C.c_uint(log_n), _p(w), _p(g), C.c_int(1 if coset_after else 0), _p(sc), C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError("ntt_bw6_761_fr_dev failed with code %d" % rc)


def witness_map(a, b, c, log_n, consts, canonical=False):
    """R1CStoQAP::witness_map from the QAP evaluations (groth16_witness_map_bw6_761).  a, b, c: (n, 6) uint64 arkworks Montgomery
    limbs (copied); consts: dict of (6,) uint64 Montgomery limbs: omega, omega_inv, coset, coset_inv, size_inv, vanishing_inv.
    Returns h (n, 6): field elements, or canonical integers with canonical=True."""
    bufs = [np.ascontiguousarray(x, dtype=np.uint64).copy() for x in (a, b, c)]
    assert all(x.shape == (1 << log_n, 6) for x in bufs)
    k = [np.ascontiguousarray(consts[n], dtype=np.uint64) for n in ("omega", "omega_inv", "coset", "coset_inv", "size_inv", "vanishing_inv")]
    rc = lib().groth16_witness_map_bw6_761(_p(bufs[0]), _p(bufs[1]), _p(bufs[2]), C.c_uint(log_n), *[_p(x) for x in k], C.c_int(1 if canonical else 0))
    if rc != 0:
        raise RuntimeError("groth16_witness_map_bw6_761 failed with code %d" % rc)
    return bufs[0]


def witness_map_dev(d_a, d_b, d_c, log_n, consts, canonical=False, stream=0):
    k = [np.ascontiguousarray(consts[n], dtype=np.uint64) for n in ("omega", "omega_inv", "coset", "coset_inv", "size_inv", "vanishing_inv")]
    rc = lib().groth16_witness_map_bw6_761_dev(C.c_void_p(d_a), C.c_void_p(d_b), C.c_void_p(d_c), C.c_uint(log_n), *[_p(x) for x in k],
                                               C.c_int(1 if canonical else 0), C.c_void_p(stream or 0))
    if rc != 0:
        raise RuntimeError("groth16_witness_map_bw6_761_dev failed with code %d" % rc)


def groth16_prove(a_query, b_g2_query, h_query, l_query, alpha_g1, beta_g2, assignment, n_aux, h):
    """create_proof_no_zk's group arithmetic (groth16_prove_bw6_761).  queries: (k, 24) uint64; alpha / beta: (24,); assignment,
    h: (k, 6) uint64 canonical scalars.  Returns (A, B, C) Jacobian limbs (36 u64 each)."""
    arrs = [_rows(x, 24) for x in (a_query, b_g2_query, h_query, l_query)]
    al, be = (np.ascontiguousarray(x, dtype=np.uint64).reshape(24) for x in (alpha_g1, beta_g2))
    asg, hh = _rows(assignment, 6), _rows(h, 6)
    out = [np.zeros(36, dtype=np.uint64) for _ in range(3)]
    rc = lib().groth16_prove_bw6_761(_p(arrs[0]), C.c_size_t(arrs[0].shape[0]), _p(arrs[1]), C.c_size_t(arrs[1].shape[0]), _p(arrs[2]), C.c_size_t(arrs[2].shape[0]),
                                     _p(arrs[3]), C.c_size_t(arrs[3].shape[0]), _p(al), _p(be), _p(asg), C.c_size_t(asg.shape[0]), C.c_size_t(n_aux),
                                     _p(hh), C.c_size_t(hh.shape[0]), _p(out[0]), _p(out[1]), _p(out[2]))
    if rc != 0:
        raise RuntimeError("groth16_prove_bw6_761 failed with code %d" % rc)
    return out


# groth16_key_layout_<curve> / groth16_load_key_<curve>_serialized (include/celo_bls_amd.h)
KEY_ERR_TRUNCATED, KEY_ERR_TRAILING, KEY_ERR_LENGTH, KEY_ERR_POINT = 30, 31, 32, 33
KEY_LAYOUT_SLOTS = {"point_bytes": 0, "len": 1, "gamma_abc_g1": 2, "a_query": 4, "b_g1_query": 6, "b_g2_query": 8, "h_query": 10, "l_query": 12}


class KeyLoadError(RuntimeError):
    def __init__(self, code, first_bad_point=None, curve="bw6_761"):
        super().__init__("groth16_load_key_%s_serialized failed with code %d%s"
                         % (curve, code, "" if first_bad_point is None else " (first rejected point: %d)" % first_bad_point))
        self.code = code
        self.first_bad_point = first_bad_point


def groth16_key_layout(data, form=0, curve="bw6_761"):
    """Host walk of a serialized ProvingKey of `curve` ("bw6_761" / "bls12_377": groth16_key_layout_<curve>): returns (rc, out) with out the
    16 u64 of the header ({section: (count, byte offset)} via KEY_LAYOUT_SLOTS; out[0] the bytes of a G1 point - a BLS12-377 G2 point has
    twice as many -, out[14] the offset of beta_g1, out[15] the number of points)."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    out = np.zeros(16, dtype=np.uint64)
    rc = getattr(lib(), "groth16_key_layout_" + curve)(_p(buf), C.c_size_t(buf.size), C.c_int(form), _p(out))
    return rc, out


class ProvingKey:
    """A loaded Groth16 proving key (groth16_load_key_bw6_761 / _bls12_377): the four queries' fixed-base tables, built once; prove() per
    assignment.  curve: "bw6_761" (points (k, 24), scalars (k, 6)) or "bls12_377" (G1 (k, 12), G2 (k, 24), scalars (k, 4))."""
    def __init__(self, curve, a_query, b_g2_query, h_query, l_query, alpha_g1, beta_g2, window_bits=0):
        self.curve = curve
        g1w = 24 if curve == "bw6_761" else 12
        self.sw = 6 if curve == "bw6_761" else 4
        self.ow = (36, 36, 36) if curve == "bw6_761" else (18, 36, 18)
        self.h = C.c_void_p()
        if a_query is None:                 # from_serialized fills the handle
            return
        q = [_rows(a_query, g1w), _rows(b_g2_query, 24), _rows(h_query, g1w), _rows(l_query, g1w)]
        al = np.ascontiguousarray(alpha_g1, dtype=np.uint64).reshape(g1w)
        be = np.ascontiguousarray(beta_g2, dtype=np.uint64).reshape(24)
        fn = lib().groth16_load_key_bw6_761 if curve == "bw6_761" else lib().groth16_load_key_bls12_377
        rc = fn(_p(q[0]), C.c_size_t(q[0].shape[0]), _p(q[1]), C.c_size_t(q[1].shape[0]), _p(q[2]), C.c_size_t(q[2].shape[0]), _p(q[3]), C.c_size_t(q[3].shape[0]),
                _p(al), _p(be), C.c_int(window_bits), C.byref(self.h))
        if rc != 0:
            raise RuntimeError("groth16_load_key_%s failed with code %d" % (curve, rc))

    @classmethod
    def from_serialized(cls, data, form=0, window_bits=0, curve="bw6_761"):
        """A key of `curve` ("bw6_761" / "bls12_377") from the bytes of a serialized ark-groth16 0.1 ProvingKey (groth16_load_key_<curve>_serialized):
        form 0 = compressed, checked; 1 = uncompressed, checked; 2 = uncompressed, unchecked.  Raises KeyLoadError (.code, .first_bad_point)."""
        k = cls(curve, None, None, None, None, None, None)
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        bad = C.c_uint64(0)
        rc = getattr(lib(), "groth16_load_key_%s_serialized" % curve)(_p(buf), C.c_size_t(buf.size), C.c_int(form), C.c_int(window_bits), C.byref(k.h), C.byref(bad))
        if rc != 0:
            k.h = C.c_void_p()
            raise KeyLoadError(rc, bad.value if rc == KEY_ERR_POINT else None, curve)
        return k

    def prove_r1cs(self, r1cs, z, log_n, consts):
        """matrices + assignment -> proof (groth16_prove_r1cs_with_key): r1cs an R1CS of this key's curve; z (n_vars, 6 | 4) Montgomery limbs of the
        full assignment (z[0] = 1); consts as for witness_map.  Returns (A, B, C) Jacobian limbs as prove() does."""
        zz = np.ascontiguousarray(z, dtype=np.uint64).reshape(-1, self.sw)
        assert zz.shape[0] == r1cs.n_vars
        k = [np.ascontiguousarray(consts[n], dtype=np.uint64).reshape(self.sw) for n in ("omega", "omega_inv", "coset", "coset_inv", "size_inv", "vanishing_inv")]
        out = [np.zeros(w, dtype=np.uint64) for w in self.ow]
        rc = lib().groth16_prove_r1cs_with_key(self.h, r1cs.h, _p(zz), C.c_uint(log_n), *[_p(x) for x in k], _p(out[0]), _p(out[1]), _p(out[2]))
        if rc != 0:
            raise RuntimeError("groth16_prove_r1cs_with_key failed with code %d" % rc)
        return out

    def prove_r1cs_dev(self, r1cs, d_z, log_n, consts):
        """prove_r1cs with z on the DEVICE (groth16_prove_r1cs_with_key_dev): d_z the address of n_vars rows, complete before the call"""
        k = [np.ascontiguousarray(consts[n], dtype=np.uint64).reshape(self.sw) for n in ("omega", "omega_inv", "coset", "coset_inv", "size_inv", "vanishing_inv")]
        out = [np.zeros(w, dtype=np.uint64) for w in self.ow]
        rc = lib().groth16_prove_r1cs_with_key_dev(self.h, r1cs.h, C.c_void_p(d_z), C.c_uint(log_n), *[_p(x) for x in k], _p(out[0]), _p(out[1]), _p(out[2]))
        if rc != 0:
            raise RuntimeError("groth16_prove_r1cs_with_key_dev failed with code %d" % rc)
        return out

    def prove(self, assignment, n_aux, h):
        asg, hh = _rows(assignment, self.sw), _rows(h, self.sw)
        out = [np.zeros(w, dtype=np.uint64) for w in self.ow]
        rc = lib().groth16_prove_with_key(self.h, _p(asg), C.c_size_t(asg.shape[0]), C.c_size_t(n_aux), _p(hh), C.c_size_t(hh.shape[0]), _p(out[0]), _p(out[1]), _p(out[2]))
        if rc != 0:
            raise RuntimeError("groth16_prove_with_key failed with code %d" % rc)
        return out

    def release(self):
        if self.h:
            lib().groth16_free_key(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class VerifyError(RuntimeError):
    def __init__(self, what, code):
        super().__init__("%s failed with code %d" % (what, code))
        self.code = code


VERIFY_PATHS = {0: "each", 1: "combined accepted", 2: "combined then each"}
VK_ERR_INPUTS = 36
VK_WIDE_INPUTS = 1024                   # the most public inputs of a wide BLS12-377 key (csrc/groth16_verify.h G16_MAX_INPUTS_WIDE)
G16_INPUT_LANES = (1, 2, 4, 8, 16, 32, 64, 128, 256)   # the widths celo_amd_groth16_set_input_lanes accepts besides 0


# per curve of the verifier: u64 of a G1 / G2 row, of one input, bytes of a compressed G1 / G2 point
VERIFY_CURVES = {"bw6_761": (24, 24, 6, 96, 96), "bls12_377": (12, 24, 4, 48, 96)}


class VerifyingKey:
    """A loaded Groth16 verifying key over BW6-761 or BLS12-377 (groth16_vk_load_<curve>): verify() checks m proofs under it in one call.
    alpha_g1 and the rows of gamma_abc_g1 (n_abc of them): 24 u64 each over BW6-761, 12 over BLS12-377; beta_g2 / gamma_g2 / delta_g2: 24 u64;
    affine arkworks limbs.  wide (BLS12-377 only): the loaders that take up to VK_WIDE_INPUTS public inputs where the others stop at 64.
    Raises VerifyError (.code)."""
    def __init__(self, alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1, curve="bw6_761", wide=False):
        assert not wide or curve == "bls12_377", "wide keys: BLS12-377 only"
        self.h = C.c_void_p()
        self.curve = curve
        self._load = "groth16_vk_load_" + curve + ("_wide" if wide else "")
        self.w1, self.w2, self.n64, b1, b2 = VERIFY_CURVES[curve]
        self.proof_bytes, self.key_head = 2 * b1 + b2, b1 + 3 * b2
        if alpha_g1 is None:                # from_serialized fills the handle
            return
        pts = [np.ascontiguousarray(x, dtype=np.uint64).reshape(w) for x, w in zip((alpha_g1, beta_g2, gamma_g2, delta_g2), (self.w1, self.w2, self.w2, self.w2))]
        abc = _rows(gamma_abc_g1, self.w1)
        self.n_inputs = abc.shape[0] - 1
        rc = getattr(lib(), self._load)(*[_p(x) for x in pts], _p(abc), C.c_size_t(abc.shape[0]), C.byref(self.h))
        if rc != 0:
            self.h = C.c_void_p()
            raise VerifyError(self._load, rc)

    @classmethod
    def from_serialized(cls, data, curve="bw6_761", wide=False):
        """from VerifyingKey::serialize bytes (compressed; decoded and checked as VerifyingKey::deserialize does)"""
        k = cls(None, None, None, None, None, curve=curve, wide=wide)
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        rc = getattr(lib(), k._load + "_serialized")(_p(buf), C.c_size_t(buf.size), C.byref(k.h))
        if rc != 0:
            k.h = C.c_void_p()
            raise VerifyError(k._load + "_serialized", rc)
        k.n_inputs = int.from_bytes(bytes(data)[k.key_head:k.key_head + 8], "little") - 1
        return k

    def _inputs(self, inputs, m):
        if self.n_inputs == 0:
            return None
        x = np.ascontiguousarray(inputs, dtype=np.uint64)
        assert x.size == m * self.n_inputs * self.n64, "inputs: m x n_inputs x %d canonical u64" % self.n64
        return x

    def verify(self, a_xy, b_xy, c_xy, inputs, mode=0, key=None, a_inf=None, b_inf=None, c_inf=None):
        """m proofs as rows of A, B, C (BW6-761: (m, 24) each; BLS12-377: (m, 12), (m, 24), (m, 12)) and inputs (m, n_inputs, 6 or 4)
        canonical integers -> uint8 [m] verdicts.  mode 0: each; 1: combined (A, C in G1 and B in G2 required), key: 8 uint32 for the
        exponent stream or None for the operating system's."""
        a, b, c = _rows(a_xy, self.w1), _rows(b_xy, self.w2), _rows(c_xy, self.w1)
        m = a.shape[0]
        assert b.shape[0] == m and c.shape[0] == m
        x = self._inputs(inputs, m)
        flags = [None if f is None else np.ascontiguousarray(f, dtype=np.uint8) for f in (a_inf, b_inf, c_inf)]
        k = None if key is None else np.ascontiguousarray(key, dtype=np.uint32).reshape(8)
        out = np.zeros(m, dtype=np.uint8)
        rc = getattr(lib(), "groth16_verify_batch_" + self.curve)(self.h, _p(a), _p(flags[0]), _p(b), _p(flags[1]), _p(c), _p(flags[2]), _p(x), C.c_size_t(m), C.c_int(mode),
                                                                  _p(k), _p(out))
        if rc != 0:
            raise VerifyError("groth16_verify_batch_" + self.curve, rc)
        return out

    def verify_serialized(self, proofs, inputs, mode=0, key=None):
        """m proofs as m x 288 bytes (BLS12-377: m x 192; Proof::serialize: A | B | C compressed), decoded and checked on the device"""
        buf = np.frombuffer(bytes(proofs), dtype=np.uint8)
        assert buf.size % self.proof_bytes == 0
        m = buf.size // self.proof_bytes
        x = self._inputs(inputs, m)
        k = None if key is None else np.ascontiguousarray(key, dtype=np.uint32).reshape(8)
        out = np.zeros(m, dtype=np.uint8)
        rc = getattr(lib(), "groth16_verify_batch_%s_serialized" % self.curve)(self.h, _p(buf), _p(x), C.c_size_t(m), C.c_int(mode), _p(k), _p(out))
        if rc != 0:
            raise VerifyError("groth16_verify_batch_%s_serialized" % self.curve, rc)
        return out

    def release(self):
        if self.h:
            rc = lib().groth16_vk_free(self.h)
            self.h = C.c_void_p()
            return rc
        return 0

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


def groth16_draw_exponents(key, m):
    """The exponents a combined verify call under `key` (8 uint32) gives its m proofs (celo_amd_groth16_draw_exponents): uint64 [m, 2]."""
    key = np.ascontiguousarray(key, dtype=np.uint32).reshape(8)
    out = np.zeros((m, 2), dtype=np.uint64)
    rc = lib().celo_amd_groth16_draw_exponents(_p(key), C.c_size_t(m), _p(out))
    if rc != 0:
        raise RuntimeError(f"celo_amd_groth16_draw_exponents failed rc={rc}")
    return out


def groth16_verify_last():
    """(path name, window bits, ms[8]) of the last verify call (celo_amd_groth16_verify_last)"""
    path, c = C.c_int(-1), C.c_int(0)
    ms = (C.c_float * 8)()
    lib().celo_amd_groth16_verify_last(C.byref(path), C.byref(c), ms)
    return VERIFY_PATHS.get(path.value, "none"), c.value, list(ms)


def groth16_set_input_lanes(lanes):
    """Lanes per input sum of every later BLS12-377 verify call (celo_amd_groth16_set_input_lanes): 0 = the rule, else one of G16_INPUT_LANES.
    A test and tuning switch; no device call."""
    rc = lib().celo_amd_groth16_set_input_lanes(C.c_int(lanes))
    if rc != 0:
        raise ValueError("celo_amd_groth16_set_input_lanes(%d) failed with code %d" % (lanes, rc))


def groth16_inputs_last():
    """(lanes per input sum, public inputs of the key) of the last verify call (celo_amd_groth16_inputs_last)"""
    lanes, n_in = C.c_int(0), C.c_int(0)
    assert lib().celo_amd_groth16_inputs_last(C.byref(lanes), C.byref(n_in)) == 0
    return lanes.value, n_in.value


# ---- the hash-helper proof's field and curve: Fr(BLS12-377) elements are 4 u64, G1 points 12 u64 affine / 18 Jacobian, G2 24 / 36
def ntt_fr377(data, log_n, omega4, coset4=None, coset_after=False, scale4=None):
    """In-place NTT over Fr(BLS12-377) on HOST data (ntt_bls12_377_fr): (n, 4) uint64 arkworks Montgomery limbs.  Returns a copy."""
    out = np.ascontiguousarray(data, dtype=np.uint64).copy()
    assert out.shape == (1 << log_n, 4)
    w = np.ascontiguousarray(omega4, dtype=np.uint64)
    g = None if coset4 is None else np.ascontiguousarray(coset4, dtype=np.uint64)
    sc = None if scale4 is None else np.ascontiguousarray(scale4, dtype=np.uint64)
    rc = lib().ntt_bls12_377_fr(_p(out), C.c_uint(log_n), _p(w), _p(g), C.c_int(1 if coset_after else 0), _p(sc))
    if rc != 0:
        raise RuntimeError("ntt_bls12_377_fr failed with code %d" % rc)
    return out


def ntt_fr377_dev(d_ptr, log_n, omega4, coset4=None, coset_after=False, scale4=None, stream=0):
    w = np.ascontiguousarray(omega4, dtype=np.uint64)
    g = None if coset4 is None else np.ascontiguousarray(coset4, dtype=np.uint64)
    sc = None if scale4 is None else np.ascontiguousarray(scale4, dtype=np.uint64)
    rc = lib().ntt_bls12_377_fr_dev(C.c_void_p(d_ptr), C.c_uint(log_n), _p(w), _p(g), C.c_int(1 if coset_after else 0), _p(sc), C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError("ntt_bls12_377_fr_dev failed with code %d" % rc)


def witness_map_fr377(a, b, c, log_n, consts, canonical=False):
    """groth16_witness_map_bls12_377: a, b, c (n, 4) uint64 Montgomery limbs (copied); consts as for witness_map, (4,) limbs each."""
    bufs = [np.ascontiguousarray(x, dtype=np.uint64).copy() for x in (a, b, c)]
    assert all(x.shape == (1 << log_n, 4) for x in bufs)
    k = [np.ascontiguousarray(consts[n], dtype=np.uint64) for n in ("omega", "omega_inv", "coset", "coset_inv", "size_inv", "vanishing_inv")]
    rc = lib().groth16_witness_map_bls12_377(_p(bufs[0]), _p(bufs[1]), _p(bufs[2]), C.c_uint(log_n), *[_p(x) for x in k], C.c_int(1 if canonical else 0))
    if rc != 0:
        raise RuntimeError("groth16_witness_map_bls12_377 failed with code %d" % rc)
    return bufs[0]


def witness_map_fr377_dev(d_a, d_b, d_c, log_n, consts, canonical=False, stream=0):
    k = [np.ascontiguousarray(consts[n], dtype=np.uint64) for n in ("omega", "omega_inv", "coset", "coset_inv", "size_inv", "vanishing_inv")]
    rc = lib().groth16_witness_map_bls12_377_dev(C.c_void_p(d_a), C.c_void_p(d_b), C.c_void_p(d_c), C.c_uint(log_n), *[_p(x) for x in k],
                                                 C.c_int(1 if canonical else 0), C.c_void_p(stream or 0))
    if rc != 0:
        raise RuntimeError("groth16_witness_map_bls12_377_dev failed with code %d" % rc)


def groth16_prove_bls12_377(a_query, b_g2_query, h_query, l_query, alpha_g1, beta_g2, assignment, n_aux, h):
    """create_proof_no_zk's group arithmetic over BLS12-377 (groth16_prove_bls12_377).  a / h / l queries: (k, 12) uint64, b_g2_query:
    (k, 24); alpha (12,), beta (24,); assignment, h: (k, 4) canonical scalars.  Returns (A (18,), B (36,), C (18,)) Jacobian limbs."""
    aq, hq, lq = (_rows(x, 12) for x in (a_query, h_query, l_query))
    bq = _rows(b_g2_query, 24)
    al = np.ascontiguousarray(alpha_g1, dtype=np.uint64).reshape(12)
    be = np.ascontiguousarray(beta_g2, dtype=np.uint64).reshape(24)
    asg, hh = _rows(assignment, 4), _rows(h, 4)
    out = [np.zeros(18, dtype=np.uint64), np.zeros(36, dtype=np.uint64), np.zeros(18, dtype=np.uint64)]
    rc = lib().groth16_prove_bls12_377(_p(aq), C.c_size_t(aq.shape[0]), _p(bq), C.c_size_t(bq.shape[0]), _p(hq), C.c_size_t(hq.shape[0]),
                                       _p(lq), C.c_size_t(lq.shape[0]), _p(al), _p(be), _p(asg), C.c_size_t(asg.shape[0]), C.c_size_t(n_aux),
                                       _p(hh), C.c_size_t(hh.shape[0]), _p(out[0]), _p(out[1]), _p(out[2]))
    if rc != 0:
        raise RuntimeError("groth16_prove_bls12_377 failed with code %d" % rc)
    return out


def ntt_timings():
    ms = (C.c_float * 4)()
    n = C.c_int(0)
    assert lib().celo_amd_ntt_last_timings(ms, C.byref(n)) == 0
    return {"load_ms": ms[0], "passes_ms": ms[1], "store_ms": ms[2], "total_ms": ms[3], "passes": n.value}


def pairing_timings():
    ms = (C.c_float * 4)()
    assert lib().celo_amd_pairing_last_timings(ms) == 0
    return {"miller_ms": ms[0], "product_ms": ms[1], "final_exp_ms": ms[2], "total_ms": ms[3]}


def msm_batch(group, bases_xy, inf, scalars, offsets, subgroup=False):
    """m independent MSMs in one call. offsets uint32 [m+1]. Returns uint64 [m, O] Jacobian results.
    subgroup=True (bls12_377_g2 only): the bases are vouched to lie in G2 (msm_batch_bls12_377_g2_subgroup: endomorphism split)."""
    A, S, O = GROUP_SHAPE[group]
    bases_xy = np.ascontiguousarray(bases_xy, dtype=np.uint64)
    scalars = np.ascontiguousarray(scalars, dtype=np.uint64)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
    m = offsets.size - 1
    assert bases_xy.size == int(offsets[-1]) * A and scalars.size == int(offsets[-1]) * S
    out = np.zeros((m, O), dtype=np.uint64)
    rc = getattr(lib(), "msm_batch_" + group + ("_subgroup" if subgroup else ""))(_p(bases_xy), _p(inf), _p(scalars), _p(offsets), C.c_size_t(m), _p(out))
    if rc != 0:
        raise RuntimeError(f"msm_batch_{group} failed rc={rc}")
    return out


def pairing_product_is_one_bw6(g1_xy, inf1, g2_xy, inf2):
    g1_xy = np.ascontiguousarray(g1_xy, dtype=np.uint64)
    g2_xy = np.ascontiguousarray(g2_xy, dtype=np.uint64)
    k = g1_xy.size // 24
    one = C.c_int(0)
    rc = lib().pairing_product_is_one_bw6_761(_p(g1_xy), _p(inf1), _p(g2_xy), _p(inf2), C.c_size_t(k), C.byref(one))
    if rc != 0:
        raise RuntimeError(f"pairing_product_is_one_bw6_761 failed rc={rc}")
    return bool(one.value)


def pairing_product_is_one_batch_bw6(g1_xy, inf1, g2_xy, inf2, offsets):
    """m independent BW6-761 products; g1_xy, g2_xy uint64 [k,24], offsets uint32 [m+1]. Returns uint8 [m]."""
    g1_xy = np.ascontiguousarray(g1_xy, dtype=np.uint64)
    g2_xy = np.ascontiguousarray(g2_xy, dtype=np.uint64)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
    m = offsets.size - 1
    out = np.zeros(m, dtype=np.uint8)
    rc = lib().pairing_product_is_one_batch_bw6_761(_p(g1_xy), _p(inf1), _p(g2_xy), _p(inf2), _p(offsets), C.c_size_t(m), _p(out))
    if rc != 0:
        raise RuntimeError(f"pairing_product_is_one_batch_bw6_761 failed rc={rc}")
    return out


def pairing_gt_bw6(g1_xy, inf1, g2_xy, inf2, offsets, miller_only=False):
    g1_xy = np.ascontiguousarray(g1_xy, dtype=np.uint64)
    g2_xy = np.ascontiguousarray(g2_xy, dtype=np.uint64)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
    m = offsets.size - 1
    out = np.zeros((m, 72), dtype=np.uint64)
    rc = lib().celo_amd_pairing_gt_bw6_761(_p(g1_xy), _p(inf1), _p(g2_xy), _p(inf2), _p(offsets), C.c_size_t(m),
                                           C.c_int(1 if miller_only else 0), _p(out))
    if rc != 0:
        raise RuntimeError(f"celo_amd_pairing_gt_bw6_761 failed rc={rc}")
    return out


def decompress(group, data, check_subgroup=True):
    """Bulk decoding of compressed points (include/celo_bls_amd.h: decompress_bls12_377_g1/_g2, decompress_bw6_761_g1/_g2).  group:
    "g1" (48 B each), "g2" (96 B each), "bw6_761_g1" / "bw6_761_g2" (96 B each); data: bytes of n concatenated encodings.  Returns
    (xy, status): xy (n, 12 | 24) uint64 affine arkworks Montgomery limbs (zero rows unless status == 0), status (n,) uint8 (0 ok,
    1 infinity, 2 invalid, 3 not in subgroup)."""
    size, words, fn = {"g1": (48, 12, "decompress_bls12_377_g1"), "g2": (96, 24, "decompress_bls12_377_g2"),
                       "bw6_761_g1": (96, 24, "decompress_bw6_761_g1"), "bw6_761_g2": (96, 24, "decompress_bw6_761_g2")}[group]
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    assert buf.size % size == 0
    n = buf.size // size
    xy = np.zeros((n, words), dtype=np.uint64)
    st = np.zeros(n, dtype=np.uint8)
    rc = getattr(lib(), fn)(_p(buf), C.c_size_t(n), C.c_int(1 if check_subgroup else 0), _p(xy), _p(st))
    if rc != 0:
        raise RuntimeError("%s failed with code %d" % (fn, rc))
    return xy, st


def decompress_dev(group, d_in, n, d_out, d_status, check_subgroup=True, stream=0):
    fn = {"g1": "decompress_bls12_377_g1_dev", "g2": "decompress_bls12_377_g2_dev",
          "bw6_761_g1": "decompress_bw6_761_g1_dev", "bw6_761_g2": "decompress_bw6_761_g2_dev"}[group]
    rc = getattr(lib(), fn)(C.c_void_p(d_in), C.c_size_t(n), C.c_int(1 if check_subgroup else 0), C.c_void_p(d_out), C.c_void_p(d_status), C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError("%s failed with code %d" % (fn, rc))


def decompress_dedup(group, data, check_subgroup=True, want_rep=True):
    """decompress() for "g1" / "g2" with each distinct byte string decoded once (decompress_bls12_377_g1/_g2_dedup).  Returns
    (xy, status, rep, decoded): xy and status as decompress(); rep (n,) uint32 (None without want_rep): a key with the same bytes at or
    before each key; decoded: how many keys went through the decoder."""
    size, words, fn = {"g1": (48, 12, "decompress_bls12_377_g1_dedup"), "g2": (96, 24, "decompress_bls12_377_g2_dedup")}[group]
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    assert buf.size % size == 0
    n = buf.size // size
    xy = np.zeros((n, words), dtype=np.uint64)
    st = np.zeros(n, dtype=np.uint8)
    rep = np.zeros(n, dtype=np.uint32) if want_rep else None
    decoded = C.c_uint64(0)
    rc = getattr(lib(), fn)(_p(buf), C.c_size_t(n), C.c_int(1 if check_subgroup else 0), _p(xy), _p(st), _p(rep), C.byref(decoded))
    if rc != 0:
        raise RuntimeError("%s failed with code %d" % (fn, rc))
    return xy, st, rep, decoded.value


def decompress_dedup_dev(group, d_in, n, d_out, d_status, d_rep=0, check_subgroup=True, stream=0):
    """The same on device buffers (integer device addresses; d_rep may be 0), on `stream`.  Returns decoded (the call drains the stream)."""
    fn = {"g1": "decompress_bls12_377_g1_dedup_dev", "g2": "decompress_bls12_377_g2_dedup_dev"}[group]
    decoded = C.c_uint64(0)
    rc = getattr(lib(), fn)(C.c_void_p(d_in), C.c_size_t(n), C.c_int(1 if check_subgroup else 0), C.c_void_p(d_out), C.c_void_p(d_status), C.c_void_p(d_rep or None),
                            C.byref(decoded), C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError("%s failed with code %d" % (fn, rc))
    return decoded.value


def key_dedup_set(on=-1, slack_log=-1, max_probes=0):
    """The key de-duplication switch (celo_amd_key_dedup_set).  on: -1 the rule, 0 never, 1 always, for the composed epoch entry points;
    slack_log 0 .. 2 (-1: the default); max_probes 1 .. 1024 (0: the default)."""
    if lib().celo_amd_key_dedup_set(C.c_int(on), C.c_int(slack_log), C.c_int(max_probes)) != 0:
        raise ValueError("celo_amd_key_dedup_set: on -1 .. 1, slack_log -1 .. 2, max_probes 0 .. 1024, not %r" % ((on, slack_log, max_probes),))


def key_dedup_get():
    """(on, slack_log, max_probes) as they stand"""
    out = (C.c_int * 3)()
    assert lib().celo_amd_key_dedup_get(out) == 0
    return tuple(out)


def key_dedup_last():
    """(keys, decoded, ms): the last de-duplicating call; ms = [table + representatives + compaction, gather, decode, scatter] (HIP events)"""
    counts = (C.c_uint64 * 2)()
    ms = (C.c_float * 4)()
    assert lib().celo_amd_key_dedup_last(counts, ms) == 0
    return int(counts[0]), int(counts[1]), list(ms)


_UNCOMPRESSED = {"g1": (96, 12, "decode_uncompressed_bls12_377_g1"), "g2": (192, 24, "decode_uncompressed_bls12_377_g2"),
                 "bw6_761_g1": (192, 24, "decode_uncompressed_bw6_761_g1"), "bw6_761_g2": (192, 24, "decode_uncompressed_bw6_761_g2")}


def decode_uncompressed(group, data, check=True):
    """Bulk decoding of uncompressed points (decode_uncompressed_<curve>_g1/_g2): group "g1" / "g2" (BLS12-377, 96 / 192 B each) or
    "bw6_761_g1" / "bw6_761_g2" (192 B each); x, then y with the flags.  check: on the curve and in the subgroup
    (deserialize_uncompressed); False: range only (deserialize_unchecked).  Returns (xy (n, 12 | 24) uint64, status (n,) uint8) as decompress()."""
    size, words, fn = _UNCOMPRESSED[group]
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    assert buf.size % size == 0
    n = buf.size // size
    xy = np.zeros((n, words), dtype=np.uint64)
    st = np.zeros(n, dtype=np.uint8)
    rc = getattr(lib(), fn)(_p(buf), C.c_size_t(n), C.c_int(1 if check else 0), _p(xy), _p(st))
    if rc != 0:
        raise RuntimeError("%s failed with code %d" % (fn, rc))
    return xy, st


def decode_uncompressed_dev(group, d_in, n, d_out, d_status, check=True, stream=0):
    """The same on device buffers (integer device addresses), on `stream`: BLS12-377 only ("g1" / "g2"); returns the entry point's code."""
    fn = _UNCOMPRESSED[group][2] + "_dev"
    return getattr(lib(), fn)(C.c_void_p(d_in), C.c_size_t(n), C.c_int(1 if check else 0), C.c_void_p(d_out), C.c_void_p(d_status), C.c_void_p(stream))


# ---- validation of affine rows (include/celo_bls_amd.h: check_points_*)
CHECK_GROUPS = {"bls12_377_g1": 12, "bls12_377_g2": 24, "bw6_761_g1": 24, "bw6_761_g2": 24}          # u64 per row


def check_points(group, xy, inf=None, level=2):
    """Bulk validation of affine rows (check_points_<group>): xy (n, 12 | 24) uint64 arkworks Montgomery limbs, inf (n,) uint8 or None;
    level 1: the curve equation, 2: the curve and the prime-order subgroup.  Returns (status (n,) uint8, first_bad): 0 good, 1 the row is
    flagged as the identity, 2 a coordinate is not below q or the point is off the curve, 3 outside the subgroup; first_bad is the smallest
    index with status 2 or 3, n if there is none."""
    words = CHECK_GROUPS[group]
    rows = _rows(xy, words)
    n = rows.shape[0]
    flags = None if inf is None else np.ascontiguousarray(inf, dtype=np.uint8)
    assert flags is None or flags.size == n
    st = np.zeros(n, dtype=np.uint8)
    first = C.c_uint64(0)
    rc = getattr(lib(), "check_points_" + group)(_p(rows), _p(flags), C.c_size_t(n), C.c_int(level), _p(st), C.byref(first))
    if rc != 0:
        raise RuntimeError("check_points_%s failed with code %d" % (group, rc))
    return st, first.value


def check_points_dev(group, d_xy, d_inf, n, d_status, level=2, stream=0):
    """The same on device buffers (integer device addresses; d_inf may be 0), on `stream`.  Returns first_bad (the call drains the stream)."""
    first = C.c_uint64(0)
    rc = getattr(lib(), "check_points_%s_dev" % group)(C.c_void_p(d_xy), C.c_void_p(d_inf or None), C.c_size_t(n), C.c_int(level), C.c_void_p(d_status),
                                                      C.byref(first), C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError("check_points_%s_dev failed with code %d" % (group, rc))
    return first.value


def check_points_last_ms():
    """kernel time of the last check_points_* call (HIP events around its kernels)"""
    ms = C.c_float(0)
    assert lib().celo_amd_check_points_last_ms(C.byref(ms)) == 0
    return ms.value


def wire761_set_subgroup_test(form):
    """Which subgroup test the BW6-761 decoders, the serialized key loader and verifiers and check_points_bw6_761_* run: 0 = the
    endomorphism form [a]P + [b]phi(P) == O (the default), 1 = the r P ladder, its definition.  The verdicts are the same."""
    if lib().celo_amd_wire761_set_subgroup_test(C.c_int(form)) != 0:
        raise ValueError("celo_amd_wire761_set_subgroup_test: 0 or 1, not %r" % (form,))


# ---- encoding into the wire form (include/celo_bls_amd.h: compress_*, encode_uncompressed_*, groth16_serialize_*)
KEY_ERR_CAPACITY = 35
_ENCODE_GROUPS = {"g1": (12, 48, "bls12_377_g1"), "g2": (24, 96, "bls12_377_g2"), "bw6_761": (24, 96, "bw6_761"),
                  "bw6_761_g1": (24, 96, "bw6_761"), "bw6_761_g2": (24, 96, "bw6_761")}


class WireEncodeError(RuntimeError):
    def __init__(self, fn, code):
        super().__init__("%s failed with code %d" % (fn, code))
        self.code = code


def _encode_fn(group, compressed, dev):
    words, size, suffix = _ENCODE_GROUPS[group]
    return words, size * (1 if compressed else 2), ("compress_" if compressed else "encode_uncompressed_") + suffix + ("_dev" if dev else "")


def encode_points(group, rows, inf=None, compressed=True):
    """Bulk encoding of affine points (compress_* / encode_uncompressed_*).  group: "g1" / "g2" (BLS12-377, rows (n, 12) / (n, 24) uint64
    arkworks Montgomery limbs) or "bw6_761" (both groups of BW6-761, rows (n, 24); "bw6_761_g1" / "bw6_761_g2" are accepted as names of the
    same); inf: uint8 (n,) or None.  Returns (out (n, 48 | 96 | 192) uint8, status (n,) uint8: 0 encoded, 1 identity, 2 not a field element)."""
    words, size, fn = _encode_fn(group, compressed, False)
    r = _rows(rows, words)
    n = r.shape[0]
    i = None if inf is None else np.ascontiguousarray(inf, dtype=np.uint8).reshape(n)
    out = np.zeros((n, size), dtype=np.uint8)
    st = np.zeros(n, dtype=np.uint8)
    rc = getattr(lib(), fn)(_p(r), _p(i), C.c_size_t(n), _p(out), _p(st))
    if rc != 0:
        raise WireEncodeError(fn, rc)
    return out, st


def encode_points_dev(group, d_rows, d_inf, n, d_out, d_status, compressed=True, stream=0):
    """The same on device buffers (integer device addresses; d_inf 0 / None: no identity bytes), on `stream`."""
    fn = _encode_fn(group, compressed, True)[2]
    rc = getattr(lib(), fn)(C.c_void_p(d_rows), C.c_void_p(d_inf or None), C.c_size_t(n), C.c_void_p(d_out), C.c_void_p(d_status), C.c_void_p(stream))
    if rc != 0:
        raise WireEncodeError(fn, rc)


class KeySerializeError(RuntimeError):
    def __init__(self, code, out_len=None, first_bad_point=None, curve="bw6_761"):
        super().__init__("groth16_serialize_key_%s failed with code %d%s" % (curve, code, "" if first_bad_point is None else " (first bad point: %d)" % first_bad_point))
        self.code = code
        self.out_len = out_len
        self.first_bad_point = first_bad_point


def groth16_serialized_key_size(n_inputs, n_vars, n_h, form=0, vk_only=False, curve="bw6_761"):
    """Byte length of the serialized ProvingKey (or VerifyingKey) of `curve` with these counts (groth16_serialized_key_size_<curve>); no device call."""
    ln = C.c_uint64(0)
    rc = getattr(lib(), "groth16_serialized_key_size_" + curve)(C.c_size_t(n_inputs), C.c_size_t(n_vars), C.c_size_t(n_h), C.c_int(form), C.c_int(1 if vk_only else 0),
                                                                C.byref(ln))
    if rc != 0:
        raise KeySerializeError(rc, curve=curve)
    return ln.value


def _key_rows(x, names):
    """a flat uint64 buffer of rows, or the dict groth16_setup returns for it (sections concatenated in serialization order)"""
    if isinstance(x, dict):
        x = np.concatenate([np.ascontiguousarray(x[k], dtype=np.uint64).reshape(-1) for k in names])
    return np.ascontiguousarray(x, dtype=np.uint64).reshape(-1)


def groth16_serialize_key(vk, rows=None, n_vars=0, n_h=0, form=0, cap=None, curve="bw6_761"):
    """ProvingKey::serialize (form 0) / serialize_uncompressed (1) of groth16_setup's "vk" and "rows" (dicts or flat buffers), or
    VerifyingKey::serialize when rows is None (groth16_serialize_key_<curve>; "bw6_761": every row 24 u64; "bls12_377": G1 rows 12 u64, G2
    rows 24).  cap: the output buffer's size (default: what is needed).
    Returns bytes; raises KeySerializeError (.code 35 with .out_len, 33 with .first_bad_point)."""
    w1 = 24 if curve == "bw6_761" else 12
    v = _key_rows(vk, ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "gamma_abc_g1"))
    assert v.size >= w1 + 72 and (v.size - w1 - 72) % w1 == 0, "vk: alpha_g1, three G2 rows, then the rows of gamma_abc_g1"
    n_inputs = (v.size - w1 - 72) // w1
    r = None if rows is None else _key_rows(rows, ("beta_g1", "delta_g1", "a_query", "b_g1_query", "b_g2_query", "h_query", "l_query"))
    if r is not None:
        assert r.size == (2 + 2 * n_vars + n_h + (n_vars - n_inputs)) * w1 + n_vars * 24, "rows do not match n_vars / n_h"
    need = groth16_serialized_key_size(n_inputs, n_vars, n_h, form, rows is None, curve)
    out = np.zeros(need if cap is None else cap, dtype=np.uint8)
    ln, bad = C.c_uint64(0), C.c_uint64(0)
    rc = getattr(lib(), "groth16_serialize_key_" + curve)(_p(v), C.c_size_t(n_inputs), _p(r), C.c_size_t(n_vars), C.c_size_t(n_h), C.c_int(form), _p(out),
                                                          C.c_size_t(out.size), C.byref(ln), C.byref(bad))
    if rc != 0:
        raise KeySerializeError(rc, ln.value, bad.value if rc == KEY_ERR_POINT else None, curve)
    return out[:ln.value].tobytes()


def groth16_serialize_proof(a_xyz, b_xyz, c_xyz, curve="bw6_761"):
    """Proof::serialize (BW6-761: 288 B; BLS12-377: 192 B) from the three Jacobian points groth16_prove / ProvingKey.prove return
    (groth16_serialize_proof_<curve>)."""
    w1, w2, nbytes = (36, 36, 288) if curve == "bw6_761" else (18, 36, 192)
    pts = [np.ascontiguousarray(x, dtype=np.uint64).reshape(w) for x, w in zip((a_xyz, b_xyz, c_xyz), (w1, w2, w1))]
    out = np.zeros(nbytes, dtype=np.uint8)
    rc = getattr(lib(), "groth16_serialize_proof_" + curve)(_p(pts[0]), _p(pts[1]), _p(pts[2]), _p(out))
    if rc != 0:
        raise RuntimeError("groth16_serialize_proof_%s failed with code %d" % (curve, rc))
    return out.tobytes()


def wire_encode_last_ms():
    ms = C.c_float(0)
    assert lib().celo_amd_wire_encode_last_ms(C.byref(ms)) == 0
    return ms.value


def wire_encode_key_timings():
    """the last groth16_serialize_key call: (rows to the device, encoding, bytes back) in ms"""
    ms = (C.c_float * 3)()
    assert lib().celo_amd_wire_encode_key_timings(ms) == 0
    return tuple(ms)


def wire761_last_timings():
    """(kernel ms of the last BW6-761 decode call, the last serialized key load's transfer / decode / table-build ms)"""
    ms = (C.c_float * 4)()
    assert lib().celo_amd_wire761_last_timings(ms) == 0
    return tuple(ms)


def decompress_last_ms():
    ms = C.c_float(0)
    assert lib().celo_amd_decompress_last_ms(C.byref(ms)) == 0
    return ms.value


def hash_to_g1_composite(domain, messages, extras=None, cip22=False):
    """Batched hash-to-G1 with the composite hasher (include/celo_bls_amd.h: hash_to_g1_composite_bls12_377); same conventions
    as hash_to_g1_direct."""
    return hash_to_g1_direct(domain, messages, extras, composite=(2 if cip22 else 1))


def hash_to_g1_direct(domain, messages, extras=None, cip22_tail=False, composite=0):
    """Batched try-and-increment hash-to-G1 over the direct hasher (include/celo_bls_amd.h: hash_to_g1_direct_bls12_377), or,
    with cip22_tail, the CIP22 loop over precomputed inner CRHs (hash_to_g1_cip22_tail_bls12_377: `messages` are the inner
    hashes).  domain: 8 bytes; messages / extras: lists of bytes (extras None = no extra data).  Returns (xy (n, 12) uint64
    affine arkworks Montgomery limbs, attempts (n,) uint8; 255 = no point)."""
    n = len(messages)
    assert len(domain) == 8 and (extras is None or len(extras) == n)

    def pack(items):
        off = np.zeros(n + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(b) for b in items], dtype=np.uint64) if n else []
        data = np.frombuffer(b"".join(items) or b"\0", dtype=np.uint8)
        return data, off
    mdat, moff = pack(messages)
    edat, eoff = pack(extras) if extras is not None else (None, None)
    dom = np.frombuffer(bytes(domain), dtype=np.uint8)
    xy = np.zeros((n, 12), dtype=np.uint64)
    att = np.zeros(n, dtype=np.uint8)
    if composite:
        rc = lib().hash_to_g1_composite_bls12_377(_p(dom), _p(mdat), _p(moff), _p(edat), _p(eoff), C.c_size_t(n), C.c_int(composite - 1), _p(xy), _p(att))
    else:
        fn = lib().hash_to_g1_cip22_tail_bls12_377 if cip22_tail else lib().hash_to_g1_direct_bls12_377
        rc = fn(_p(dom), _p(mdat), _p(moff), _p(edat), _p(eoff), C.c_size_t(n), _p(xy), _p(att))
    if rc != 0:
        raise RuntimeError("hash_to_g1 (%s) failed with code %d" % ("cip22 tail" if cip22_tail else "direct", rc))
    return xy, att


def hash_to_g2_composite(domain, messages, extras=None, cip22=False, compat=0):
    """Batched hash-to-G2 with the composite hasher (include/celo_bls_amd.h: hash_to_g2_composite_bls12_377); same conventions as
    hash_to_g2_direct."""
    return hash_to_g2_direct(domain, messages, extras, composite=(2 if cip22 else 1), compat=compat)


def hash_to_g2_direct(domain, messages, extras=None, cip22_tail=False, composite=0, compat=0):
    """Batched try-and-increment hash-to-G2 (include/celo_bls_amd.h: hash_to_g2_direct_bls12_377; cip22_tail: hash_to_g2_cip22_tail_bls12_377
    over precomputed inner CRHs).  Arguments as hash_to_g1_direct; compat 0: the flags as the XOF gives them (the reference's vectors), 1: the
    deployed remap.  Returns (xy (n, 24) uint64: x.c0, x.c1, y.c0, y.c1 as arkworks Montgomery limbs, attempts (n,) uint8; 255 = no point)."""
    n = len(messages)
    assert len(domain) == 8 and (extras is None or len(extras) == n)

    def pack(items):
        off = np.zeros(n + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(b) for b in items], dtype=np.uint64) if n else []
        data = np.frombuffer(b"".join(items) or b"\0", dtype=np.uint8)
        return data, off
    mdat, moff = pack(messages)
    edat, eoff = pack(extras) if extras is not None else (None, None)
    dom = np.frombuffer(bytes(domain), dtype=np.uint8)
    xy = np.zeros((n, 24), dtype=np.uint64)
    att = np.zeros(n, dtype=np.uint8)
    if composite:
        rc = lib().hash_to_g2_composite_bls12_377(_p(dom), _p(mdat), _p(moff), _p(edat), _p(eoff), C.c_size_t(n), C.c_int(composite - 1), C.c_int(compat), _p(xy), _p(att))
    else:
        fn = lib().hash_to_g2_cip22_tail_bls12_377 if cip22_tail else lib().hash_to_g2_direct_bls12_377
        rc = fn(_p(dom), _p(mdat), _p(moff), _p(edat), _p(eoff), C.c_size_t(n), C.c_int(compat), _p(xy), _p(att))
    if rc != 0:
        raise RuntimeError("hash_to_g2 (%s) failed with code %d" % ("composite" if composite else "cip22 tail" if cip22_tail else "direct", rc))
    return xy, att


def hash_to_g2_one(domain, message, extra=b"", mode=0, compat=0):
    """One message through the serial loop on the host (hash_to_g2_one_bls12_377: no device is touched).  mode 0 direct, 1 the CIP22 tail
    (message = the inner CRH), 2 composite, 3 composite CIP22.  Returns (xy (24,) uint64, attempt; 255 = no point)."""
    assert len(domain) == 8
    xy = np.zeros(24, dtype=np.uint64)
    att = C.c_int(0)
    rc = lib().hash_to_g2_one_bls12_377(bytes(domain), bytes(message), C.c_size_t(len(message)), bytes(extra), C.c_size_t(len(extra)), C.c_int(mode), C.c_int(compat),
                                        _p(xy), C.byref(att))
    if rc != 0:
        raise RuntimeError("hash_to_g2_one failed with code %d" % rc)
    return xy, att.value


def hash_g2_set_lane_budget_log(log):
    """celo_amd_hash_g2_set_lane_budget_log: rounds give each open message the widest power of two of counters <= 16 with open * width <=
    2^log (4 ... 17, default 17).  Returns the code: 0, or 2 for a value outside the range (nothing changes then)."""
    return lib().celo_amd_hash_g2_set_lane_budget_log(C.c_int(log))


def hash_g2_last_split():
    """(candidate rounds ms, cofactor kernel ms) of the last hash_to_g2_* call"""
    ms = (C.c_float * 2)()
    assert lib().celo_amd_hash_g2_last_split(ms) == 0
    return tuple(ms)


def hash_last_ms():
    ms = C.c_float(0)
    assert lib().celo_amd_hash_last_ms(C.byref(ms)) == 0
    return ms.value


def hash_last_rounds():
    """Candidate rounds (kernel launches of the try-and-increment loop) of the last hash_to_g1_* or hash_to_g2_* call that hashed a message."""
    r = C.c_int(0)
    assert lib().celo_amd_hash_last_rounds(C.byref(r)) == 0
    return r.value


CRH_LANES = (1, 2, 4, 8, 16, 32, 64, 128, 256)   # the widths celo_amd_crh_set_lanes accepts besides 0 (csrc/pedersen.h)


def crh_set_lanes(lanes):
    """lanes per message of the CRH kernel (0 = the rule of csrc/pedersen.h, else one of CRH_LANES); needs no device"""
    rc = lib().celo_amd_crh_set_lanes(C.c_int(lanes))
    if rc != 0:
        raise ValueError("celo_amd_crh_set_lanes(%d) failed with code %d" % (lanes, rc))


def crh_last_lanes():
    """the width the last CRH kernel of this process ran with (0 before the first)"""
    lanes = C.c_int(0)
    assert lib().celo_amd_crh_last_lanes(C.byref(lanes)) == 0
    return lanes.value


def composite_crh(messages):
    """The composite hasher's Pedersen CRH of n messages in one GPU launch (include/celo_bls_amd.h: composite_crh_bls12_377).
    Returns a list of n 48-byte hashes."""
    n = len(messages)
    off = np.zeros(n + 1, dtype=np.uint64)
    if n:
        off[1:] = np.cumsum([len(b) for b in messages], dtype=np.uint64)
    data = np.frombuffer(b"".join(messages) or b"\0", dtype=np.uint8)
    out = np.zeros((n, 48), dtype=np.uint8)
    rc = lib().composite_crh_bls12_377(_p(data), _p(off), C.c_size_t(n), _p(out))
    if rc != 0:
        raise RuntimeError("composite_crh_bls12_377 failed with code %d" % rc)
    return [out[i].tobytes() for i in range(n)]


def composite_crh_dev(d_msgs, msg_off, n, d_out48, stream=0):
    """composite_crh_bls12_377_dev: message bytes and the n x 48 output on the device (data pointers), msg_off a host array.  Returns the code."""
    off = None if msg_off is None else np.ascontiguousarray(msg_off, dtype=np.uint64).reshape(-1)
    return lib().composite_crh_bls12_377_dev(C.c_void_p(d_msgs or None), _p(off), C.c_size_t(n), C.c_void_p(d_out48 or None), C.c_void_p(stream))


def hash_to_g1_dev(domain, d_msgs, msg_off, d_extras, extra_off, n, d_out_xy, d_attempts, mode=0, stream=0):
    """The hash_to_g1_*_bls12_377_dev entries: bytes, rows (n x 12 u64) and attempts (n) on the device (data pointers; d_extras 0 / None with
    extra_off None = no extra data), the offsets host arrays.  mode 0 direct, 1 the CIP22 tail (d_msgs are the inner CRHs), 2 composite, 3 composite
    CIP22.  Returns the code (0, or 2: nothing written)."""
    moff = None if msg_off is None else np.ascontiguousarray(msg_off, dtype=np.uint64).reshape(-1)
    eoff = None if extra_off is None else np.ascontiguousarray(extra_off, dtype=np.uint64).reshape(-1)
    dom = None if domain is None else np.frombuffer(bytes(domain), dtype=np.uint8)
    args = (_p(dom), C.c_void_p(d_msgs or None), _p(moff), C.c_void_p(d_extras or None), _p(eoff), C.c_size_t(n))
    outs = (C.c_void_p(d_out_xy or None), C.c_void_p(d_attempts or None), C.c_void_p(stream))
    if mode in (2, 3):
        return lib().hash_to_g1_composite_bls12_377_dev(*args, C.c_int(mode - 2), *outs)
    if mode not in (0, 1):
        raise ValueError("hash_to_g1_dev: mode is 0 .. 3")
    return (lib().hash_to_g1_cip22_tail_bls12_377_dev if mode == 1 else lib().hash_to_g1_direct_bls12_377_dev)(*args, *outs)


def normalize(group, jac):
    """Jacobian -> affine for n points in one GPU launch (include/celo_bls_amd.h: normalize_bls12_377_g1/_g2, normalize_bw6_761_g1/_g2).
    group: "g1" | "g2" (BLS12-377) | "bw6_761_g1" | "bw6_761_g2".  jac: (n, 18 | 36) uint64; returns (xy (n, 12 | 24) uint64, inf (n,) uint8)."""
    words, fn = {"g1": (6, "normalize_bls12_377_g1"), "g2": (12, "normalize_bls12_377_g2"),
                 "bw6_761_g1": (12, "normalize_bw6_761_g1"), "bw6_761_g2": (12, "normalize_bw6_761_g2")}[group]
    j = np.ascontiguousarray(jac, dtype=np.uint64).reshape(-1, 3 * words)
    n = j.shape[0]
    xy = np.zeros((n, 2 * words), dtype=np.uint64)
    inf = np.zeros(n, dtype=np.uint8)
    rc = getattr(lib(), fn)(_p(j), C.c_size_t(n), _p(xy), _p(inf))
    if rc != 0:
        raise RuntimeError("%s failed with code %d" % (fn, rc))
    return xy, inf


# ---- batched fixed-base scalar multiplication and Groth16 setup (include/celo_bls_amd.h: fixed_base_mul_*, groth16_setup_*)
def fixed_base_mul(group, gen_xy, scalars):
    """out_i = k_i G: gen_xy the affine generator (12 | 24 uint64 limbs), scalars (n, 4 | 6) canonical uint64 limbs.  Returns (xy (n, 12 | 24)
    uint64, inf (n,) uint8).  Raises ValueError on code 2 (a scalar >= r, the identity as generator)."""
    aw, sw, _ = GROUP_SHAPE[group]
    g = np.ascontiguousarray(gen_xy, dtype=np.uint64).reshape(aw)
    sc = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, sw)
    n = sc.shape[0]
    xy = np.zeros((n, aw), dtype=np.uint64)
    inf = np.zeros(n, dtype=np.uint8)
    rc = getattr(lib(), "fixed_base_mul_" + group)(_p(g), _p(sc), C.c_size_t(n), _p(xy), _p(inf))
    if rc == 2:
        raise ValueError("fixed_base_mul_%s: bad arguments (code 2)" % group)
    if rc != 0:
        raise RuntimeError("fixed_base_mul_%s failed with code %d" % (group, rc))
    return xy, inf


def fixed_base_mul_dev(group, gen_xy, d_scalars, n, d_out, d_inf, stream=0):
    """The same on device buffers (data pointers); returns the code (0, or 2 for a scalar >= r: nothing written)."""
    aw = GROUP_SHAPE[group][0]
    g = np.ascontiguousarray(gen_xy, dtype=np.uint64).reshape(aw)
    return getattr(lib(), "fixed_base_mul_%s_dev" % group)(_p(g), C.c_void_p(d_scalars), C.c_size_t(n), C.c_void_p(d_out), C.c_void_p(d_inf),
                                                         C.c_void_p(stream))


def set_fixed_base_window(c):
    """the generator tables' window bits (0 = the default)"""
    rc = lib().celo_amd_fixed_base_set_window(C.c_int(c))
    if rc != 0:
        raise ValueError("celo_amd_fixed_base_set_window(%d) failed with code %d" % (c, rc))


def setup_timings():
    """the last fixed_base_mul_* / groth16_setup_* call: {table, fr_prep, g1_rows, g2_rows, normalize, key_tables, wall} in ms"""
    ms = (C.c_float * 8)()
    lib().celo_amd_setup_last_timings(ms)
    return dict(zip(("table", "fr_prep", "g1_rows", "g2_rows", "normalize", "key_tables", "wall"), list(ms)[:7]))


# ---- batched variable-base scalar multiplication and batched signing (include/celo_bls_amd.h: scalar_mul_batch_*, sign_batch_bls12_377)
SCALAR_MUL_BLOCK = 64                    # lanes per workgroup of the table and ladder kernels (csrc/unit_varbase.hip VB_BLOCK)
SCALAR_MUL_WINDOWS = tuple(range(2, 9))  # the window bits celo_amd_scalar_mul_set_window accepts besides 0 (csrc/var_base.h VB_MIN_C .. VB_MAX_C)
SIG_DOMAIN, POP_DOMAIN = b"ULforxof", b"ULforpop"


def _scalar_mul_name(group, subgroup):
    if subgroup and group != "bls12_377_g1":
        raise ValueError("the subgroup path exists for bls12_377_g1 only")
    return "scalar_mul_batch_" + group + ("_subgroup" if subgroup else "")


def scalar_mul_batch(group, xy, inf, scalars, subgroup=False):
    """out_i = [k_i] P_i: xy (n, 12 | 24) affine arkworks limbs, inf (n,) uint8 or None, scalars (n, 4 | 6) canonical uint64 limbs - or ONE row,
    shared by every point.  subgroup (bls12_377_g1 only): the caller vouches for points of the prime-order subgroup (the GLV ladder).
    Returns (xy, inf) in the row format of fixed_base_mul.  Raises ValueError on code 2 (a scalar >= r, a scalar count that is neither 1 nor n)."""
    aw, sw, _ = GROUP_SHAPE[group]
    name = _scalar_mul_name(group, subgroup)
    pts = _rows(xy, aw)
    n = pts.shape[0]
    sc = _rows(scalars, sw)
    fl = None if inf is None else np.ascontiguousarray(inf, dtype=np.uint8)
    assert fl is None or fl.shape == (n,)
    out = np.zeros((n, aw), dtype=np.uint64)
    oinf = np.zeros(n, dtype=np.uint8)
    rc = getattr(lib(), name)(_p(pts), _p(fl), _p(sc), C.c_size_t(sc.shape[0]), C.c_size_t(n), _p(out), _p(oinf))
    if rc == 2:
        raise ValueError("%s: bad arguments (code 2)" % name)
    if rc != 0:
        raise RuntimeError("%s failed with code %d" % (name, rc))
    return out, oinf


def scalar_mul_batch_dev(group, d_xy, d_inf, d_scalars, n_scalars, n, d_out, d_out_inf, subgroup=False, stream=0):
    """The same on device buffers (data pointers; d_inf may be 0 / None); returns the code (0, or 2: nothing written)."""
    return getattr(lib(), _scalar_mul_name(group, subgroup) + "_dev")(C.c_void_p(d_xy), C.c_void_p(d_inf or None), C.c_void_p(d_scalars), C.c_size_t(n_scalars),
                                                                     C.c_size_t(n), C.c_void_p(d_out), C.c_void_p(d_out_inf), C.c_void_p(stream))


def set_scalar_mul_window(c):
    """the ladder's window bits (0 = the default, else one of SCALAR_MUL_WINDOWS)"""
    rc = lib().celo_amd_scalar_mul_set_window(C.c_int(c))
    if rc != 0:
        raise ValueError("celo_amd_scalar_mul_set_window(%d) failed with code %d" % (c, rc))


def set_scalar_mul_chunk_rows(rows):
    """rows per chunk of the per-call workspace (0 = the default)"""
    rc = lib().celo_amd_scalar_mul_set_chunk_rows(C.c_uint32(rows))
    if rc != 0:
        raise ValueError("celo_amd_scalar_mul_set_chunk_rows(%d) failed with code %d" % (rows, rc))


def scalar_mul_last_ms():
    """the last scalar_mul_batch_* / sign_batch call: {table, ladder, normalize, wall} in ms"""
    ms = (C.c_float * 4)()
    assert lib().celo_amd_scalar_mul_last_ms(ms) == 0
    return dict(zip(("table", "ladder", "normalize", "wall"), list(ms)))


def sign_batch(sk, domain, messages, extras=None, mode=0):
    """sig_i = [sk_i] H(msg_i) (include/celo_bls_amd.h: sign_batch_bls12_377).  sk: (1 | n, 4) canonical uint64 limbs (one key for every message,
    or one per message); domain: SIG_DOMAIN | POP_DOMAIN; messages / extras: lists of bytes (extras None = no extra data); mode 0 direct,
    2 composite, 3 composite CIP22.  Returns (sigs (n, 48) uint8 as serialize_signature writes them, attempts (n,) uint8; 255 = no point and a
    zero signature).  Raises ValueError on code 2."""
    n = len(messages)
    assert len(domain) == 8 and (extras is None or len(extras) == n)

    def pack(items):
        off = np.zeros(n + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(b) for b in items], dtype=np.uint64) if n else []
        data = np.frombuffer(b"".join(items) or b"\0", dtype=np.uint8)
        return data, off
    mdat, moff = pack(messages)
    edat, eoff = pack(extras) if extras is not None else (None, None)
    dom = np.frombuffer(bytes(domain), dtype=np.uint8)
    keys = _rows(sk, 4)
    sig = np.zeros((n, 48), dtype=np.uint8)
    att = np.zeros(n, dtype=np.uint8)
    rc = lib().sign_batch_bls12_377(_p(keys), C.c_size_t(keys.shape[0]), _p(dom), _p(mdat), _p(moff), _p(edat), _p(eoff), C.c_size_t(n), C.c_int(mode), _p(sig),
                                    _p(att))
    if rc == 2:
        raise ValueError("sign_batch_bls12_377: bad arguments (code 2)")
    if rc != 0:
        raise RuntimeError("sign_batch_bls12_377 failed with code %d" % rc)
    return sig, att


# ---- masked segmented point sums (include/celo_bls_amd.h: aggregate_by_bitmap_*)
AGGREGATE_LANES = (1, 2, 4, 8, 16, 32, 64)   # the lane widths celo_amd_aggregate_set_lanes accepts besides 0 (csrc/aggregate.h)
AGGREGATE_GROUPS = ("bls12_377_g1", "bls12_377_g2")


def aggregate_by_bitmap(group, pk_xy, pk_inf, offsets, bits):
    """out_i = sum of the rows of pk_xy that bits_i selects.  offsets: (m + 1,) uint32 with bits (rows,) parallel to the rows - per-seal sets -
    or (2,) with bits (m, n) - one shared set of n = offsets[1] - offsets[0] rows.  pk_inf: (rows,) uint8 or None.  Returns (xy (m, 12 | 24), inf (m,),
    count (m,) uint32) in the row format of fixed_base_mul.  Raises ValueError on code 2."""
    if group not in AGGREGATE_GROUPS:
        raise ValueError("aggregate_by_bitmap: group is one of %s" % (AGGREGATE_GROUPS,))
    aw = GROUP_SHAPE[group][0]
    pts = _rows(pk_xy, aw)
    off = np.ascontiguousarray(offsets, dtype=np.uint32).reshape(-1)
    b = np.ascontiguousarray(bits, dtype=np.uint8)
    n_sets = off.shape[0] - 1
    m = b.shape[0] if (b.ndim == 2 and n_sets == 1) else n_sets
    fl = None if pk_inf is None else np.ascontiguousarray(pk_inf, dtype=np.uint8)
    o = [int(v) for v in off]
    if n_sets < 1 or any(hi < lo for lo, hi in zip(o, o[1:])) or pts.shape[0] < o[-1] or (fl is not None and fl.shape != (pts.shape[0],)) or \
            b.size != (m * (o[1] - o[0]) if n_sets == 1 else o[-1]):
        raise ValueError("aggregate_by_bitmap_%s: offsets, rows and bits do not match" % group)
    if pts.shape[0] == 0:
        pts = np.zeros((1, aw), dtype=np.uint64)      # (a pointer to pass: no row is read)
    if b.size == 0:
        b = np.zeros(1, dtype=np.uint8)
    out = np.zeros((m, aw), dtype=np.uint64)
    oinf = np.zeros(m, dtype=np.uint8)
    cnt = np.zeros(m, dtype=np.uint32)
    rc = getattr(lib(), "aggregate_by_bitmap_" + group)(_p(pts), _p(fl), _p(off), C.c_size_t(n_sets), _p(b), C.c_size_t(m), _p(out), _p(oinf), _p(cnt))
    if rc == 2:
        raise ValueError("aggregate_by_bitmap_%s: bad arguments (code 2)" % group)
    if rc != 0:
        raise RuntimeError("aggregate_by_bitmap_%s failed with code %d" % (group, rc))
    return out, oinf, cnt


def aggregate_by_bitmap_dev(group, d_pk_xy, d_pk_inf, offsets, d_bits, m, d_out_xy, d_out_inf, d_out_count=0, stream=0):
    """The same on device buffers (data pointers; d_pk_inf and d_out_count may be 0 / None); offsets stays a host array.  Returns the code
    (0, or 2: nothing written)."""
    off = np.ascontiguousarray(offsets, dtype=np.uint32).reshape(-1)
    return getattr(lib(), "aggregate_by_bitmap_" + group + "_dev")(C.c_void_p(d_pk_xy), C.c_void_p(d_pk_inf or None), _p(off), C.c_size_t(off.shape[0] - 1),
                                                                  C.c_void_p(d_bits), C.c_size_t(m), C.c_void_p(d_out_xy), C.c_void_p(d_out_inf),
                                                                  C.c_void_p(d_out_count or None), C.c_void_p(stream))


def set_aggregate_lanes(lanes):
    """lanes per sum (0 = the rule of csrc/aggregate.h, else one of AGGREGATE_LANES)"""
    rc = lib().celo_amd_aggregate_set_lanes(C.c_int(lanes))
    if rc != 0:
        raise ValueError("celo_amd_aggregate_set_lanes(%d) failed with code %d" % (lanes, rc))


def set_aggregate_complement(mode):
    """-1 = the side rule, 0 = always sum the ones, 1 = the complement for every seal of a shared-set call"""
    rc = lib().celo_amd_aggregate_set_complement(C.c_int(mode))
    if rc != 0:
        raise ValueError("celo_amd_aggregate_set_complement(%d) failed with code %d" % (mode, rc))


def seals_last():
    """the last aggregate_by_bitmap / verify_aggregated_seals call: {path (-1: a bare sum; 0 each, 1 combined accepted, 2 combined rejected then
    each), lanes, ms: sums, decode, hash, combine, products, transfers, wall, count}"""
    path, lanes, ms = C.c_int(0), C.c_int(0), (C.c_float * 8)()
    assert lib().celo_amd_seals_last(C.byref(path), C.byref(lanes), ms) == 0
    return {"path": path.value, "lanes": lanes.value, "ms": dict(zip(("sums", "decode", "hash", "combine", "products", "transfers", "wall", "count"), list(ms)))}


def verify_aggregated_seals(pk_xy, pk_inf, offsets, bits, min_signers, domain, messages, extras, sigs, neg_g2_xy, hash_mode=0, mode=0, key=None):
    """m aggregated seals to verdicts (include/celo_bls_amd.h: verify_aggregated_seals_bls12_377).  pk_xy / pk_inf / offsets / bits as
    aggregate_by_bitmap (G2 keys); min_signers (m,) uint32 or None; messages / extras: lists of bytes (extras None = no extra data); sigs (m, 48)
    uint8 as serialize_signature writes them; hash_mode 0 direct, 2 composite, 3 composite CIP22; mode 0 each, 1 combined; key (8,) uint32 or
    None = OS randomness.  Returns (ok (m,) uint8, status (m,) uint8).  Raises ValueError on code 2."""
    m = len(messages)
    assert len(domain) == 8 and (extras is None or len(extras) == m)

    def pack(items):
        off = np.zeros(m + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(b) for b in items], dtype=np.uint64) if m else []
        return np.frombuffer(b"".join(items) or b"\0", dtype=np.uint8), off
    mdat, moff = pack(messages)
    edat, eoff = pack(extras) if extras is not None else (None, None)
    pts = _rows(pk_xy, 24)
    off = np.ascontiguousarray(offsets, dtype=np.uint32).reshape(-1)
    b = np.ascontiguousarray(bits, dtype=np.uint8)
    fl = None if pk_inf is None else np.ascontiguousarray(pk_inf, dtype=np.uint8)
    mins = None if min_signers is None else np.ascontiguousarray(min_signers, dtype=np.uint32)
    sg = np.ascontiguousarray(sigs, dtype=np.uint8).reshape(-1, 48)
    o = [int(v) for v in off]
    n_sets = off.shape[0] - 1
    if n_sets < 1 or any(hi < lo for lo, hi in zip(o, o[1:])) or pts.shape[0] < o[-1] or (fl is not None and fl.shape != (pts.shape[0],)) or \
            b.size != (m * (o[1] - o[0]) if n_sets == 1 else o[-1]) or sg.shape[0] != m or (mins is not None and mins.shape != (m,)):
        raise ValueError("verify_aggregated_seals_bls12_377: offsets, rows, bits, signatures and thresholds do not match")
    if pts.shape[0] == 0:
        pts = np.zeros((1, 24), dtype=np.uint64)
    if b.size == 0:
        b = np.zeros(1, dtype=np.uint8)
    k = None if key is None else np.ascontiguousarray(key, dtype=np.uint32).reshape(8)
    ng2 = np.ascontiguousarray(neg_g2_xy, dtype=np.uint64).reshape(24)
    dom = np.frombuffer(bytes(domain), dtype=np.uint8)
    ok = np.zeros(m, dtype=np.uint8)
    st = np.zeros(m, dtype=np.uint8)
    rc = lib().verify_aggregated_seals_bls12_377(_p(pts), _p(fl), _p(off), C.c_size_t(n_sets), _p(b), _p(mins), _p(dom), _p(mdat), _p(moff), _p(edat), _p(eoff),
                                                 C.c_int(hash_mode), _p(sg), _p(ng2), C.c_size_t(m), C.c_int(mode), _p(k), _p(ok), _p(st))
    if rc == 2:
        raise ValueError("verify_aggregated_seals_bls12_377: bad arguments (code 2)")
    if rc != 0:
        raise RuntimeError("verify_aggregated_seals_bls12_377 failed with code %d" % rc)
    return ok, st


# ---- epoch blocks to bytes, public inputs and verdicts (include/celo_bls_amd.h: epoch_*; csrc/epoch.h)
EPOCH_KINDS = {"first": 0, "last": 1, "inner": 2, "legacy": 3}
EPOCH_MAX_KEYS = 1 << 16


class EpochBlocksC(C.Structure):
    """celo_epoch_blocks"""
    _fields_ = [("index", C.c_void_p), ("round", C.c_void_p), ("max_non_signers", C.c_void_p), ("max_validators", C.c_void_p), ("epoch_entropy", C.c_void_p),
                ("parent_entropy", C.c_void_p), ("keys", C.c_void_p), ("keys_inf", C.c_void_p), ("key_off", C.c_void_p), ("keys_form", C.c_int)]


class EpochBlocks:
    """nb epoch blocks in the layout of celo_epoch_blocks.  index / round / max_non_signers / max_validators: (nb,) integers; epoch_entropy /
    parent_entropy: (nb, 16) uint8 or None (every entropy absent); key_off: (nb + 1,) uint32; keys: (key_off[nb], 96) uint8 compressed G2 keys
    (keys_form 0) or (key_off[nb], 24) uint64 affine rows with keys_inf (key_off[nb],) uint8 or None (keys_form 1).  Keeps the arrays alive."""
    def __init__(self, index, round_, max_non_signers, max_validators, epoch_entropy, parent_entropy, keys, key_off, keys_form=0, keys_inf=None):
        self.index = np.ascontiguousarray(index, dtype=np.uint16).reshape(-1)
        self.nb = self.index.shape[0]
        self.round = np.ascontiguousarray(round_, dtype=np.uint8).reshape(-1)
        self.mns = np.ascontiguousarray(max_non_signers, dtype=np.uint32).reshape(-1)
        self.maxv = np.ascontiguousarray(max_validators, dtype=np.uint32).reshape(-1)
        self.ee = None if epoch_entropy is None else np.ascontiguousarray(epoch_entropy, dtype=np.uint8).reshape(self.nb, 16)
        self.pe = None if parent_entropy is None else np.ascontiguousarray(parent_entropy, dtype=np.uint8).reshape(self.nb, 16)
        self.key_off = np.ascontiguousarray(key_off, dtype=np.uint32).reshape(-1)
        self.keys_form = int(keys_form)
        n = int(self.key_off[-1]) if self.key_off.size else 0
        if self.keys_form == 0:
            self.keys = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1, 96)
        else:
            self.keys = _rows(keys, 24)
        self.inf = None if keys_inf is None else np.ascontiguousarray(keys_inf, dtype=np.uint8).reshape(-1)
        if not (self.round.shape[0] == self.mns.shape[0] == self.maxv.shape[0] == self.nb and self.key_off.shape[0] == self.nb + 1 and self.keys.shape[0] >= n and
                (self.inf is None or self.inf.shape[0] >= n)):
            raise ValueError("EpochBlocks: the arrays do not match")
        if self.keys.shape[0] == 0:
            self.keys = np.zeros((1, self.keys.shape[1]), dtype=self.keys.dtype)      # (a pointer to pass: no key is read)
        self.c = EpochBlocksC(*[_p(a).value if a is not None else None for a in (self.index, self.round, self.mns, self.maxv, self.ee, self.pe, self.keys, self.inf,
                                                                                  self.key_off)], self.keys_form)

    def n_keys(self):
        return (self.key_off[1:].astype(np.int64) - self.key_off[:-1].astype(np.int64))


def epoch_encoded_size(kind, n_keys, max_validators):
    """bytes of one block of `kind` (0 .. 3 or a name of EPOCH_KINDS).  Raises ValueError on code 2."""
    out = C.c_uint64(0)
    rc = lib().epoch_encoded_size(C.c_int(EPOCH_KINDS.get(kind, kind)), C.c_uint64(n_keys), C.c_uint64(max_validators), C.byref(out))
    if rc != 0:
        raise ValueError("epoch_encoded_size: bad arguments (code %d)" % rc)
    return out.value


def _epoch_rc(name, rc):
    if rc == 2:
        raise ValueError("%s: bad arguments (code 2)" % name)
    if rc != 0:
        raise RuntimeError("%s failed with code %d" % (name, rc))


def epoch_encode_blocks(blocks, kind):
    """Every block of an EpochBlocks in the form `kind` -> (list of bytes, extras (nb, 7) uint8 or None, status (nb,) uint8, (msgs, msg_off) as the
    hash entry points take them).  A block whose status is 1 comes out as zero bytes."""
    kind = EPOCH_KINDS.get(kind, kind)
    nb = blocks.nb
    if kind not in (0, 1, 2, 3):
        raise ValueError("epoch_encode_blocks: kind is 0 .. 3")
    sizes = [epoch_encoded_size(kind, int(n), int(v)) for n, v in zip(blocks.n_keys(), blocks.maxv)]
    off = np.zeros(nb + 1, dtype=np.uint64)
    off[1:] = np.cumsum(sizes, dtype=np.uint64) if nb else []
    out = np.zeros(max(1, int(off[-1])), dtype=np.uint8)
    extras = np.zeros((nb, 7), dtype=np.uint8) if kind == 2 else None
    status = np.zeros(nb, dtype=np.uint8)
    _epoch_rc("epoch_encode_blocks_bls12_377", lib().epoch_encode_blocks_bls12_377(C.byref(blocks.c), C.c_size_t(nb), C.c_int(kind), _p(off), _p(out), _p(extras), _p(status)))
    return [out[int(off[i]):int(off[i + 1])].tobytes() for i in range(nb)], extras, status, (out, off)


def epoch_encode_blocks_dev(blocks_c, nb, kind, out_off, d_out, d_extras, d_status, stream=0):
    """The same with device keys / entropies (an EpochBlocksC whose keys, keys_inf and entropies are device addresses) and device outputs; returns the code."""
    off = np.ascontiguousarray(out_off, dtype=np.uint64)
    return lib().epoch_encode_blocks_bls12_377_dev(C.byref(blocks_c), C.c_size_t(nb), C.c_int(kind), _p(off), C.c_void_p(d_out), C.c_void_p(d_extras or None),
                                                   C.c_void_p(d_status), C.c_void_p(stream))


def epoch_public_inputs(first, last):
    """m (first, last) block pairs -> (inputs (m, 2, 6) uint64 canonical, status (m,) uint8: 0, 1 bad first block, 2 bad last block)"""
    m = first.nb
    if last.nb != m:
        raise ValueError("epoch_public_inputs: as many last blocks as first blocks")
    out = np.zeros((m, 2, 6), dtype=np.uint64)
    st = np.zeros(m, dtype=np.uint8)
    _epoch_rc("epoch_public_inputs_bw6_761", lib().epoch_public_inputs_bw6_761(C.byref(first.c), C.byref(last.c), C.c_size_t(m), _p(out), _p(st)))
    return out, st


def epoch_public_inputs_dev(first_c, last_c, m, d_out_inputs, d_out_status, stream=0):
    return lib().epoch_public_inputs_bw6_761_dev(C.byref(first_c), C.byref(last_c), C.c_size_t(m), C.c_void_p(d_out_inputs), C.c_void_p(d_out_status), C.c_void_p(stream))


def verify_epoch_proofs(vk, proofs, first, last, mode=0, key=None):
    """m serialized proofs (m x 288 bytes) of the epoch circuit under a VerifyingKey (BW6-761, two inputs) with their first and last blocks ->
    (ok (m,) uint8, status (m,) uint8: 0 accepted, 1 / 2 bad first / last block, 3 bad proof point, 4 product not one)"""
    m = first.nb
    buf = np.frombuffer(bytes(proofs) or b"\0", dtype=np.uint8)
    if last.nb != m or len(bytes(proofs)) != 288 * m:
        raise ValueError("verify_epoch_proofs: m first blocks, m last blocks, m x 288 proof bytes")
    k = None if key is None else np.ascontiguousarray(key, dtype=np.uint32).reshape(8)
    ok = np.zeros(m, dtype=np.uint8)
    st = np.zeros(m, dtype=np.uint8)
    _epoch_rc("verify_epoch_proofs_bw6_761", lib().verify_epoch_proofs_bw6_761(vk.h, _p(buf), C.byref(first.c), C.byref(last.c), C.c_size_t(m), C.c_int(mode), _p(k), _p(ok),
                                                                                _p(st)))
    return ok, st


def epoch_last():
    """the last epoch_* / verify_epoch_proofs call's times in ms (celo_amd_epoch_last)"""
    ms = (C.c_float * 8)()
    assert lib().celo_amd_epoch_last(ms) == 0
    return dict(zip(("decode", "sums", "pack", "hash", "transfers", "verify", "wall"), list(ms)[:7]))


TRANSITION_STATUS = ("accepted", "bad key", "bad signing set", "index", "key count", "parent entropy", "threshold", "padding key selected", "bad signature",
                     "no counter", "product")


def verify_epoch_transitions(blocks, chain_off, bits, sigs, domain, neg_g2_xy, mode=0, want=("status", "chain_ok", "crh", "attempts", "asig")):
    """Chains of epoch transitions to verdicts (include/celo_bls_amd.h: verify_epoch_transitions_bls12_377).  blocks: an EpochBlocks (round
    required); chain_off (n_chains + 1,) uint32; bits (key_off[nb],) uint8, the bytes under block p selecting the signers of block p + 1; sigs
    (nb, 48) uint8; mode 0 each, 1 chain product; want: the optional outputs to ask for.  Returns {ok (nb,), status (nb,), chain_ok (n_chains,),
    crh (nb, 48), attempts (nb,), asig_xy (n_chains, 12) uint64, asig_inf (n_chains,)}, the entries not asked for None.  Raises ValueError on code 2."""
    nb = blocks.nb
    co = np.ascontiguousarray(chain_off, dtype=np.uint32).reshape(-1)
    nc = co.shape[0] - 1
    b = np.ascontiguousarray(bits, dtype=np.uint8).reshape(-1)
    sg = np.ascontiguousarray(sigs, dtype=np.uint8).reshape(-1, 48)
    if nc < 0 or sg.shape[0] != nb or b.size != (int(blocks.key_off[-1]) if nb else 0):
        raise ValueError("verify_epoch_transitions_bls12_377: chain_off, bits and signatures do not match the blocks")
    if b.size == 0:
        b = np.zeros(1, dtype=np.uint8)
    if sg.shape[0] == 0:
        sg = np.zeros((1, 48), dtype=np.uint8)
    ng2 = np.ascontiguousarray(neg_g2_xy, dtype=np.uint64).reshape(24)
    dom = np.frombuffer(bytes(domain), dtype=np.uint8)
    assert dom.size == 8
    ok = np.zeros(nb, dtype=np.uint8)
    st = np.zeros(nb, dtype=np.uint8) if "status" in want else None
    cok = np.zeros(max(nc, 0), dtype=np.uint8) if "chain_ok" in want else None
    crh = np.zeros((nb, 48), dtype=np.uint8) if "crh" in want else None
    att = np.zeros(nb, dtype=np.uint8) if "attempts" in want else None
    axy = np.zeros((max(nc, 0), 12), dtype=np.uint64) if "asig" in want else None
    ainf = np.zeros(max(nc, 0), dtype=np.uint8) if "asig" in want else None
    _epoch_rc("verify_epoch_transitions_bls12_377", lib().verify_epoch_transitions_bls12_377(
        C.byref(blocks.c), C.c_size_t(nb), _p(co), C.c_size_t(max(nc, 0)), _p(b), _p(sg), _p(dom), _p(ng2), C.c_int(mode), _p(ok), _p(st), _p(cok), _p(crh), _p(att),
        _p(axy), _p(ainf)))
    return {"ok": ok, "status": st, "chain_ok": cok, "crh": crh, "attempts": att, "asig_xy": axy, "asig_inf": ainf}


def transitions_last():
    """the last verify_epoch_transitions call: {path (0 each, 1 every chain product held, 2 a chain fell back), ms: decode, sums, pack, hash, transfers,
    products, wall, signatures}"""
    path, ms = C.c_int(0), (C.c_float * 8)()
    assert lib().celo_amd_transitions_last(C.byref(path), ms) == 0
    return {"path": path.value, "ms": dict(zip(("decode", "sums", "pack", "hash", "transfers", "products", "wall", "signatures"), list(ms)))}


class SetupError(RuntimeError):
    def __init__(self, curve, code):
        super().__init__("groth16_setup_%s failed with code %d" % (curve, code))
        self.code = code


def groth16_setup(curve, qap_a, qap_b, qap_c, n_inputs, zt, tau, n_h, toxic, g1_xy, g2_xy, window_bits=0, want_vk=True, want_rows=True, want_key=False):
    """Groth16 parameters after the QAP evaluation at tau (groth16_setup_bw6_761 / _bls12_377).  curve: "bw6_761" (Fr 6 u64, G1 rows 24) or
    "bls12_377" (Fr 4 u64, G1 rows 12); qap_*: (n_vars, 6 | 4) Montgomery limbs; zt, tau: one Montgomery element each; toxic: alpha, beta, gamma,
    delta (4 elements).  Returns {"vk": {alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1}, "rows": {beta_g1, delta_g1, a_query, b_g1_query,
    b_g2_query, h_query, l_query}, "key": ProvingKey or None}."""
    N, R1 = (6, 24) if curve == "bw6_761" else (4, 12)
    qa, qb, qc = (np.ascontiguousarray(q, dtype=np.uint64).reshape(-1, N) for q in (qap_a, qap_b, qap_c))
    n_vars = qa.shape[0]
    z = np.ascontiguousarray(zt, dtype=np.uint64).reshape(N)
    t = np.ascontiguousarray(tau, dtype=np.uint64).reshape(N)
    tox = np.ascontiguousarray(toxic, dtype=np.uint64).reshape(4 * N)
    g1 = np.ascontiguousarray(g1_xy, dtype=np.uint64).reshape(R1)
    g2 = np.ascontiguousarray(g2_xy, dtype=np.uint64).reshape(24)
    n_l = max(n_vars - n_inputs, 0)
    vk = np.zeros(R1 + 3 * 24 + n_inputs * R1, dtype=np.uint64) if want_vk else None
    rows = np.zeros(2 * R1 + 2 * n_vars * R1 + n_vars * 24 + (n_h + n_l) * R1, dtype=np.uint64) if want_rows else None
    key = ProvingKey(curve, None, None, None, None, None, None) if want_key else None
    fn = getattr(lib(), "groth16_setup_" + curve)
    rc = fn(_p(qa), _p(qb), _p(qc), C.c_size_t(n_vars), C.c_size_t(n_inputs), _p(z), _p(t), C.c_size_t(n_h), _p(tox), _p(g1), _p(g2),
            C.c_int(window_bits), _p(vk), _p(rows), C.byref(key.h) if key is not None else None)
    if rc != 0:
        raise SetupError(curve, rc)
    return _setup_outputs(vk, rows, key, n_vars, n_inputs, n_h, R1)


def _setup_outputs(vk, rows, key, n_vars, n_inputs, n_h, R1):
    """the flat vk / rows buffers of groth16_setup_* -> the dict groth16_setup documents"""
    n_l = max(n_vars - n_inputs, 0)
    out = {"vk": None, "rows": None, "key": key}
    if vk is not None:
        out["vk"] = {"alpha_g1": vk[:R1].copy(), "beta_g2": vk[R1:R1 + 24].copy(), "gamma_g2": vk[R1 + 24:R1 + 48].copy(),
                     "delta_g2": vk[R1 + 48:R1 + 72].copy(), "gamma_abc_g1": vk[R1 + 72:].reshape(n_inputs, R1).copy()}
    if rows is not None:
        o, d = 0, {}
        for name, k, w in (("beta_g1", 1, R1), ("delta_g1", 1, R1), ("a_query", n_vars, R1), ("b_g1_query", n_vars, R1), ("b_g2_query", n_vars, 24),
                           ("h_query", n_h, R1), ("l_query", n_l, R1)):
            d[name] = rows[o:o + k * w].reshape(k, w).copy()
            o += k * w
        d["beta_g1"], d["delta_g1"] = d["beta_g1"][0], d["delta_g1"][0]
        out["rows"] = d
    return out


# ---- R1CS matrices on the device (include/celo_bls_amd.h: groth16_r1cs_*, groth16_prove_r1cs_with_key, groth16_setup_r1cs_*)
R1CS_ERR_MATRIX = 34
# csrc/r1cs.h (tests/test_r1cs_host.py checks them against the built twin): a list of more than R1CS_LONG entries is cut into chunks of R1CS_CHUNK
R1CS_LONG, R1CS_CHUNK = 128, 1024


class R1CSLoadError(RuntimeError):
    def __init__(self, curve, code, first_bad=None):
        super().__init__("groth16_r1cs_load_%s failed with code %d%s"
                         % (curve, code, "" if first_bad is None else " (matrix %d, index %d)" % (first_bad >> 60, first_bad & ((1 << 60) - 1))))
        self.code = code
        self.first_bad = first_bad


def _csr_args(mats, N):
    """three (row_ptr, col, val) -> the contiguous arrays and the argument list of groth16_r1cs_load_* / ht_r1cs_validate"""
    keep, args = [], []
    for row_ptr, col, val in mats:
        rp = np.ascontiguousarray(row_ptr, dtype=np.uint64)
        cc = np.ascontiguousarray(col, dtype=np.uint32)
        vv = np.ascontiguousarray(val, dtype=np.uint64).reshape(-1, N)
        keep.append((rp, cc, vv))
        args += [_p(rp), _p(cc), _p(vv), C.c_size_t(cc.shape[0])]
    return keep, args


class R1CS:
    """Constraint matrices on the device (groth16_r1cs_load_*): load once, then rows() / check() per assignment and qap_at_tau() per setup.
    mats: three (row_ptr (m + 1,) uint64, col (nnz,) uint32, val (nnz, 6 | 4) uint64 Montgomery limbs) in a, b, c order."""
    def __init__(self, curve, n_constraints, n_vars, n_inputs, mats):
        self.curve, self.m, self.n_vars, self.n_inputs = curve, n_constraints, n_vars, n_inputs
        self.N = 6 if curve == "bw6_761" else 4
        self.h = C.c_void_p()
        keep, args = _csr_args(mats, self.N)
        for rp, _, _ in keep:
            assert rp.shape[0] == n_constraints + 1
        bad = C.c_uint64(0)
        rc = getattr(lib(), "groth16_r1cs_load_" + curve)(C.c_size_t(n_constraints), C.c_size_t(n_vars), C.c_size_t(n_inputs), *args, C.byref(self.h), C.byref(bad))
        if rc != 0:
            self.h = C.c_void_p()
            raise R1CSLoadError(curve, rc, bad.value if rc == R1CS_ERR_MATRIX else None)

    @classmethod
    def load(cls, curve, n_constraints, n_vars, n_inputs, mats):
        return cls(curve, n_constraints, n_vars, n_inputs, mats)

    def info(self):
        out = np.zeros(8, dtype=np.uint64)
        rc = lib().groth16_r1cs_info(self.h, _p(out))
        if rc != 0:
            raise RuntimeError("groth16_r1cs_info failed with code %d" % rc)
        return dict(zip(("curve", "n_constraints", "n_vars", "n_inputs", "nnz_a", "nnz_b", "nnz_c", "device_bytes"), (int(v) for v in out)))

    def _z(self, z):
        zz = np.ascontiguousarray(z, dtype=np.uint64).reshape(-1, self.N)
        assert zz.shape[0] == self.n_vars
        return zz

    def rows(self, z, log_n):
        """(A z, B z, C z) over 2^log_n rows with the input-consistency rows: three (2^log_n, 6 | 4) uint64 arrays (groth16_r1cs_rows)"""
        zz = self._z(z)
        out = [np.zeros((1 << log_n, self.N), dtype=np.uint64) for _ in range(3)]
        rc = lib().groth16_r1cs_rows(self.h, _p(zz), C.c_uint(log_n), _p(out[0]), _p(out[1]), _p(out[2]))
        if rc != 0:
            raise RuntimeError("groth16_r1cs_rows failed with code %d" % rc)
        return out

    def rows_dev(self, d_z, log_n, d_a, d_b, d_c, stream=0):
        rc = lib().groth16_r1cs_rows_dev(self.h, C.c_void_p(d_z), C.c_uint(log_n), C.c_void_p(d_a), C.c_void_p(d_b), C.c_void_p(d_c), C.c_void_p(stream or 0))
        if rc != 0:
            raise RuntimeError("groth16_r1cs_rows_dev failed with code %d" % rc)

    def check(self, z):
        """the smallest unsatisfied constraint, or -1 (groth16_r1cs_check)"""
        zz = self._z(z)
        first = C.c_int64(0)
        rc = lib().groth16_r1cs_check(self.h, _p(zz), C.byref(first))
        if rc != 0:
            raise RuntimeError("groth16_r1cs_check failed with code %d" % rc)
        return first.value

    def qap_at_tau(self, log_n, omega, tau):
        """(a, b, c (n_vars, 6 | 4), zt (6 | 4,)): the four inputs of groth16_setup (groth16_r1cs_qap_at_tau); omega, tau: Montgomery limbs"""
        w = np.ascontiguousarray(omega, dtype=np.uint64).reshape(self.N)
        t = np.ascontiguousarray(tau, dtype=np.uint64).reshape(self.N)
        out = [np.zeros((self.n_vars, self.N), dtype=np.uint64) for _ in range(3)]
        zt = np.zeros(self.N, dtype=np.uint64)
        rc = lib().groth16_r1cs_qap_at_tau(self.h, C.c_uint(log_n), _p(w), _p(t), _p(out[0]), _p(out[1]), _p(out[2]), _p(zt))
        if rc != 0:
            raise RuntimeError("groth16_r1cs_qap_at_tau failed with code %d" % rc)
        return out[0], out[1], out[2], zt

    def qap_at_tau_dev(self, log_n, omega, tau, d_a, d_b, d_c, stream=0):
        """the same into device buffers; returns zt"""
        w = np.ascontiguousarray(omega, dtype=np.uint64).reshape(self.N)
        t = np.ascontiguousarray(tau, dtype=np.uint64).reshape(self.N)
        zt = np.zeros(self.N, dtype=np.uint64)
        rc = lib().groth16_r1cs_qap_at_tau_dev(self.h, C.c_uint(log_n), _p(w), _p(t), C.c_void_p(d_a), C.c_void_p(d_b), C.c_void_p(d_c), _p(zt), C.c_void_p(stream or 0))
        if rc != 0:
            raise RuntimeError("groth16_r1cs_qap_at_tau_dev failed with code %d" % rc)
        return zt

    def release(self):
        if self.h:
            lib().groth16_r1cs_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


def r1cs_timings():
    """the last R1CS calls: {load, rows, lagrange, columns, prove_r1cs_wall, setup_r1cs_wall} in ms"""
    ms = (C.c_float * 8)()
    lib().celo_amd_r1cs_last_timings(ms)
    return dict(zip(("load", "rows", "lagrange", "columns", "prove_r1cs_wall", "setup_r1cs_wall"), list(ms)[:6]))


def groth16_setup_r1cs(r1cs, log_n, omega, tau, toxic, g1_xy, g2_xy, window_bits=0, want_vk=True, want_rows=True, want_key=False):
    """Groth16 parameters from the matrices (groth16_setup_r1cs_*): the QAP at tau on the device, then groth16_setup with n_h = 2^log_n - 1.
    Returns what groth16_setup returns."""
    curve, N = r1cs.curve, r1cs.N
    R1 = 24 if curve == "bw6_761" else 12
    n_vars, n_inputs, n_h = r1cs.n_vars, r1cs.n_inputs, (1 << log_n) - 1
    w = np.ascontiguousarray(omega, dtype=np.uint64).reshape(N)
    t = np.ascontiguousarray(tau, dtype=np.uint64).reshape(N)
    tox = np.ascontiguousarray(toxic, dtype=np.uint64).reshape(4 * N)
    g1 = np.ascontiguousarray(g1_xy, dtype=np.uint64).reshape(R1)
    g2 = np.ascontiguousarray(g2_xy, dtype=np.uint64).reshape(24)
    n_l = n_vars - n_inputs
    vk = np.zeros(R1 + 3 * 24 + n_inputs * R1, dtype=np.uint64) if want_vk else None
    rows = np.zeros(2 * R1 + 2 * n_vars * R1 + n_vars * 24 + (n_h + n_l) * R1, dtype=np.uint64) if want_rows else None
    key = ProvingKey(curve, None, None, None, None, None, None) if want_key else None
    rc = getattr(lib(), "groth16_setup_r1cs_" + curve)(r1cs.h, C.c_uint(log_n), _p(w), _p(t), _p(tox), _p(g1), _p(g2), C.c_int(window_bits), _p(vk), _p(rows),
                                                       C.byref(key.h) if key is not None else None)
    if rc != 0:
        raise SetupError(curve, rc)
    return _setup_outputs(vk, rows, key, n_vars, n_inputs, n_h, R1)


# ---- the HashToBits circuit of the hash-helper proof over BLS12-377 (include/celo_bls_amd.h: hash_to_bits_*, groth16_hash_helper_prove_bls12_377)
HASH_TO_BITS_SIZE_KEYS = ("n_constraints", "n_vars", "n_inputs", "nnz_a", "nnz_b", "nnz_c", "log_n", "stride")


def hash_to_bits_size(n_epochs):
    """(rc, sizes) of the circuit for n_epochs messages (hash_to_bits_r1cs_size_bls12_377; host only): sizes a dict of HASH_TO_BITS_SIZE_KEYS"""
    out = np.zeros(8, dtype=np.uint64)
    rc = lib().hash_to_bits_r1cs_size_bls12_377(C.c_size_t(n_epochs), _p(out))
    return rc, dict(zip(HASH_TO_BITS_SIZE_KEYS, (int(v) for v in out)))


def _hb_size(n_epochs):
    rc, s = hash_to_bits_size(n_epochs)
    if rc != 0:
        raise RuntimeError("hash_to_bits_r1cs_size_bls12_377(%d) failed with code %d" % (n_epochs, rc))
    return s


def hash_to_bits_r1cs(n_epochs):
    """(sizes, [(row_ptr, col, val (nnz, 4))] for a, b, c): the matrices on the host (hash_to_bits_r1cs_bls12_377)"""
    s = _hb_size(n_epochs)
    mats, args = [], []
    for k in "abc":
        rp = np.zeros(s["n_constraints"] + 1, dtype=np.uint64)
        col = np.zeros(s["nnz_" + k], dtype=np.uint32)
        val = np.zeros((s["nnz_" + k], 4), dtype=np.uint64)
        mats.append((rp, col, val))
        args += [_p(rp), _p(col), _p(val)]
    rc = lib().hash_to_bits_r1cs_bls12_377(C.c_size_t(n_epochs), *args)
    if rc != 0:
        raise RuntimeError("hash_to_bits_r1cs_bls12_377 failed with code %d" % rc)
    return s, mats


def _hb_rows(rows48, n=None):
    r = np.ascontiguousarray(np.frombuffer(rows48, dtype=np.uint8) if isinstance(rows48, (bytes, bytearray)) else rows48, dtype=np.uint8).reshape(-1, 48)
    assert n is None or r.shape[0] == n
    return r


def hash_to_bits_r1cs_load(n_epochs):
    """the circuit as an R1CS handle of curve bls12_377 (hash_to_bits_r1cs_load_bls12_377)"""
    s = _hb_size(n_epochs)
    r = R1CS.__new__(R1CS)
    r.curve, r.m, r.n_vars, r.n_inputs, r.N = "bls12_377", s["n_constraints"], s["n_vars"], s["n_inputs"], 4
    r.h = C.c_void_p()
    rc = lib().hash_to_bits_r1cs_load_bls12_377(C.c_size_t(n_epochs), C.byref(r.h))
    if rc != 0:
        r.h = C.c_void_p()
        raise R1CSLoadError("bls12_377", rc)
    return r


def hash_to_bits_assignment(rows48, bit_order=0, host=False):
    """the full assignment (n_vars, 4) of the messages in rows48 ((m, 48) bytes): on the device (hash_to_bits_assignment_bls12_377) or, with
    host=True, by the host twin (celo_amd_hash_to_bits_assignment_host)"""
    r = _hb_rows(rows48)
    s = _hb_size(r.shape[0])
    z = np.zeros((s["n_vars"], 4), dtype=np.uint64)
    fn = lib().celo_amd_hash_to_bits_assignment_host if host else lib().hash_to_bits_assignment_bls12_377
    rc = fn(_p(r), C.c_size_t(r.shape[0]), C.c_int(bit_order), _p(z))
    if rc != 0:
        raise RuntimeError("hash_to_bits assignment (%s) failed with code %d" % ("host" if host else "device", rc))
    return z


def hash_to_bits_assignment_dev(d_rows48, n_epochs, bit_order, d_z, stream=0):
    rc = lib().hash_to_bits_assignment_bls12_377_dev(C.c_void_p(d_rows48), C.c_size_t(n_epochs), C.c_int(bit_order), C.c_void_p(d_z), C.c_void_p(stream or 0))
    if rc != 0:
        raise RuntimeError("hash_to_bits_assignment_bls12_377_dev failed with code %d" % rc)


def hash_to_bits_public_inputs(rows48, n_proofs, n_epochs, bit_order=0):
    """(n_proofs, n_inputs - 1, 4) canonical limbs: the inputs of groth16_verify_batch_bls12_377 (hash_to_bits_public_inputs_bls12_377)"""
    r = _hb_rows(rows48, n_proofs * n_epochs)
    s = _hb_size(n_epochs)
    out = np.zeros((n_proofs, s["n_inputs"] - 1, 4), dtype=np.uint64)
    rc = lib().hash_to_bits_public_inputs_bls12_377(_p(r), C.c_size_t(n_proofs), C.c_size_t(n_epochs), C.c_int(bit_order), _p(out))
    if rc != 0:
        raise RuntimeError("hash_to_bits_public_inputs_bls12_377 failed with code %d" % rc)
    return out


def hash_to_bits_public_inputs_dev(d_rows48, n_proofs, n_epochs, bit_order, d_out, stream=0):
    rc = lib().hash_to_bits_public_inputs_bls12_377_dev(C.c_void_p(d_rows48), C.c_size_t(n_proofs), C.c_size_t(n_epochs), C.c_int(bit_order), C.c_void_p(d_out),
                                                        C.c_void_p(stream or 0))
    if rc != 0:
        raise RuntimeError("hash_to_bits_public_inputs_bls12_377_dev failed with code %d" % rc)


def hash_helper_prove_rc(key, r1cs, rows48, bit_order, log_n, consts):
    """(rc, A, B, C, inputs) of groth16_hash_helper_prove_bls12_377: the return code with the outputs (Jacobian limbs; inputs (n_inputs - 1, 4) canonical)"""
    r = _hb_rows(rows48)
    s = _hb_size(r.shape[0])
    k = [np.ascontiguousarray(consts[n], dtype=np.uint64).reshape(4) for n in ("omega", "omega_inv", "coset", "coset_inv", "size_inv", "vanishing_inv")]
    out = [np.zeros(w, dtype=np.uint64) for w in (18, 36, 18)]
    inputs = np.zeros((s["n_inputs"] - 1, 4), dtype=np.uint64)
    rc = lib().groth16_hash_helper_prove_bls12_377(key.h, r1cs.h, _p(r), C.c_size_t(r.shape[0]), C.c_int(bit_order), C.c_uint(log_n), *[_p(x) for x in k],
                                                   _p(out[0]), _p(out[1]), _p(out[2]), _p(inputs))
    return rc, out[0], out[1], out[2], inputs


def hash_helper_prove(key, r1cs, rows48, bit_order, log_n, consts):
    """generate_hash_helper in one call: (A, B, C, inputs)"""
    rc, a, b, c, inputs = hash_helper_prove_rc(key, r1cs, rows48, bit_order, log_n, consts)
    if rc != 0:
        raise RuntimeError("groth16_hash_helper_prove_bls12_377 failed with code %d" % rc)
    return a, b, c, inputs


def hash_helper_verify(vk, rows48, n_epochs, proofs, bit_order=0, mode=0, key=None):
    """The verifier's side of generate_hash_helper in one call (groth16_hash_helper_verify_bls12_377): vk a BLS12-377 VerifyingKey of
    n_inputs(n_epochs) - 1 inputs, rows48 (n_proofs x n_epochs, 48) CRH rows, proofs n_proofs x 192 serialized bytes -> uint8 [n_proofs] verdicts.
    Raises VerifyError (.code)."""
    buf = np.frombuffer(bytes(proofs), dtype=np.uint8)
    assert buf.size % 192 == 0
    n_proofs = buf.size // 192
    r = np.ascontiguousarray(rows48, dtype=np.uint8).reshape(-1, 48)
    assert r.shape[0] == n_proofs * n_epochs, "rows48: n_proofs x n_epochs rows of 48 bytes"
    k = None if key is None else np.ascontiguousarray(key, dtype=np.uint32).reshape(8)
    out = np.zeros(n_proofs, dtype=np.uint8)
    rc = lib().groth16_hash_helper_verify_bls12_377(vk.h, _p(r), C.c_size_t(n_proofs), C.c_size_t(n_epochs), C.c_int(bit_order), _p(buf), C.c_int(mode), _p(k), _p(out))
    if rc != 0:
        raise VerifyError("groth16_hash_helper_verify_bls12_377", rc)
    return out


def hash_helper_last():
    """the last groth16_hash_helper_prove_bls12_377 call: {trace, expand, pack, prove, wall} in ms"""
    ms = (C.c_float * 8)()
    lib().celo_amd_hash_helper_last(ms)
    return dict(zip(("trace", "expand", "pack", "prove", "wall"), list(ms)[:5]))
