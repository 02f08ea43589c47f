"""GPU: a serialized ark-groth16 0.1 ProvingKey<BW6_761> loaded by groth16_load_key_bw6_761_serialized (decoded and checked on the device,
straight into the fixed-base tables) proves exactly what the limb-loaded key and groth16_prove_bw6_761 prove; rejected points, truncation and
the cleanup of failed loads.  The key is synthetic and serialized by tests/bw6_serial.py: the reference ships no serialized ProvingKey."""
import ctypes as C
import numpy as np
import pytest
import torch  # before the library: both must share one HIP runtime
from oracle.py import ecc
from oracle import cpu_oracle as co
import bw6_serial as bs

pytestmark = pytest.mark.gpu
N_INPUTS, N_AUX, N_H = 2, 4094, 4095


@pytest.fixture(scope="module")
def key_parts(gpu):
    from celo_bls_snark_rs_amd import synthetic as syn
    vk = bs.reference_vk()
    E1, E2 = ecc.E1_761, ecc.E2_761
    alpha, beta = ecc.deser_point(E1, vk[0:96]), ecc.deser_point(E2, vk[96:192])
    n_abc = int.from_bytes(vk[384:392], "little")

    def pts(group, k, seed):
        return syn.device_points(group, k, seed).cpu().numpy().view(np.uint64).reshape(k, 24)
    n_assign = N_INPUTS + N_AUX
    rows = {"a_query": pts("bw6_761_g1", n_assign + 1, 31), "b_g1_query": pts("bw6_761_g1", n_assign + 1, 32),
            "b_g2_query": pts("bw6_761_g2", n_assign + 1, 33), "h_query": pts("bw6_761_g1", N_H, 34), "l_query": pts("bw6_761_g1", N_AUX, 35)}
    one = co.to_mont([1], ecc.Q761)[0]
    zero_row = np.concatenate([np.zeros(12, dtype=np.uint64), one])
    for name, idx in (("a_query", (0, 6, 1000)), ("b_g2_query", (8, 1001)), ("l_query", (4, 3499))):   # identity rows (query[0] included)
        for i in idx:
            rows[name][i] = zero_row
    key = {"alpha_g1": alpha, "beta_g2": beta, "gamma_g2": ecc.deser_point(E2, vk[192:288]), "delta_g2": ecc.deser_point(E2, vk[288:384]),
           "gamma_abc_g1": [ecc.deser_point(E1, vk[392 + 96 * i:488 + 96 * i]) for i in range(n_abc)],
           "beta_g1": E1.mul(alpha, 3), "delta_g1": E1.mul(alpha, 5)}
    for name, r in rows.items():
        key[name] = [None if np.array_equal(row, zero_row) else P for row, P in zip(r, bs.rows_to_points(r))]
    asg = syn.witness_like_scalars("bw6_761_g1", n_assign, 36)
    h = syn.uniform_scalars("bw6_761_g1", N_H, 37)
    return {"key": key, "rows": rows, "alpha": co.pack_761([alpha])[0][0], "beta": co.pack_761([beta])[0][0], "asg": asg, "h": h}


@pytest.mark.wall_clock(900)
def test_serialized_key_proves_like_the_limb_loaded_key(gpu, key_parts):
    kp, r = key_parts, key_parts["rows"]
    want = gpu.groth16_prove(r["a_query"], r["b_g2_query"], r["h_query"], r["l_query"], kp["alpha"], kp["beta"], kp["asg"], N_AUX, kp["h"])
    limb_key = gpu.ProvingKey("bw6_761", r["a_query"], r["b_g2_query"], r["h_query"], r["l_query"], kp["alpha"], kp["beta"])
    limb = limb_key.prove(kp["asg"], N_AUX, kp["h"])
    limb_key.release()
    for form in (0, 1, 2):
        data = bs.ser_key(kp["key"], form)
        rc, layout = gpu.groth16_key_layout(data, form)
        assert rc == 0 and int(layout[15]) == len(bs.key_point_order(kp["key"]))
        key = gpu.ProvingKey.from_serialized(data, form)
        got = key.prove(kp["asg"], N_AUX, kp["h"])
        key.release()
        for g, l_, w in zip(got, limb, want):                                    # A, B, C as affine points (Jacobian Z is not canonical)
            assert co.jac_to_affine(g, "761") == co.jac_to_affine(l_, "761") == co.jac_to_affine(w, "761"), form
        ms = gpu.wire761_last_timings()
        assert ms[2] > 0 and ms[3] > 0


def _spoil(kp, section, index):
    """the key with one point of `section` replaced by a curve point outside the subgroup; its index in serialization order"""
    key = dict(kp["key"])
    bad = bs.random_curve_points(ecc.E2_761 if section in bs.G2_FIELDS else ecc.E1_761, 1, 41)[0]
    if isinstance(key[section], list):
        key[section] = list(key[section])
        key[section][index] = bad
    else:
        key[section] = bad
    return key, bs.key_point_order(key).index((section, index))


@pytest.mark.wall_clock(900)
def test_rejected_points_and_truncation(gpu, key_parts):
    for section, index in (("b_g1_query", 123), ("delta_g1", 0)):
        key, where = _spoil(key_parts, section, index)
        for form in (0, 1):
            with pytest.raises(gpu.KeyLoadError) as e:
                gpu.ProvingKey.from_serialized(bs.ser_key(key, form), form)
            assert e.value.code == gpu.KEY_ERR_POINT and e.value.first_bad_point == where, (section, form)
        k = gpu.ProvingKey.from_serialized(bs.ser_key(key, 2), 2)             # unchecked: loads
        k.release()
    data = bs.ser_key(key_parts["key"], 0)
    with pytest.raises(gpu.KeyLoadError) as e:
        gpu.ProvingKey.from_serialized(data[:-50], 0)
    assert e.value.code == gpu.KEY_ERR_TRUNCATED


@pytest.mark.wall_clock(900)
def test_failed_loads_leak_nothing(gpu, key_parts):
    key, where = _spoil(key_parts, "l_query", 77)
    data = np.frombuffer(bs.ser_key(key, 0), dtype=np.uint8)
    lib = gpu.lib()

    def fail_once():
        h = C.c_void_p(0x1234)
        bad = C.c_uint64(0)
        rc = lib.groth16_load_key_bw6_761_serialized(data.ctypes.data_as(C.c_void_p), C.c_size_t(data.size), C.c_int(0), C.c_int(0),
                                                     C.byref(h), C.byref(bad))
        assert rc == gpu.KEY_ERR_POINT and bad.value == where and h.value is None
    torch.cuda.synchronize()
    fail_once()
    free_1 = torch.cuda.mem_get_info()[0]
    for _ in range(10):
        fail_once()
    free_11 = torch.cuda.mem_get_info()[0]
    assert free_1 - free_11 <= 2 << 20, (free_1, free_11)
