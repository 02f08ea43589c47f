"""GPU: the byte boundary of a Groth16 proving key over BLS12-377.  groth16_setup_r1cs_bls12_377 -> groth16_serialize_key (bytes equal
to the Python serializer's, tests/bls377_serial.py) -> ProvingKey.from_serialized(curve="bls12_377") in all three forms -> prove_r1cs -> a
serialized proof that the VerifyingKey loaded from the key's own prefix accepts; rejected points in every section class, truncation, and the
cleanup of failed loads.

Keys: r1cs_cases.toy (6 variables), chain(62) (64 variables: a_query, b_g1_query and b_g2_query fill one 64-lane block exactly, h_query and
l_query are one and two short of it) and chain(70) (72 variables: every query runs into a second block).  All have arkworks-zero rows."""
import ctypes as C
import random
import numpy as np
import pytest
import torch  # before the library: both must share one HIP runtime
from oracle.py import groth16_prover as gp
from oracle import cpu_oracle as co
import groth16_setup_ref as gs
import r1cs_cases as rc
import bls377_serial as bs
from groth16_verify377_cases import off_subgroup_point

pytestmark = pytest.mark.gpu
CURVE = "bls12_377"
P_FR = gs.FIELDS[CURVE]
CASES = {"toy": lambda: rc.toy(CURVE), "chain62": lambda: rc.chain(CURVE, 62), "chain70": lambda: rc.chain(CURVE, 70)}
_SETUPS = {}


def setup(gpu, name):
    """one setup per circuit for the whole module: the circuit on the device, vk / rows as limbs, the setup's own handle, the key as python
    points and its serializations"""
    if name in _SETUPS:
        return _SETUPS[name]
    case = CASES[name]()
    log_n = case.log_n()
    r = gpu.R1CS.load(CURVE, case.m, case.n_vars, case.n_inputs, case.csr())
    rng = random.Random(377)
    tau, toxic = rng.randrange(2, P_FR), [rng.randrange(1, P_FR) for _ in range(4)]
    out = gpu.groth16_setup_r1cs(r, log_n, rc.mont([gs.root_of_unity(CURVE, log_n)], P_FR)[0], rc.mont([tau], P_FR)[0], rc.mont(toxic, P_FR),
                                 gs.pack(CURVE, 1, [gs.generators(CURVE)[0]])[0][0], gs.pack(CURVE, 2, [gs.generators(CURVE)[1]])[0][0],
                                 want_rows=True, want_key=True)
    key = {}
    for part in (out["vk"], out["rows"]):
        for sec, rows in part.items():
            pts = bs.rows_to_points(bs.E2 if sec in bs.G2_FIELDS else bs.E1, rows, ark_zero=True)
            key[sec] = pts if rows.ndim == 2 else pts[0]
    k = gp.domain_constants(log_n, gs.root_of_unity(CURVE, log_n), gs.coset_generator(P_FR), P_FR)
    z = gs.toy_witness(7, P_FR) if name == "toy" else gs.squaring_witness(case.m, 7, P_FR)
    s = {"case": case, "r": r, "log_n": log_n, "out": out, "key": key, "n_h": (1 << log_n) - 1, "z": z,
         "consts": {n: co.to_mont([v], P_FR)[0] for n, v in k.items()}, "bytes": {f: bs.ser_key(key, f) for f in (0, 1)}}
    if name != "toy":       # no constraint of a squaring chain has the one or the output in b: b_g2_query begins with arkworks-zero rows
        assert key["b_g2_query"][0] is None and key["b_g1_query"][1] is None and any(P is not None for P in key["b_g2_query"])
    _SETUPS[name] = s
    return s


def affine(out):
    return tuple(co.jac_to_affine(o, k) for o, k in zip(out, ("g1_377", "g2_377", "g1_377")))


@pytest.mark.parametrize("name", list(CASES))
def test_writer_equals_the_python_serializer(gpu, name):
    s = setup(gpu, name)
    case, out = s["case"], s["out"]
    for form in (0, 1):
        data = gpu.groth16_serialize_key(out["vk"], out["rows"], case.n_vars, s["n_h"], form, curve=CURVE)
        assert data == s["bytes"][form], form
        vk_only = gpu.groth16_serialize_key(out["vk"], form=form, curve=CURVE)
        assert vk_only == bs.ser_key(s["key"], form, bs.SECTIONS[:5]) and data.startswith(vk_only)
        rc_, lay = gpu.groth16_key_layout(data, form, curve=CURVE)
        assert rc_ == 0 and int(lay[15]) == len(bs.key_point_order(s["key"])) and int(lay[14]) == len(vk_only)
        if form == 0:
            assert len(vk_only) == 7 * 48 + 8 + 48 * case.n_inputs
            vk = gpu.VerifyingKey.from_serialized(vk_only, curve=CURVE)           # the prefix is a VerifyingKey::serialize
            assert vk.n_inputs == case.n_inputs - 1
            vk.release()
    with pytest.raises(gpu.KeySerializeError) as e:
        gpu.groth16_serialize_key(out["vk"], out["rows"], case.n_vars, s["n_h"], 0, cap=len(s["bytes"][0]) - 1, curve=CURVE)
    assert e.value.code == gpu.KEY_ERR_CAPACITY and e.value.out_len == len(s["bytes"][0])


@pytest.mark.parametrize("name", list(CASES))
def test_round_trip_proves_and_verifies(gpu, name):
    s = setup(gpu, name)
    case, out, r, rows = s["case"], s["out"], s["r"], s["out"]["rows"]
    z = rc.mont(s["z"], P_FR)
    bad = list(s["z"])
    bad[3] = (bad[3] + 1) % P_FR
    assert r.check(z) == -1 and r.check(rc.mont(bad, P_FR)) >= 0
    want = affine(out["key"].prove_r1cs(r, z, s["log_n"], s["consts"]))
    limb_key = gpu.ProvingKey(CURVE, rows["a_query"], rows["b_g2_query"], rows["h_query"], rows["l_query"], out["vk"]["alpha_g1"], out["vk"]["beta_g2"])
    assert affine(limb_key.prove_r1cs(r, z, s["log_n"], s["consts"])) == want
    limb_key.release()
    vk = gpu.VerifyingKey.from_serialized(bs.ser_key(s["key"], 0, bs.SECTIONS[:5]), curve=CURVE)
    public = co.ints_to_limbs(s["z"][1:case.n_inputs], 4).reshape(1, case.n_inputs - 1, 4)
    for form in (0, 1, 2):
        key = gpu.ProvingKey.from_serialized(s["bytes"][min(form, 1)], form, curve=CURVE)
        proof = key.prove_r1cs(r, z, s["log_n"], s["consts"])
        assert affine(proof) == want, form                                     # A, B, C as affine points (Jacobian Z is not canonical)
        assert vk.verify_serialized(gpu.groth16_serialize_proof(*proof, curve=CURVE), public).tolist() == [1], form
        wrong = key.prove_r1cs(r, rc.mont(bad, P_FR), s["log_n"], s["consts"])
        assert vk.verify_serialized(gpu.groth16_serialize_proof(*wrong, curve=CURVE), public).tolist() == [0], form
        key.release()
        ms = gpu.wire761_last_timings()
        assert ms[2] > 0 and ms[3] > 0
    vk.release()


def _load_fails(gpu, data, form):
    with pytest.raises(gpu.KeyLoadError) as e:
        gpu.ProvingKey.from_serialized(data, form, curve=CURVE)
    return e.value


# one point of every section class: (section, index in it); chain70 has 72 variables, so a_query[30] sits mid-block, b_g2_query[63] and [64] on
# the two sides of the 64-lane block border, h_query[126] is its last element
SPOILED = [("alpha_g1", 0), ("gamma_g2", 0), ("gamma_abc_g1", 1), ("delta_g1", 0), ("a_query", 30), ("b_g1_query", 5), ("b_g2_query", 63),
           ("b_g2_query", 64), ("h_query", 126), ("l_query", 69)]


def test_one_spoiled_point_in_every_section_class(gpu):
    s = setup(gpu, "chain70")
    assert len(s["key"]["h_query"]) == 127 and len(s["key"]["b_g2_query"]) == 72 and len(s["key"]["l_query"]) == 70
    order = bs.key_point_order(s["key"])
    for k, (section, index) in enumerate(SPOILED):
        key = dict(s["key"])
        badp = off_subgroup_point(section in bs.G2_FIELDS, 40 + k)               # on the curve, outside the prime-order subgroup
        if isinstance(key[section], list):
            key[section] = list(key[section])
            key[section][index] = badp
        else:
            key[section] = badp
        where = order.index((section, index))
        for form in (0, 1):
            err = _load_fails(gpu, bs.ser_key(key, form), form)
            assert err.code == gpu.KEY_ERR_POINT and err.first_bad_point == where, (section, index, form)
        gpu.ProvingKey.from_serialized(bs.ser_key(key, 1), 2, curve=CURVE).release()   # unchecked: loads
    # an x that is no field element (x = q), in l_query and - with an earlier index - in b_g2_query: rejected in every form, the first one named
    for form in (0, 1, 2):
        data = bytearray(s["bytes"][min(form, 1)])
        rc_, lay = gpu.groth16_key_layout(bytes(data), form, curve=CURVE)
        assert rc_ == 0
        P, S = int(lay[0]), gpu.KEY_LAYOUT_SLOTS
        at = int(lay[S["l_query"] + 1]) + 7 * P
        data[at:at + 48] = bs.Q.to_bytes(48, "little")
        err = _load_fails(gpu, bytes(data), form)
        assert err.code == gpu.KEY_ERR_POINT and err.first_bad_point == order.index(("l_query", 7)), form
        at = int(lay[S["b_g2_query"] + 1]) + 65 * 2 * P + 48                     # x.c1 of b_g2_query[65]
        data[at:at + 48] = bs.Q.to_bytes(48, "little")
        err = _load_fails(gpu, bytes(data), form)
        assert err.code == gpu.KEY_ERR_POINT and err.first_bad_point == order.index(("b_g2_query", 65)), form


def test_malformed_keys_fail_cleanly(gpu):
    import bw6_serial as b761
    s = setup(gpu, "toy")
    for form in (0, 1, 2):
        data = s["bytes"][min(form, 1)]
        assert _load_fails(gpu, data[:-50], form).code == gpu.KEY_ERR_TRUNCATED
        assert _load_fails(gpu, data[:200], form).code == gpu.KEY_ERR_TRUNCATED
        assert _load_fails(gpu, data + b"\x00", form).code == gpu.KEY_ERR_TRAILING
        assert _load_fails(gpu, s["bytes"][0 if form else 1], form).code != 0     # the bytes of the other point size
    empty = dict(s["key"], a_query=[])
    assert _load_fails(gpu, bs.ser_key(empty, 0), 0).code == 2                    # the proof needs a_query[0]
    # a BW6-761 key: the reference's verifying key and identity sections
    vk = b761.reference_vk()
    n_abc = int.from_bytes(vk[384:392], "little")
    k761 = {"alpha_g1": None, "beta_g2": None, "gamma_g2": None, "delta_g2": None, "gamma_abc_g1": [None] * n_abc, "beta_g1": None, "delta_g1": None,
            "a_query": [None] * 6, "b_g1_query": [None] * 6, "b_g2_query": [None] * 6, "h_query": [None] * 7, "l_query": [None] * 4}
    other = vk + b761.ser_key(k761, 0)[len(vk):]
    assert gpu.groth16_key_layout(other, 0, curve="bw6_761")[0] == 0
    h, badpt = C.c_void_p(0x1234), C.c_uint64(0)
    buf = np.frombuffer(other, dtype=np.uint8)
    rc_ = gpu.lib().groth16_load_key_bls12_377_serialized(buf.ctypes.data_as(C.c_void_p), C.c_size_t(buf.size), C.c_int(0), C.c_int(0), C.byref(h), C.byref(badpt))
    assert rc_ in (gpu.KEY_ERR_TRUNCATED, gpu.KEY_ERR_TRAILING, gpu.KEY_ERR_LENGTH, gpu.KEY_ERR_POINT) and h.value is None
    # ... and the library is as it was: the next load is a normal one
    gpu.ProvingKey.from_serialized(s["bytes"][0], 0, curve=CURVE).release()


def test_failed_loads_leak_nothing(gpu):
    s = setup(gpu, "chain62")
    key = dict(s["key"], l_query=list(s["key"]["l_query"]))
    key["l_query"][33] = off_subgroup_point(False, 77)
    where = bs.key_point_order(key).index(("l_query", 33))
    data = np.frombuffer(bs.ser_key(key, 1), dtype=np.uint8)
    lib = gpu.lib()

    def fail_once():
        h, bad = C.c_void_p(0x1234), C.c_uint64(0)
        rc_ = lib.groth16_load_key_bls12_377_serialized(data.ctypes.data_as(C.c_void_p), C.c_size_t(data.size), C.c_int(1), C.c_int(0), C.byref(h), C.byref(bad))
        assert rc_ == gpu.KEY_ERR_POINT and bad.value == where and h.value is None
    torch.cuda.synchronize()
    fail_once()
    free_1 = torch.cuda.mem_get_info()[0]
    for _ in range(10):
        fail_once()
    free_11 = torch.cuda.mem_get_info()[0]
    assert free_1 - free_11 <= 2 << 20, (free_1, free_11)


def test_handle_from_another_device(gpu):
    n = gpu.device_count()
    if n < 2:
        pytest.skip("needs >= 2 MI355X devices (this box has %d)" % n)
    s = setup(gpu, "toy")
    key = gpu.ProvingKey.from_serialized(s["bytes"][0], 0, curve=CURVE)
    z = rc.mont(s["z"], P_FR)
    try:
        gpu.use_device(1)
        k = [np.ascontiguousarray(s["consts"][c], dtype=np.uint64) for c in ("omega", "omega_inv", "coset", "coset_inv", "size_inv", "vanishing_inv")]
        out = [np.zeros(w, dtype=np.uint64) for w in (18, 36, 18)]
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        rc_ = gpu.lib().groth16_prove_r1cs_with_key(key.h, s["r"].h, p(z), C.c_uint(s["log_n"]), *[p(x) for x in k], *[p(o) for o in out])
        assert rc_ == 101
    finally:
        gpu.use_device(0)
        key.release()
