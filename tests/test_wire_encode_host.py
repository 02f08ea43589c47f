"""CPU (-m "not gpu"): the point encoders (csrc/wire.h WireEnc, csrc/wire761.h) through their host twins under bounds tracking - the kernels
run the same templates -, against oracle/py/ecc.ser_point, for all four groups and both forms:

- the edge table of tests/wire_encode_cases.py (coordinate values around 0, the limb boundaries, (q - 1) / 2 and q - 1; rows that are no
  field elements; the identity through `inf` and through a zero row; (0, 1) as a point, and as the identity under the key writer's rule);
- the reference's own VK and proof points: decoded by the oracle, encoded by the twin, the reference's 96 bytes each; the proof's points
  also from Jacobian triples with Z != 1 and Z = 0;
- the new symbols are declared, exported and wrapped, and refuse without a device;
- groth16_serialized_key_size_bw6_761 against the length of tests/bw6_serial.ser_key."""
import ctypes as C
import numpy as np
import pytest
from oracle.py import ecc
from oracle import cpu_oracle as co
import bw6_serial as bs
import wire_encode_cases as wc
from helpers import build_hosttest

ENCODERS = ["compress_bls12_377_g1", "compress_bls12_377_g2", "compress_bw6_761", "encode_uncompressed_bls12_377_g1", "encode_uncompressed_bls12_377_g2",
            "encode_uncompressed_bw6_761"]
NEW_SYMBOLS = ENCODERS + [n + "_dev" for n in ENCODERS] + ["groth16_serialized_key_size_bw6_761", "groth16_serialize_key_bw6_761", "groth16_serialize_proof_bw6_761",
                                                         "celo_amd_wire_encode_last_ms", "celo_amd_wire_encode_key_timings"]


@pytest.fixture(scope="module")
def ht():
    return C.CDLL(build_hosttest())


def encode(ht, g, rows, inf, compressed, ark_zero=False):
    rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, g.words)
    n = rows.shape[0]
    out = np.full((n, g.size[compressed]), 0xA5, dtype=np.uint8)             # every byte has to be written
    st = np.full(n, 0xA5, dtype=np.uint8)
    rc = ht.ht_wire_encode(C.c_int(g.code), C.c_int(1 if compressed else 0), rows.ctypes.data_as(C.c_void_p),
                           None if inf is None else inf.ctypes.data_as(C.c_void_p), C.c_size_t(n), C.c_int(1 if ark_zero else 0),
                           out.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return out, st


@pytest.mark.parametrize("compressed", [True, False], ids=["compressed", "uncompressed"])
@pytest.mark.parametrize("name", wc.GROUP_IDS)
def test_edge_table(ht, name, compressed):
    g = wc.GROUPS[name]
    rows, inf, points, status = wc.edge_table(g)
    want = wc.expected_bytes(g, points, status, compressed)
    got, st = encode(ht, g, rows, inf, compressed)
    assert np.array_equal(st, status), np.nonzero(st != status)[0]
    assert np.array_equal(got, want), np.nonzero((got != want).any(axis=1))[0]
    flags = got[:, -1] & 0xC0
    seen = set()
    for i, P in enumerate(points):
        if status[i] == 0 and compressed:
            seen.add(int(flags[i]))
            if wc.flag_must_be_clear(g, P):
                assert flags[i] == 0, P
        if status[i] == 0 and not compressed:
            assert flags[i] == 0                                              # no sign bit in the uncompressed form
        if status[i] == 1:
            assert flags[i] == 0x40 and not got[i, :-1].any() and got[i, -1] == 0x40
        if status[i] == 2:
            assert not got[i].any()
    if compressed:
        assert seen == {0, 0x80}
    # without an inf array the zero row is still the identity, and nothing else is
    keep = inf == 0
    got2, st2 = encode(ht, g, rows[keep], None, compressed)
    assert np.array_equal(st2, status[keep]) and np.array_equal(got2, want[keep])


@pytest.mark.parametrize("name", wc.GROUP_IDS)
def test_zero_one_is_a_point_unless_key_level(ht, name):
    g = wc.GROUPS[name]
    P = ((0, 0), (1, 0)) if g.f2 else (0, 1)
    row = g.pack([P])[0]
    for compressed in (True, False):
        got, st = encode(ht, g, row, None, compressed)
        assert st[0] == 0 and got[0].tobytes() == g.ser(P, compressed)
        got, st = encode(ht, g, row, None, compressed, ark_zero=True)
        assert st[0] == 1 and got[0].tobytes() == g.ser(None, compressed)
    # the key writer's rule touches nothing else: x = 0 with another y, another x with y = 1
    others = [(P[0], ((2, 0) if g.f2 else 2)), (((1, 0) if g.f2 else 1), P[1])] + ([(P[0], (1, 1)), ((0, 1), P[1])] if g.f2 else [])
    got, st = encode(ht, g, g.pack(others)[0], None, True, ark_zero=True)
    assert (st == 0).all() and got.tobytes() == b"".join(g.ser(Q, True) for Q in others)


def test_reference_points(ht):
    pts = bs.reference_points()
    assert len(pts) == 10
    for curve, data in pts:
        g = wc.GROUPS["g2_761" if curve is ecc.E2_761 else "g1_761"]
        P = ecc.deser_point(curve, data)
        got, st = encode(ht, g, co.pack_761([P])[0], None, True)
        assert st[0] == 0 and got[0].tobytes() == data
        got, st = encode(ht, g, co.pack_761([P])[0], None, False)
        assert st[0] == 0 and got[0].tobytes() == ecc.ser_point(curve, P, compressed=False)


def jacobian(P, z):
    """an arkworks Jacobian triple (X Z^2, Y Z^3, Z) of the affine point P as 36 u64 Montgomery limbs; P None: (1, 1, 0)"""
    q = ecc.Q761
    if P is None:
        return co.to_mont([1, 1, 0], q).reshape(36)
    return co.to_mont([P[0] * z * z % q, P[1] * z * z * z % q, z], q).reshape(36)


def test_proof_points_from_jacobian(ht):
    rng = ecc.SplitMix64(288)
    for curve, data in bs.reference_points()[-3:]:
        P = ecc.deser_point(curve, data)
        for z in (1, 2, ecc.Q761 - 1, ecc.random_scalar(rng, ecc.Q761)):
            out = np.zeros(96, dtype=np.uint8)
            assert ht.ht_wire761_encode_jacobian(jacobian(P, z).ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == 0
            assert out.tobytes() == data
    out = np.zeros(96, dtype=np.uint8)
    assert ht.ht_wire761_encode_jacobian(jacobian(None, 0).ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == 1
    assert out.tobytes() == ecc.ser_point(ecc.E1_761, None)


def test_new_symbols_declared_exported_and_wrapped():
    import os
    import re
    from celo_bls_snark_rs_amd import ffi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "celo_bls_amd.h")).read(), flags=re.S)
    lib = C.CDLL(ffi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in ffi.EXPORTS and hasattr(lib, name) and re.search(r"\bint\s+%s\s*\(" % name, hdr), name
    for fn in (ffi.encode_points, ffi.encode_points_dev, ffi.groth16_serialized_key_size, ffi.groth16_serialize_key, ffi.groth16_serialize_proof,
               ffi.wire_encode_last_ms, ffi.wire_encode_key_timings):
        assert callable(fn)
    assert lib.celo_amd_wire_encode_last_ms(None) == 2 and lib.celo_amd_wire_encode_key_timings(None) == 2
    assert ffi.wire_encode_last_ms() >= 0.0 and len(ffi.wire_encode_key_timings()) == 3
    # the proof writer is host code: NULL pointers are refused, and it needs no device
    assert lib.groth16_serialize_proof_bw6_761(None, None, None, None) == 2
    pr = bs.reference_points()[-3:]
    jac = [jacobian(ecc.deser_point(c, d), 3 + i) for i, (c, d) in enumerate(pr)]
    assert ffi.groth16_serialize_proof(*jac) == b"".join(d for _, d in pr)
    assert ffi.groth16_serialize_proof(jac[0], jacobian(None, 0), jac[2])[96:192] == ecc.ser_point(ecc.E2_761, None)


def test_argument_checks_need_no_device():
    """n == 0 returns 0 and bad arguments return 2 before the device is looked for: the same answers with and without one."""
    from celo_bls_snark_rs_amd import ffi
    lib = ffi.lib()
    buf = np.zeros(192, dtype=np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    for name in ENCODERS:
        assert getattr(lib, name)(None, None, C.c_size_t(0), None, None) == 0, name
        assert getattr(lib, name + "_dev")(None, None, C.c_size_t(0), None, None, None) == 0, name
        assert getattr(lib, name)(None, None, C.c_size_t(1), p, p) == 2 and getattr(lib, name)(p, None, C.c_size_t(1), None, p) == 2
        assert getattr(lib, name)(p, None, C.c_size_t(1), p, None) == 2 and getattr(lib, name)(p, None, C.c_size_t(1 << 31), p, p) == 2
        assert getattr(lib, name + "_dev")(C.c_void_p(8), None, C.c_size_t(1), C.c_void_p(12), C.c_void_p(8), None) == 2, name     # output not 8-byte aligned


def test_device_entry_points_refuse_without_a_device():
    """No quiet host fall-back: without a HIP device every bulk encoder and the key writer return an error."""
    import torch
    from celo_bls_snark_rs_amd import ffi
    if torch.cuda.is_available():
        pytest.skip("GPU present: tests/test_wire_encode_gpu.py runs these entry points")
    for name, g in wc.GROUPS.items():
        row = g.pack([g.gen()])[0]
        for compressed in (True, False):
            with pytest.raises(ffi.WireEncodeError):
                ffi.encode_points(g.ffi_group, row, None, compressed)
            with pytest.raises(ffi.WireEncodeError):                          # (refused before any pointer is looked at)
                ffi.encode_points_dev(g.ffi_group, 8, 0, 1, 8, 8, compressed)
    vk = co.pack_761([wc.GROUPS["g1_761"].gen()] * 5)[0]
    with pytest.raises(ffi.KeySerializeError) as e:
        ffi.groth16_serialize_key(vk)
    assert e.value.code not in (0, 2, 33, 35)


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("counts", [(1, 1, 0), (1, 2, 1), (3, 7, 8)])
def test_serialized_key_size(ht, counts, form):
    from celo_bls_snark_rs_amd import ffi
    n_inputs, n_vars, n_h = counts
    key = {"alpha_g1": None, "beta_g2": None, "gamma_g2": None, "delta_g2": None, "gamma_abc_g1": [None] * n_inputs, "beta_g1": None, "delta_g1": None,
           "a_query": [None] * n_vars, "b_g1_query": [None] * n_vars, "b_g2_query": [None] * n_vars, "h_query": [None] * n_h, "l_query": [None] * (n_vars - n_inputs)}
    full = len(bs.ser_key(key, form))
    vk = len(bs.ser(bs.E1, None, form)) + 3 * len(bs.ser(bs.E2, None, form)) + len(bs.ser_vec(bs.E1, key["gamma_abc_g1"], form))
    assert ffi.groth16_serialized_key_size(n_inputs, n_vars, n_h, form) == full
    assert ffi.groth16_serialized_key_size(n_inputs, n_vars, n_h, form, vk_only=True) == vk
    ln = C.c_uint64(0)
    assert ht.ht_wire761_key_size(C.c_size_t(n_inputs), C.c_size_t(n_vars), C.c_size_t(n_h), C.c_int(form), C.c_int(0), C.byref(ln)) == 0 and ln.value == full
    # what the layout walk of the loader accepts has exactly this length
    rc, out = ffi.groth16_key_layout(bs.ser_key(key, form), form)
    assert rc == 0 and int(out[1]) == full and int(out[15]) == 4 + n_inputs + 2 + 3 * n_vars + n_h + (n_vars - n_inputs)


def test_serialized_key_size_rejections():
    from celo_bls_snark_rs_amd import ffi
    for args in ((0, 1, 0, 0), (2, 1, 0, 0), (1, 1, 0, 2), (1, 1, 0, -1), (1, 1 << 63, 0, 1)):
        with pytest.raises(ffi.KeySerializeError) as e:
            ffi.groth16_serialized_key_size(*args)
        assert e.value.code == 2
    assert ffi.lib().groth16_serialized_key_size_bw6_761(C.c_size_t(1), C.c_size_t(1), C.c_size_t(0), C.c_int(0), C.c_int(0), None) == 2
    # the cap check comes before any device call: one byte short reports the size needed
    vk = co.pack_761([wc.GROUPS["g1_761"].gen()] * 5)[0]
    need = ffi.groth16_serialized_key_size(1, 0, 0, 0, vk_only=True)
    with pytest.raises(ffi.KeySerializeError) as e:
        ffi.groth16_serialize_key(vk, cap=need - 1)
    assert e.value.code == ffi.KEY_ERR_CAPACITY and e.value.out_len == need
