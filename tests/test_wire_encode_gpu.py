"""GPU: the bulk point encoders (compress_* / encode_uncompressed_*, csrc/unit_wire_encode.hip) and the key, VK and proof writers on top of them.

- Every group and form at n = 1, 63, 64, 65, 130 (one lane; a partial, an exact, a ragged second and a ragged third block of the 64-lane
  launch), host-pointer and _dev forms: whole outputs and whole status arrays against oracle/py/ecc.ser_point, with
  identities at lanes 0, 63, 64 and n - 1 and the edge table of tests/wire_encode_cases.py appended to the largest size.
- Round trips through the decoders.
- The reference's VK bytes from its decoded points; the reference's proof bytes from Jacobian triples of its points.
- groth16_setup_bw6_761's rows -> groth16_serialize_key_bw6_761 == tests/bw6_serial.ser_key; the bytes load and prove like the setup's own key;
  the error codes."""
import ctypes as C
import numpy as np
import pytest
import torch  # before the library: both must share one HIP runtime
from oracle.py import ecc
from oracle import cpu_oracle as co
import bw6_serial as bs
import groth16_setup_ref as gs
import wire_encode_cases as wc
from test_groth16_setup_gpu import setup_inputs, run_setup, prove

pytestmark = pytest.mark.gpu
SIZES = [1, 63, 64, 65, 130]
_CASES = {}


def cases(name):
    """per group, computed once: 65 pairs k G, -(k G) (both values of the sign flag) as rows, and the edge table"""
    if name not in _CASES:
        g = wc.GROUPS[name]
        pts, P = [], None
        for _ in range(65):
            P = g.curve.add(P, g.gen())
            pts += [P, g.curve.neg(P)]
        _CASES[name] = {"points": pts, "rows": g.pack(pts)[0], "edge": wc.edge_table(g)}
    return _CASES[name]


def batch(name, n, identities=True):
    """(rows, inf, points, status) of n lanes: the pairs, identities at lanes 0, 63, 64 and n - 1 (through a zero row and through inf in
    turn; the inf lanes keep their row), and for the largest size the edge table behind them"""
    g, c = wc.GROUPS[name], cases(name)
    rows, points = c["rows"][:n].copy(), list(c["points"][:n])
    inf, status = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    for k, lane in enumerate(sorted({0, 63, 64, n - 1} & set(range(n))) if identities else []):
        if k & 1:
            inf[lane] = 1
        else:
            rows[lane] = 0
        points[lane], status[lane] = None, 1
    if n == SIZES[-1]:
        er, ei, ep, es = c["edge"]
        rows, inf, points, status = np.concatenate([rows, er]), np.concatenate([inf, ei]), points + ep, np.concatenate([status, es])
    return rows, inf, points, status


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else a.dtype)).cuda()


def encode_dev(gpu, g, rows, inf, compressed):
    n = rows.shape[0]
    d_rows, d_inf = dev(rows), (None if inf is None else dev(inf))
    d_out = torch.full((n * g.size[compressed],), 0xA5, dtype=torch.uint8, device="cuda")       # every byte has to be written
    d_st = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    gpu.encode_points_dev(g.ffi_group, d_rows.data_ptr(), 0 if d_inf is None else d_inf.data_ptr(), n, d_out.data_ptr(), d_st.data_ptr(), compressed)
    return d_out.cpu().numpy().reshape(n, -1), d_st.cpu().numpy()


@pytest.mark.parametrize("compressed", [True, False], ids=["compressed", "uncompressed"])
@pytest.mark.parametrize("name", wc.GROUP_IDS)
def test_whole_outputs_at_every_block_shape(gpu, name, compressed):
    g = wc.GROUPS[name]
    flags = set()
    for n, identities in [(n, True) for n in SIZES] + [(1, False)]:           # (n = 1 with lane 0 the identity, and with a point there)
        rows, inf, points, status = batch(name, n, identities)
        want = wc.expected_bytes(g, points, status, compressed)
        for form in ("host", "dev"):
            got, st = gpu.encode_points(g.ffi_group, rows, inf, compressed) if form == "host" else encode_dev(gpu, g, rows, inf, compressed)
            assert np.array_equal(st, status), (n, form, np.nonzero(st != status)[0])
            assert np.array_equal(got, want), (n, form, np.nonzero((got != want).any(axis=1))[0])
        flags |= {int(b) for b in want[status == 0][:, -1] & 0x80}
        assert gpu.wire_encode_last_ms() > 0
    if compressed:
        assert flags == {0, 0x80}                                              # both values of the sign flag occurred
    # no inf array: the zero rows are still identities
    rows, inf, points, status = batch(name, 65)
    rows[inf != 0] = 0
    want = wc.expected_bytes(g, points, status, compressed)
    for got, st in (gpu.encode_points(g.ffi_group, rows, None, compressed), encode_dev(gpu, g, rows, None, compressed)):
        assert np.array_equal(st, status) and np.array_equal(got, want)


def decode(gpu, name, data, compressed):
    g = wc.GROUPS[name]
    if g.code == 2:
        group = "bw6_761_g2" if name == "g2_761" else "bw6_761_g1"
        return gpu.decompress(group, data) if compressed else gpu.decode_uncompressed(group, data)
    return gpu.decompress(g.ffi_group, data)


@pytest.mark.parametrize("name", wc.GROUP_IDS)
def test_round_trips_through_the_decoders(gpu, name):
    g = wc.GROUPS[name]
    rows, inf, points, status = batch(name, 65)
    rows[inf != 0] = 0                                                         # what a decoder returns for the identity
    for compressed in ((True, False) if g.code == 2 else (True,)):             # BLS12-377 has compressed decoders only
        enc, st = gpu.encode_points(g.ffi_group, rows, inf, compressed)
        assert np.array_equal(st, status)
        back, dst = decode(gpu, name, enc.tobytes(), compressed)
        assert np.array_equal(dst, status) and np.array_equal(back, rows)      # status 0 or 1, the same in both directions
    if g.code == 2:
        ref = [d for c, d in bs.reference_points() if c is g.curve]
        xy, dst = decode(gpu, name, b"".join(ref), True)
        assert (dst == 0).all()
        enc, st = gpu.encode_points(g.ffi_group, xy, None, True)
        assert (st == 0).all() and enc.tobytes() == b"".join(ref)
    else:
        ref = b"".join(g.ser(P, True) for P in points)
        xy, dst = decode(gpu, name, ref, True)
        enc, st = gpu.encode_points(g.ffi_group, xy, dst, True)                # a decoder's status 1 is an `inf` byte
        assert np.array_equal(st, status) and enc.tobytes() == ref


def test_argument_checks(gpu):
    lib = gpu.lib()
    g = wc.GROUPS["g1_761"]
    rows, inf, points, status = batch("g1_761", 64)
    d_rows, d_out, d_st = dev(rows), torch.zeros(64 * 192 + 8, dtype=torch.uint8, device="cuda"), torch.zeros(64, dtype=torch.uint8, device="cuda")
    for compressed in (True, False):
        with pytest.raises(gpu.WireEncodeError) as e:                          # a _dev output pointer that is not 8-byte aligned
            gpu.encode_points_dev("bw6_761", d_rows.data_ptr(), 0, 64, d_out.data_ptr() + 4, d_st.data_ptr(), compressed)
        assert e.value.code == 2
    assert not d_out.any() and not d_st.any()
    out, st = np.zeros(96, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.compress_bw6_761(None, None, C.c_size_t(1), p(out), p(st)) == 2
    assert lib.compress_bw6_761(p(rows), None, C.c_size_t(1), None, p(st)) == 2
    assert lib.compress_bw6_761(p(rows), None, C.c_size_t(1), p(out), None) == 2
    assert lib.compress_bw6_761(p(rows), None, C.c_size_t(1 << 31), p(out), p(st)) == 2
    assert lib.compress_bw6_761(None, None, C.c_size_t(0), None, None) == 0    # n == 0


def test_reference_vk_bytes(gpu):
    vk = bs.reference_vk()
    pts = bs.reference_points()[:-3]
    g1 = [d for c, d in pts if c is ecc.E1_761]
    g2 = [d for c, d in pts if c is ecc.E2_761]
    x1, s1 = gpu.decompress("bw6_761_g1", b"".join(g1))
    x2, s2 = gpu.decompress("bw6_761_g2", b"".join(g2))
    assert (s1 == 0).all() and (s2 == 0).all() and len(g2) == 3
    out_vk = np.concatenate([x1[:1], x2, x1[1:]])                              # alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1
    assert gpu.groth16_serialize_key(out_vk) == vk
    assert gpu.groth16_serialized_key_size(len(g1) - 1, 0, 0, 0, vk_only=True) == len(vk)
    unc = gpu.groth16_serialize_key(out_vk, form=1)
    assert unc == b"".join(ecc.ser_point(c, ecc.deser_point(c, d), compressed=False) for c, d in pts[:4]) + (len(g1) - 1).to_bytes(8, "little") + \
        b"".join(ecc.ser_point(c, ecc.deser_point(c, d), compressed=False) for c, d in pts[4:])


def test_reference_proof_bytes(gpu, golden):
    proof = bytes.fromhex(golden["groth16_bw6_761"]["proof"])
    assert len(proof) == 288
    q, rng = ecc.Q761, ecc.SplitMix64(2880)
    jac = []
    for curve, data in bs.reference_points()[-3:]:
        P = ecc.deser_point(curve, data)
        z = ecc.random_scalar(rng, q - 2) + 2                                  # Z != 0, 1
        jac.append(co.to_mont([P[0] * z * z % q, P[1] * z * z * z % q, z], q).reshape(36))
    assert gpu.groth16_serialize_proof(*jac) == proof
    at_infinity = co.to_mont([5, 7, 0], q).reshape(36)                         # Z == 0
    got = gpu.groth16_serialize_proof(jac[0], jac[1], at_infinity)
    assert got[:192] == proof[:192] and got[192:] == ecc.ser_point(ecc.E1_761, None)


def key_dict(out):
    """groth16_setup's rows as the python points tests/bw6_serial.ser_key takes (rows (0, 1) -> None)"""
    pts = {name: gs.to_points("bw6_761", 2 if name in bs.G2_FIELDS else 1, rows) for part in ("vk", "rows") for name, rows in out[part].items()}
    return {name: (pts[name] if name in ("gamma_abc_g1", "a_query", "b_g1_query", "b_g2_query", "h_query", "l_query") else pts[name][0]) for name in bs.SECTIONS}


@pytest.mark.parametrize("size", ["toy", "chain_2"])
def test_setup_key_serializes_loads_and_proves(gpu, size):
    curve, p = "bw6_761", gs.FIELDS["bw6_761"]
    circ, z = (gs.toy_circuit(), gs.toy_witness(3, p)) if size == "toy" else (gs.squaring_chain(2), gs.squaring_witness(2, 7, p))
    s = setup_inputs(curve, circ, 17)
    out = run_setup(gpu, curve, s, want_key=True)
    key = out["key"]
    try:
        kd = key_dict(out)
        assert any(P is None for name in ("a_query", "b_g1_query", "b_g2_query", "h_query", "l_query") for P in kd[name])      # identity rows are there
        n_vars, n_h, n_in = s["n_vars"], s["n_h"], s["n_in"]
        ser = {form: gpu.groth16_serialize_key(out["vk"], out["rows"], n_vars, n_h, form) for form in (0, 1)}
        for form in (0, 1):
            assert ser[form] == bs.ser_key(kd, form), form
            assert len(ser[form]) == gpu.groth16_serialized_key_size(n_in, n_vars, n_h, form)
        t = gpu.wire_encode_key_timings()
        assert t[1] > 0
        assert gpu.groth16_serialize_key(out["vk"]) == ser[0][:4 * 96 + 8 + 96 * n_in]                       # the VerifyingKey is the key's prefix
        loaded = gpu.ProvingKey.from_serialized(ser[0], 0)
        try:
            assert prove(gpu, loaded, curve, circ, z, s["log_n"]) == prove(gpu, key, curve, circ, z, s["log_n"])
        finally:
            loaded.release()
        # cap one byte short: the size code and the size needed
        with pytest.raises(gpu.KeySerializeError) as e:
            gpu.groth16_serialize_key(out["vk"], out["rows"], n_vars, n_h, 0, cap=len(ser[0]) - 1)
        assert e.value.code == gpu.KEY_ERR_CAPACITY and e.value.out_len == len(ser[0])
        # a row of h_query whose limbs are q: no field element; reported by its index in serialization order, the loader's index space
        j = n_h - 1
        rows = {k: np.array(v, copy=True) for k, v in out["rows"].items()}
        rows["h_query"][j, 12:] = co.ints_to_limbs([ecc.Q761], 12)[0]
        for form in (0, 1):
            with pytest.raises(gpu.KeySerializeError) as e:
                gpu.groth16_serialize_key(out["vk"], rows, n_vars, n_h, form)
            assert e.value.code == gpu.KEY_ERR_POINT and e.value.first_bad_point == bs.key_point_order(kd).index(("h_query", j))
        flat = np.concatenate([np.asarray(rows[k], dtype=np.uint64).reshape(-1) for k in ("beta_g1", "delta_g1", "a_query", "b_g1_query", "b_g2_query", "h_query", "l_query")])
        vkf = np.concatenate([np.asarray(out["vk"][k], dtype=np.uint64).reshape(-1) for k in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "gamma_abc_g1")])
        buf, ln, bad = np.full(len(ser[0]), 0xA5, dtype=np.uint8), C.c_uint64(0), C.c_uint64(0)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert gpu.lib().groth16_serialize_key_bw6_761(p(vkf), C.c_size_t(n_in), p(flat), C.c_size_t(n_vars), C.c_size_t(n_h), C.c_int(0), p(buf), C.c_size_t(buf.size),
                                                       C.byref(ln), C.byref(bad)) == gpu.KEY_ERR_POINT
        assert (buf == 0xA5).all() and ln.value == len(ser[0])                                               # with 33 nothing is written to out
        # bad counts
        for args in ((out["vk"], out["rows"], n_vars, n_h, 2),):
            with pytest.raises(gpu.KeySerializeError) as e:
                gpu.groth16_serialize_key(*args)
            assert e.value.code == 2
    finally:
        key.release()


def test_failed_key_writes_leak_nothing(gpu):
    """33 (a bad row) on every call: the device memory in use does not grow"""
    n_in, n_vars, n_h = 2, 300, 511
    g = wc.GROUPS["g1_761"]
    row = g.pack([g.gen()])[0][0]
    vk = np.tile(row, (4 + n_in, 1))
    rows = np.tile(row, (2 + 3 * n_vars + n_h + n_vars - n_in, 1))
    rows[700, :12] = co.ints_to_limbs([ecc.Q761], 12)[0]

    def fail_once():
        with pytest.raises(gpu.KeySerializeError) as e:
            gpu.groth16_serialize_key(vk, rows, n_vars, n_h, 0)
        assert e.value.code == gpu.KEY_ERR_POINT and e.value.first_bad_point == 4 + n_in + 700
    torch.cuda.synchronize()
    fail_once()
    free_1 = torch.cuda.mem_get_info()[0]
    for _ in range(10):
        fail_once()
    assert free_1 - torch.cuda.mem_get_info()[0] <= 2 << 20
