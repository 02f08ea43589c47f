"""CPU (-m "not gpu"): the constructed BLS12-377 Groth16 proofs of tests/groth16_verify377_cases.py against the oracle, the combined equation,
the BLS12-377 host twins of the verifier's lane routines under bounds tracking, the serialized key parse and its refusals, the window rule and
the lane kernels' resources.

Mutation pairs of the verifier (tests/test_groth16_verify377_gpu.py runs them on the device): all r_i = 1 -> the cancelling pair; dropping the
input range test -> the r / r + 1 inputs; an off-by-one in the window count -> the all-ones inputs; the 8 / 9-pair border of the combined
product -> m = 5 / 6."""
import ctypes as C
import os
import re
import numpy as np
import pytest
from oracle.py import ecc
from oracle import cpu_oracle as co
from tests import groth16_verify377_cases as gc
from tests import helpers as H

R = gc.R
KEY8 = np.arange(8, dtype=np.uint32)
WANT = {"valid": 1, "rerandomised": 1, "inf_a_accept": 1, "edge_0": 1, "edge_1": 1, "edge_rm1": 1, "edge_ones": 1}


@pytest.fixture(scope="module")
def key2():
    return gc.Key(2, 0x6116)


@pytest.fixture(scope="module")
def ht():
    return C.CDLL(H.build_hosttest())


@pytest.mark.parametrize("n_in", [0, 2])
def test_builder_verdicts_equal_the_oracles(n_in):
    """every case class once (and, with inputs, the cancelling and the swapped pair): the verdict its formula says, the verdict the scalars
    give and the oracle's product of the four pairs are one value"""
    key = gc.Key(n_in, 0x6116 + n_in)
    rng = ecc.SplitMix64(11)
    proofs = [gc.special_proof(key, rng, k) for k in gc.classes_for(key)] + list(gc.cancelling_pair(key, rng))
    if n_in:
        proofs += list(gc.swapped_pair(key, rng))
    else:
        assert {p.kind for p in proofs}.isdisjoint(gc.INPUT_CLASSES)
    b = gc.Batch(key, proofs)
    for i, p in enumerate(proofs):
        assert b.expect[i] == WANT.get(p.kind, 0), p.kind
        assert gc.oracle_verdict(b, i) == b.expect[i], p.kind


def test_combined_equation_on_the_oracle(key2):
    """a valid batch of 5 satisfies the combined equation under the drawn exponents; (C_1 + D, C_2 - D) satisfies it with r = (1, 1) - the
    reason the combination is random - and not with drawn exponents"""
    ok = gc.batch_with(key2, 5, {}, 14)
    assert ok.expect.tolist() == [1] * 5 and gc.oracle_combined(ok, gc.exponents_ref(KEY8, 5)) == 1
    b = gc.Batch(key2, list(gc.cancelling_pair(key2, ecc.SplitMix64(13))))
    assert b.expect.tolist() == [0, 0]
    assert gc.oracle_combined(b, [1, 1]) == 1
    assert gc.oracle_combined(b, gc.exponents_ref(KEY8, 2)) == 0


@pytest.mark.parametrize("n_in", [0, 1, 2, 3, 8])
def test_host_twin_input_row(ht, n_in):
    """ht_g16_input_row_377 (the body of k_g16_inputs<G16Bls>, bounds tracked) against the oracle's MSM: the edge inputs, random ones, r and r + 1"""
    key = gc.Key(n_in, 100 + n_in)
    rng = ecc.SplitMix64(200 + n_in)
    xs = [[v] * n_in for v in gc.EDGE_INPUTS] + [[ecc.random_scalar(rng, R) for _ in range(n_in)] for _ in range(2)]
    if n_in:
        xs += [[R] + [1] * (n_in - 1), [2] * (n_in - 1) + [R + 1], [(1 << 256) - 1] * n_in]
    n = len(xs)
    inputs = co.ints_to_limbs([v for x in xs for v in x], 4).reshape(n, n_in, 4) if n_in else np.zeros((n, 0, 4), dtype=np.uint64)
    for c in ({0: (4,), 8: (9,)}.get(n_in, (4, 5, 10))):
        out = np.zeros((n, 12), dtype=np.uint64)
        inf = np.zeros(n, dtype=np.uint8)
        st = np.zeros(n, dtype=np.uint8)
        abc = np.ascontiguousarray(key.abc)
        ht.ht_g16_input_row_377(co._p(abc), C.c_size_t(n_in + 1), co._p(inputs), C.c_size_t(n), C.c_int(c), co._p(out), co._p(inf), co._p(st))
        assert st.tolist() == [0 if all(v < R for v in x) else 1 for x in xs]
        good = [i for i in range(n) if not st[i]]
        want, winf = gc.acc_rows(key, inputs[good])
        assert np.array_equal(out[good], want) and np.array_equal(inf[good], winf), (n_in, c)


def test_host_twin_scale(ht):
    """ht_g16_scale_377 (the body of k_g16_scale<G16Bls>) against orc_mul_bls12_377_g1: 2^127, 2^128 - 1, random exponents; a point of small x
    (on the curve, outside the subgroup)"""
    G1, _ = gc.generators()
    rng = ecc.SplitMix64(31)
    small = next(P for P in ((x, ecc.sqrt_fp((x ** 3 + 1) % ecc.Q377, ecc.Q377)) for x in range(2, 200)) if P[1] is not None)
    pts = np.concatenate([gc.mul_rows(G1, [1 + ecc.random_scalar(rng, R - 1) for _ in range(4)])[0], co.pack_g1_377([small])[0]])
    exps = [1 << 127, (1 << 128) - 1, (1 << 127) | ecc.random_scalar(rng, 1 << 127), (1 << 127) | ecc.random_scalar(rng, 1 << 127), (1 << 127) | 5]
    r2 = co.ints_to_limbs([e & ((1 << 127) - 1) for e in exps], 2)            # the top bit is the routine's own
    n = len(exps)
    out = np.zeros((n, 12), dtype=np.uint64)
    inf = np.zeros(n, dtype=np.uint8)
    ht.ht_g16_scale_377(co._p(np.ascontiguousarray(pts)), co._p(r2), C.c_size_t(n), co._p(out), co._p(inf))
    for i in range(n):
        want = ecc.E1_377.mul(gc.row_point(pts[i]), exps[i])
        assert gc.row_point(out[i], inf[i]) == want and inf[i] == 0, i
        if i < 4:                                                             # (the C++ oracle's multiple takes a scalar below r)
            jac = np.zeros(18, dtype=np.uint64)
            assert co.lib().orc_mul_bls12_377_g1(co._p(np.ascontiguousarray(pts[i])), co._p(co.ints_to_limbs([exps[i]], 4)[0]), co._p(jac)) == 0
            assert co.jac_to_affine(jac, "g1_377") == want


# ---- the serialized-key parser
def parse(ht, data, cap=70):
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    rows = np.zeros((cap, 24), dtype=np.uint64)
    inf = np.zeros(cap, dtype=np.uint8)
    n, bad = C.c_uint64(0), C.c_uint64(1 << 40)
    rc = ht.ht_g16_vk_parse_377(co._p(buf), C.c_size_t(buf.size), C.c_size_t(cap), co._p(rows), co._p(inf), C.byref(n), C.byref(bad))
    return rc, rows[:4 + n.value], inf[:4 + n.value], bad.value


def key_rows(key, abc):
    """what the parser returns for a key: every row in a slot of 24 u64, a G1 row in its first half"""
    rows = np.zeros((4 + len(abc), 24), dtype=np.uint64)
    rows[0, :12] = key.alpha
    rows[1], rows[2], rows[3] = key.beta, key.gamma, key.delta
    rows[4:, :12] = abc
    return rows


@pytest.fixture(scope="module")
def abc65():
    """65 rows of gamma_abc (64 inputs) - and one more for the refusal"""
    G1, _ = gc.generators()
    return gc.mul_rows(G1, [3 + 7 * j for j in range(66)])[0]


def test_parse_key_without_inputs(ht):
    key0 = gc.Key(0, 5)
    data = key0.serialize()
    assert len(data) == 48 + 3 * 96 + 8 + 48
    rc, rows, inf, _ = parse(ht, data)
    assert rc == 0 and not inf.any() and np.array_equal(rows, key_rows(key0, key0.abc))


def test_parse_key_with_64_inputs(ht, key2, abc65):
    rc, rows, inf, _ = parse(ht, key2.serialize(abc65[:65]))
    assert rc == 0 and not inf.any() and np.array_equal(rows, key_rows(key2, abc65[:65]))


def test_parse_refuses_65_inputs(ht, key2, abc65):
    assert parse(ht, key2.serialize(abc65))[0] == 36


def test_parse_refuses_a_key_one_byte_short(ht, key2):
    assert parse(ht, key2.serialize()[:-1])[0] == 30


def test_parse_refuses_a_key_one_byte_long(ht, key2):
    assert parse(ht, key2.serialize() + b"\0")[0] == 31


def test_parse_names_the_point_off_the_subgroup(ht, abc65):
    """gamma_abc[3] on the curve and outside the subgroup: 33, first_bad = 4 + 3 in serialization order"""
    key = gc.Key(4, 9)
    off = gc.off_subgroup_point(False, 5)
    data = bytearray(key.serialize())
    at = 48 + 3 * 96 + 8 + 3 * 48
    data[at:at + 48] = ecc.ser_point(ecc.E1_377, off)
    rc, _, _, bad = parse(ht, data)
    assert rc == 33 and bad == 7
    data = bytearray(key.serialize())
    data[48:48 + 96] = ecc.ser_point(ecc.E2_377, gc.off_subgroup_point(True, 6))      # beta_g2
    rc, _, _, bad = parse(ht, data)
    assert rc == 33 and bad == 1


def test_window_rule(ht):
    """g16_window_bits<G16Bls> equals the rule restated from fb_windows and the entry size: the widest of 10 .. 4 bits whose tables fit
    64 MiB.  An entry is 128 B (two coordinates of 16 stored words), which puts the 10 / 9-bit border at 39 / 40 inputs"""
    for n in (0, 1, 39, 40, 45, 46, 64):
        c = ht.ht_g16_window_bits_377(C.c_size_t(n))
        assert c == gc.window_bits(n), n
        assert n * gc.fb_windows(253, c) * (1 << (c - 1)) * gc.ENTRY_BYTES <= gc.TABLE_BUDGET
        assert c == 10 or n * gc.fb_windows(253, c + 1) * (1 << c) * gc.ENTRY_BYTES > gc.TABLE_BUDGET
    assert [gc.window_bits(n) for n in (1, 39, 40, 64)] == [10, 10, 9, 9]


def test_argument_refusals_need_no_device():
    from celo_bls_snark_rs_amd import ffi
    lib = ffi.lib()
    z = np.zeros(24, dtype=np.uint64)
    abc = np.zeros((66, 12), dtype=np.uint64)
    h = C.c_void_p()
    p = co._p
    assert lib.groth16_vk_load_bls12_377(None, p(z), p(z), p(z), p(abc), C.c_size_t(1), C.byref(h)) == 2
    assert lib.groth16_vk_load_bls12_377(p(z), p(z), p(z), p(z), p(abc), C.c_size_t(1), None) == 2
    assert lib.groth16_vk_load_bls12_377(p(z), p(z), p(z), p(z), p(abc), C.c_size_t(0), C.byref(h)) == 2
    assert lib.groth16_vk_load_bls12_377(p(z), p(z), p(z), p(z), p(abc), C.c_size_t(66), C.byref(h)) == ffi.VK_ERR_INPUTS == 36
    short = np.zeros(343, dtype=np.uint8)
    assert lib.groth16_vk_load_bls12_377_serialized(p(short), C.c_size_t(343), C.byref(h)) == 30
    assert lib.groth16_vk_load_bls12_377_serialized(None, C.c_size_t(500), C.byref(h)) == 2
    hdr = np.zeros(344 + 48, dtype=np.uint8)
    hdr[336] = 66
    assert lib.groth16_vk_load_bls12_377_serialized(p(hdr), C.c_size_t(hdr.size), C.byref(h)) == 36
    assert not h.value
    out = np.zeros(1, dtype=np.uint8)
    assert lib.groth16_verify_batch_bls12_377(None, p(z), None, p(z), None, p(z), None, None, C.c_size_t(0), C.c_int(0), None, p(out)) == 0      # m = 0
    assert lib.groth16_verify_batch_bls12_377(None, p(z), None, p(z), None, p(z), None, None, C.c_size_t(1), C.c_int(0), None, p(out)) == 2
    assert lib.groth16_verify_batch_bls12_377(C.c_void_p(0x1000), p(z), None, p(z), None, p(z), None, None, C.c_size_t(1), C.c_int(0), None, p(out)) == 2
    assert lib.groth16_verify_batch_bls12_377_serialized(C.c_void_p(0x1000), None, None, C.c_size_t(1), C.c_int(0), None, p(out)) == 2
    assert lib.groth16_serialize_proof_bls12_377(None, p(z), p(z), p(out)) == 2


def test_proof_writer_matches_the_oracle():
    """groth16_serialize_proof_bls12_377 (host only) on Jacobian points with Z != 1, and on the identity: the oracle's ser_point of A | B | C"""
    from celo_bls_snark_rs_amd import ffi
    rng = ecc.SplitMix64(77)
    P = [ecc.E1_377.mul(ecc.G1_377, 1 + ecc.random_scalar(rng, R - 1)), ecc.E2_377.mul(ecc.G2_377, 1 + ecc.random_scalar(rng, R - 1)),
         ecc.E1_377.mul(ecc.G1_377, 1 + ecc.random_scalar(rng, R - 1))]
    q = ecc.Q377
    z1, z3 = 2 + ecc.random_scalar(rng, q - 2), 2 + ecc.random_scalar(rng, q - 2)
    zb = (3 + ecc.random_scalar(rng, q - 3), 1 + ecc.random_scalar(rng, q - 1))
    F2 = ecc.F2_377
    zb2 = F2.sqr(zb)
    a = co.to_mont([P[0][0] * z1 * z1 % q, P[0][1] * z1 ** 3 % q, z1], q).reshape(-1)
    c = co.to_mont([P[2][0] * z3 * z3 % q, P[2][1] * z3 ** 3 % q, z3], q).reshape(-1)
    bx, by = F2.mul(P[1][0], zb2), F2.mul(P[1][1], F2.mul(zb2, zb))
    b = co.to_mont([bx[0], bx[1], by[0], by[1], zb[0], zb[1]], q).reshape(-1)
    got = ffi.groth16_serialize_proof(a, b, c, curve="bls12_377")
    assert got == ecc.ser_point(ecc.E1_377, P[0]) + ecc.ser_point(ecc.E2_377, P[1]) + ecc.ser_point(ecc.E1_377, P[2]) and len(got) == 192
    a0 = a.copy(); a0[12:] = 0                                                # Z = 0: the identity
    got = ffi.groth16_serialize_proof(a0, b, c, curve="bls12_377")
    assert got[:48] == ecc.ser_point(ecc.E1_377, None) and got[48:] == ecc.ser_point(ecc.E2_377, P[1]) + ecc.ser_point(ecc.E1_377, P[2])


def test_resources_of_the_lane_kernels():
    """from the build's own resource remarks: the two BLS12-377 lane kernels run without scratch, at two waves per SIMD"""
    txt = open(os.path.join(gc.ROOT, "celo-bls-snark-rs_amd", "build", "unit_groth16_verify377.remarks.txt")).read()
    for kernel in ("k_g16_inputs", "k_g16_scale"):
        m = re.search(r"Function Name: \S*%s\S*G16Bls\S*.*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)" % kernel, txt, re.S)
        assert m, kernel
        assert int(m.group(1)) == 0 and int(m.group(2)) == 2, (kernel, m.groups())
