"""GPU (-m gpu): groth16_verify_batch_bw6_761 - m Groth16 proofs under one verifying key, per proof ("each") and combined - on proofs whose
verdict is known by construction (tests/groth16_verify_cases.py), with samples against the oracle's own product of the four pairs.

Mutation pairs: all r_i = 1 -> test_combined_cancelling_pair; dropping the input range test -> the input_r / input_r1 classes of
test_every_class_at_every_position; an off-by-one in the window count -> its edge_ones class and test_input_counts; the k = 7 / 8 border of
the pairing engine -> m = 4 / 5 of test_dispatch_borders in combined mode."""
import os
import re
import threading
import numpy as np
import pytest
from oracle.py import ecc
from oracle.py import epoch as ep
from oracle import cpu_oracle as co
from tests import bw6_serial as bs
from tests import groth16_verify_cases as gc
from tests import helpers as H

pytestmark = pytest.mark.gpu
R = gc.R
KEY8 = np.array([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0, 0x082EFA98, 0xEC4E6C89], dtype=np.uint32)
BUILD = os.path.join(gc.ROOT, "celo-bls-snark-rs_amd", "build")


def load(gpu, key):
    return gpu.VerifyingKey(key.alpha, key.beta, key.gamma, key.delta, key.abc)


def run(vk, b, mode, key=KEY8):
    return vk.verify(b.a, b.b, b.c, b.inputs, mode=mode, key=key, a_inf=b.a_inf, b_inf=b.b_inf, c_inf=b.c_inf)


def device_mul(gpu):
    """the multiples of a batch from the library's fixed-base rows (the large batches; a sample is compared with the oracle's)"""
    def mul(gen, scalars, on_g2):
        xy, inf = gpu.fixed_base_mul("bw6_761_g2" if on_g2 else "bw6_761_g1", gen, co.ints_to_limbs([int(k) % R for k in scalars], 6))
        xy[inf != 0] = 0
        return xy, inf
    return mul


@pytest.fixture(scope="module")
def key2():
    return gc.Key(2, 0x6116)


@pytest.fixture(scope="module")
def vk2(gpu, key2):
    vk = load(gpu, key2)
    yield vk
    vk.release()


@pytest.fixture(scope="module")
def pool(key2):
    """257 valid proofs, and the same proofs with position-dependent damage: every seventh one with a wrong input (oracle multiples)"""
    good = gc.batch_with(key2, 257, {}, 21)
    rng = ecc.SplitMix64(22)
    proofs = []
    for i, p in enumerate(good.proofs):
        q = gc.Proof(p.s, p.t, p.c, p.x, p.kind)
        if i % 7 == 3:
            q.x[0] = (q.x[0] + 1 + ecc.random_scalar(rng, R - 1)) % R
            q.kind = "wrong_input"
        proofs.append(q)
    bad = gc.take(good, range(257))
    bad.proofs = proofs
    bad.inputs = co.ints_to_limbs([v for p in proofs for v in p.x], 6).reshape(257, 2, 6)
    bad.expect = np.array([p.expect(key2) for p in proofs], dtype=np.uint8)
    assert good.expect.all() and bad.expect.sum() == 257 - len(range(3, 257, 7))
    for i in range(8):                                   # the sample against the oracle's product (positions 0 .. 7 hold a damaged proof)
        assert gc.oracle_verdict(good, i) == 1 and gc.oracle_verdict(bad, i) == bad.expect[i]
    return good, bad


def reference_batch(golden):
    """the reference's own vector, seven times: rows 2 and 5 with a flipped input bit, row 4 with C doubled"""
    vk, pr, inputs = H.groth16_setup(golden)
    bad_c = ecc.E1_761.add(pr["c"], pr["c"])
    a = np.repeat(co.pack_761([pr["a"]])[0], 7, axis=0)
    b = np.repeat(co.pack_761([pr["b"]])[0], 7, axis=0)
    c = np.repeat(co.pack_761([pr["c"]])[0], 7, axis=0)
    c[4] = co.pack_761([bad_c])[0][0]
    x = [list(inputs) for _ in range(7)]
    x[2][0] ^= 1
    x[5][1] ^= 1 << 100
    want = np.array([1, 1, 0, 1, 0, 0, 1], dtype=np.uint8)
    proof = bytes.fromhex(golden["groth16_bw6_761"]["proof"])
    ser = [proof] * 7
    ser[4] = proof[:192] + ecc.ser_point(ecc.E1_761, bad_c)
    return vk, a, b, c, co.ints_to_limbs([v for r in x for v in r], 6).reshape(7, 2, 6), want, b"".join(ser)


def test_reference_vector_both_entries_both_modes(gpu, golden):
    vk, a, b, c, x, want, ser = reference_batch(golden)
    rows = co.pack_761([vk["alpha_g1"], vk["beta_g2"], vk["gamma_g2"], vk["delta_g2"]] + list(vk["gamma_abc_g1"]))[0]
    k_limb = gpu.VerifyingKey(rows[0], rows[1], rows[2], rows[3], rows[4:])
    k_ser = gpu.VerifyingKey.from_serialized(bytes.fromhex(golden["groth16_bw6_761"]["vk"]))
    try:
        for k in (k_limb, k_ser):
            for mode in (0, 1):
                assert k.verify(a[:1], b[:1], c[:1], x[:1], mode=mode, key=KEY8).tolist() == [1]
                assert gpu.groth16_verify_last()[0] == ("each", "combined accepted")[mode]
                assert k.verify_serialized(ser[:288], x[:1], mode=mode, key=KEY8).tolist() == [1]
                assert np.array_equal(k.verify(a, b, c, x, mode=mode, key=KEY8), want)
                assert gpu.groth16_verify_last()[0] == ("each", "combined then each")[mode]
                assert np.array_equal(k.verify_serialized(ser, x, mode=mode, key=KEY8), want)
    finally:
        k_limb.release()
        k_ser.release()


@pytest.mark.parametrize("m", [1, 4, 5, 6, 63, 64, 65, 257])
def test_dispatch_borders(gpu, vk2, pool, m):
    """both sides of every border: combined k = m + 3 crosses the latency path's 7 pairs, the 8-pair product and the tree; 63 / 64 / 65 and
    257 are the wave and block borders of the lane kernels and tree levels with an odd count"""
    good, bad = pool
    g, b = gc.take(good, range(m)), gc.take(bad, range(m))
    assert run(vk2, g, 0).tolist() == [1] * m and gpu.groth16_verify_last()[0] == "each"
    assert np.array_equal(run(vk2, b, 0), b.expect)
    assert run(vk2, g, 1).tolist() == [1] * m and gpu.groth16_verify_last()[0] == "combined accepted"
    assert np.array_equal(run(vk2, b, 1), b.expect)
    assert gpu.groth16_verify_last()[0] == ("combined then each" if m > 3 else "combined accepted")      # (the first damaged proof sits at 3)


@pytest.fixture(scope="module")
def large(gpu, key2):
    """16 421 proofs from the library's fixed-base rows, 1 % with C moved; a sample of the rows against the oracle's multiples"""
    rng = ecc.SplitMix64(77)
    proofs = [gc.valid_proof(key2, rng) for _ in range(16421)]
    for i in range(50, 16421, 100):
        proofs[i].c = (proofs[i].c + 1 + i) % R
    b = gc.Batch(key2, proofs, mul=device_mul(gpu))
    G1, G2 = gc.generators()
    idx = [0, 50, 8191, 16383, 16384, 16420]
    assert np.array_equal(b.a[idx], gc.mul_rows(G1, [proofs[i].s for i in idx])[0]) and np.array_equal(b.b[idx], gc.mul_rows(G2, [proofs[i].t for i in idx])[0])
    assert np.array_equal(b.c[idx], gc.mul_rows(G1, [proofs[i].c for i in idx])[0])
    return b


@pytest.mark.parametrize("m", [16384, 16421])
def test_each_across_the_shared_accumulator_threshold(gpu, vk2, large, m):
    b = gc.take(large, range(m))
    got = run(vk2, b, 0)
    assert np.array_equal(got, b.expect) and 0 < b.expect.sum() < m
    for i in (0, 50, 150, m - 1, m - 34, 8191, 8192, 4050):       # the oracle's product on eight of them
        assert gc.oracle_verdict(b, i) == got[i]


@pytest.mark.parametrize("n_in", [0, 1, 2, 3, 8, 64])
def test_input_counts(gpu, n_in):
    """every input count, with the edge inputs in every slot; the window width the key chose, read back from the last record"""
    key = gc.Key(n_in, 300 + n_in)
    rng = ecc.SplitMix64(400 + n_in)
    proofs = [gc.valid_proof(key, rng, x=[v] * n_in) for v in gc.EDGE_INPUTS] + [gc.valid_proof(key, rng) for _ in range(3)]
    if n_in:
        proofs += [gc.special_proof(key, rng, k) for k in ("wrong_input", "input_r", "input_r1")]
    b = gc.Batch(key, proofs)
    vk = load(gpu, key)
    try:
        for mode in (0, 1):
            assert np.array_equal(run(vk, b, mode), b.expect), (n_in, mode)
        c = gpu.groth16_verify_last()[1]
        windows = (377 + 1 + c - 1) // c
        assert c == {64: 7}.get(n_in, 10) and n_in * windows * (1 << (c - 1)) * 224 <= 64 << 20
        for i in range(min(8, b.m) if n_in <= 8 else 2):
            assert gc.oracle_verdict(b, i) == b.expect[i]
    finally:
        vk.release()


def test_65_inputs_refused(gpu):
    z = np.zeros(24, dtype=np.uint64)
    with pytest.raises(gpu.VerifyError) as e:
        gpu.VerifyingKey(z, z, z, z, np.zeros((66, 24), dtype=np.uint64))
    assert e.value.code == 36


def test_every_class_at_every_position(gpu, vk2, key2, pool):
    """65-proof batches: every case class lands on every position once over 48 batches (batch t puts class (i + t) mod 16 at the positions
    i = t mod 3, so (t mod 16, t mod 3) runs through all pairs); the other positions hold valid proofs, and each special flips only its byte"""
    good, _ = pool
    classes = gc.classes_for(key2)
    assert len(classes) == 16
    rng = ecc.SplitMix64(55)
    sp = gc.Batch(key2, [gc.special_proof(key2, rng, k) for k in classes])
    for i in range(16):                                  # the oracle's product on every special, and on eight valid ones in the pool fixture
        assert gc.oracle_verdict(sp, i) == sp.expect[i], classes[i]
    seen = set()
    for t in range(48):
        names = ("a", "a_inf", "b", "b_inf", "c", "c_inf", "inputs", "expect")
        b = gc.take(good, range(65))
        for i in range(t % 3, 65, 3):
            k = (i + t) % 16
            seen.add((i, k))
            for n in names:
                getattr(b, n)[i] = getattr(sp, n)[k]
        got = run(vk2, b, 0)
        assert np.array_equal(got, b.expect), (t, np.nonzero(got != b.expect)[0].tolist())
        if t % 12 == 0:
            assert np.array_equal(run(vk2, b, 1), b.expect), t
            assert gpu.groth16_verify_last()[0] == "combined then each"
    assert len(seen) == 65 * 16
    pair = gc.Batch(key2, list(gc.swapped_pair(key2, rng)))
    b = gc.take(good, range(65))
    for n in ("a", "a_inf", "b", "b_inf", "c", "c_inf", "inputs", "expect"):
        getattr(b, n)[[9, 40]] = getattr(pair, n)
    assert pair.expect.tolist() == [0, 0] and np.array_equal(run(vk2, b, 0), b.expect)


def test_combined_paths_and_exponents(gpu, vk2, key2, pool):
    good, bad = pool
    g = gc.take(good, range(33))
    assert run(vk2, g, 1).tolist() == [1] * 33 and gpu.groth16_verify_last()[0] == "combined accepted"
    assert run(vk2, g, 1).tolist() == [1] * 33 and gpu.groth16_verify_last()[0] == "combined accepted"      # the same key, the same path
    assert run(vk2, g, 1, key=None).tolist() == [1] * 33 and gpu.groth16_verify_last()[0] == "combined accepted"
    b = gc.take(bad, range(33))
    assert np.array_equal(run(vk2, b, 1), b.expect) and gpu.groth16_verify_last()[0] == "combined then each"
    assert np.array_equal(run(vk2, b, 1, key=None), b.expect)
    for m in (1, 2, 65, 300):
        ex = gpu.groth16_draw_exponents(KEY8, m)
        assert co.limbs_to_ints(ex, 2) == gc.exponents_ref(KEY8, m)


def test_combined_cancelling_pair(gpu, vk2, key2, pool):
    """(C_1 + D, C_2 - D) among valid proofs: the unweighted sum would pass; with drawn exponents both are rejected, alone"""
    good, _ = pool
    pair = gc.Batch(key2, list(gc.cancelling_pair(key2, ecc.SplitMix64(13))))
    b = gc.take(good, range(10))
    for n in ("a", "a_inf", "b", "b_inf", "c", "c_inf", "inputs", "expect"):
        getattr(b, n)[[2, 7]] = getattr(pair, n)
    assert b.expect.tolist() == [1, 1, 0, 1, 1, 1, 1, 0, 1, 1]
    for key in (KEY8, None):
        assert np.array_equal(run(vk2, b, 1, key=key), b.expect) and gpu.groth16_verify_last()[0] == "combined then each"
    only = gc.take(b, [2, 7])
    assert run(vk2, only, 1).tolist() == [0, 0] and gpu.groth16_verify_last()[0] == "combined then each"


def test_serialized_entry(gpu, vk2, key2, pool):
    """a proof whose bytes do not decode and one with a point off the subgroup are rejected alone; VK bytes and limb VK agree"""
    good, bad = pool
    b = gc.take(bad, range(12))
    ser = bytearray(b.serialize())
    want = b.expect.copy()
    off1 = bs.random_curve_points(ecc.E1_761, 1, 5)[0]
    off2 = bs.random_curve_points(ecc.E2_761, 1, 6)[0]
    assert not ecc.E1_761.in_subgroup(off1) and not ecc.E2_761.in_subgroup(off2)
    ser[288 * 1:288 * 1 + 96] = ecc.ser_point(ecc.E1_761, off1); want[1] = 0                       # A off the subgroup
    ser[288 * 4 + 96:288 * 4 + 192] = ecc.ser_point(ecc.E2_761, off2); want[4] = 0                 # B off the subgroup
    ser[288 * 6 + 287] |= 0xC0; want[6] = 0                                                         # C: both flags - no encoding
    ser[288 * 8:288 * 8 + 96] = bs.non_residue_x(ecc.E1_761, 9).to_bytes(96, "little"); want[8] = 0   # A: no point has this x
    ser[288 * 9 + 192:288 * 9 + 288] = ecc.ser_point(ecc.E1_761, None); want[9] = 0                # C at infinity: decodes, does not verify
    k_ser = gpu.VerifyingKey.from_serialized(key2.serialize())
    try:
        for mode in (0, 1):
            got = vk2.verify_serialized(bytes(ser), b.inputs, mode=mode, key=KEY8)
            assert np.array_equal(got, want), (mode, got.tolist())
            assert np.array_equal(k_ser.verify_serialized(bytes(ser), b.inputs, mode=mode, key=KEY8), got)
            assert np.array_equal(k_ser.verify(b.a, b.b, b.c, b.inputs, mode=mode, key=KEY8), b.expect)
        g = gc.take(good, range(12))
        assert vk2.verify_serialized(g.serialize(), g.inputs, mode=1, key=KEY8).tolist() == [1] * 12
        assert gpu.groth16_verify_last()[0] == "combined accepted" and gpu.groth16_verify_last()[2][0] > 0      # decoding was timed
    finally:
        k_ser.release()


def test_handles(gpu, vk2, key2, pool):
    good, bad = pool
    b = gc.take(bad, range(20))
    out = {}

    def work(name, mode):
        gpu.use_device(0)
        out[name] = [run(vk2, b, mode) for _ in range(3)]
    th = [threading.Thread(target=work, args=("t%d" % i, i % 2)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert all(np.array_equal(r, b.expect) for v in out.values() for r in v) and len(out) == 2
    # a freed handle and a pointer that never was one are refused
    import ctypes as C
    k = load(gpu, key2)
    h = C.c_void_p(k.h.value)
    assert k.release() == 0
    res = np.zeros(b.m, dtype=np.uint8)
    args = [co._p(b.a), None, co._p(b.b), None, co._p(b.c), None, co._p(np.ascontiguousarray(b.inputs)), C.c_size_t(b.m), C.c_int(0), None, co._p(res)]
    assert gpu.lib().groth16_verify_batch_bw6_761(h, *args) == 2 and gpu.lib().groth16_vk_free(h) == 2
    foreign = np.zeros(64, dtype=np.uint64)
    assert gpu.lib().groth16_verify_batch_bw6_761(co._p(foreign), *args) == 2 and gpu.lib().groth16_vk_free(co._p(foreign)) == 2
    # two keys of different shapes used in turn: the pairing engines see another layout every call
    key5 = gc.Key(5, 0x5155)
    b5 = gc.batch_with(key5, 7, {3: gc.special_proof(key5, ecc.SplitMix64(1), "wrong_c")}, 2)
    k5 = load(gpu, key5)
    try:
        for _ in range(2):
            for mode in (0, 1):
                assert np.array_equal(run(vk2, b, mode), b.expect)
                assert np.array_equal(run(k5, b5, mode), b5.expect)
    finally:
        k5.release()


def test_resources_of_the_lane_kernels():
    """from the build's own resource remarks: k_g16_inputs runs without scratch, as k_fbm_rows; k_g16_scale needs no more than
    k_subgroup761, the ladder it is modelled on"""
    def scratch(unit, kernel):
        txt = open(os.path.join(BUILD, unit + ".remarks.txt")).read()
        m = re.search(r"Function Name: \S*%s\S*.*?ScratchSize \[bytes/lane\]: (\d+)" % kernel, txt, re.S)
        assert m, (unit, kernel)
        return int(m.group(1))
    assert scratch("unit_groth16_verify", "k_g16_inputs") == 0
    assert scratch("unit_groth16_verify", "k_g16_scale") <= scratch("unit_wire761", "k_subgroup761")
