"""GPU (-m gpu): groth16_verify_batch_bls12_377 - m Groth16 proofs over BLS12-377 under one verifying key, per proof ("each") and combined -
on proofs whose verdict is known by construction (tests/groth16_verify377_cases.py), with samples against the oracle's own product of the four
pairs, and end to end behind the library's own setup and prover.

Mutation pairs: all r_i = 1 -> test_combined_cancelling_pair; dropping the input range test -> the input_r / input_r1 classes of
test_every_class_at_every_position; an off-by-one in the window count -> its edge_ones class and test_input_counts; the 8 / 9-pair border of
the combined product -> m = 5 / 6 of test_dispatch_borders; a handle of the other curve followed instead of refused -> test_handles."""
import ctypes as C
import random
import threading
import numpy as np
import pytest
import torch  # noqa: F401  (before the library: both must share one HIP runtime)
from oracle.py import ecc
from oracle import cpu_oracle as co
from tests import groth16_verify377_cases as gc
from tests import groth16_verify_cases as gc761
import groth16_setup_ref as gs
import r1cs_cases as rc
from oracle.py import groth16_prover as gp

pytestmark = pytest.mark.gpu
R = gc.R
KEY8 = np.array([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0, 0x082EFA98, 0xEC4E6C89], dtype=np.uint32)
NAMES = ("a", "a_inf", "b", "b_inf", "c", "c_inf", "inputs", "expect")
CURVE = "bls12_377"


def load(gpu, key):
    return gpu.VerifyingKey(key.alpha, key.beta, key.gamma, key.delta, key.abc, curve=CURVE)


def run(vk, b, mode, key=KEY8):
    return vk.verify(b.a, b.b, b.c, b.inputs, mode=mode, key=key, a_inf=b.a_inf, b_inf=b.b_inf, c_inf=b.c_inf)


def device_mul(gpu):
    """the multiples of a batch from the library's fixed-base rows (the large batches; a sample is compared with the oracle's)"""
    def mul(gen, scalars, on_g2):
        xy, inf = gpu.fixed_base_mul("bls12_377_g2" if on_g2 else "bls12_377_g1", gen, co.ints_to_limbs([int(k) % R for k in scalars], 4))
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
    bad.inputs = gc.input_limbs(proofs, 2)
    bad.expect = np.array([p.expect(key2) for p in proofs], dtype=np.uint8)
    assert good.expect.all() and bad.expect.sum() == 257 - len(range(3, 257, 7))
    for i in range(8):                                   # the sample against the oracle's product (positions 0 .. 7 hold a damaged proof)
        assert gc.oracle_verdict(good, i) == 1 and gc.oracle_verdict(bad, i) == bad.expect[i]
    return good, bad


@pytest.mark.parametrize("m", [1, 2, 5, 6, 63, 64, 65, 257])
def test_dispatch_borders(gpu, vk2, pool, m):
    """both sides of every border: combined k = m + 3 crosses from the 8-pair product (m = 5) to the pairwise tree (m = 6); 63 / 64 / 65 and
    257 are the wave and block borders of the lane kernels and tree levels with an odd count.  The path is named by the last record"""
    good, bad = pool
    g, b = gc.take(good, range(m)), gc.take(bad, range(m))
    assert run(vk2, g, 0).tolist() == [1] * m and gpu.groth16_verify_last()[0] == "each"
    assert np.array_equal(run(vk2, b, 0), b.expect) and gpu.groth16_verify_last()[0] == "each"
    assert run(vk2, g, 1).tolist() == [1] * m and gpu.groth16_verify_last()[0] == "combined accepted"
    assert np.array_equal(run(vk2, b, 1), b.expect)
    assert gpu.groth16_verify_last()[0] == ("combined then each" if m > 3 else "combined accepted")      # (the first damaged proof sits at 3)


@pytest.fixture(scope="module")
def large(gpu, key2):
    """16 421 proofs from the library's fixed-base rows, 1 % with C moved; six of the rows against the oracle's multiples"""
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
    """from 16 384 proofs mode 0 runs the shared-accumulator kernel (four pairs per product): both sides of a product count that is no
    multiple of anything"""
    b = gc.take(large, range(m))
    got = run(vk2, b, 0)
    assert gpu.groth16_verify_last()[0] == "each"
    assert np.array_equal(got, b.expect) and 0 < b.expect.sum() < m
    for i in (0, 50, 150, m - 1, m - 34, 8191, 8192, 4050):       # the oracle's product on eight of them
        assert gc.oracle_verdict(b, i) == got[i]


def test_combined_at_16421_all_valid(gpu, vk2, large):
    idx = np.array([i for i in range(16421) if large.expect[i]][:16421 - 164] + [0] * 164)      # the all-valid rows, padded to 16 421 with a valid one
    b = gc.take(large, idx)
    assert b.m == 16421 and b.expect.all()
    assert run(vk2, b, 1).tolist() == [1] * 16421 and gpu.groth16_verify_last()[0] == "combined accepted"


@pytest.mark.parametrize("n_in", [0, 1, 2, 3, 8, 39, 40, 45, 46, 64])
def test_input_counts(gpu, n_in):
    """every input count, with the edge inputs (all 2^252 - 1 among them) in every slot and random ones; the window width the key chose, read
    back from the last record, is the restated rule's (39 / 40 is its border; 45 / 46 would be with 112-byte entries)"""
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
        assert c == gc.window_bits(n_in) == (10 if n_in <= 39 else 9)
        assert n_in * gc.fb_windows(253, c) * (1 << (c - 1)) * gc.ENTRY_BYTES <= gc.TABLE_BUDGET
        for i in range(min(8, b.m) if n_in <= 8 else 2):
            assert gc.oracle_verdict(b, i) == b.expect[i]
    finally:
        vk.release()


def test_65_inputs_refused(gpu):
    z = np.zeros(24, dtype=np.uint64)
    with pytest.raises(gpu.VerifyError) as e:
        gpu.VerifyingKey(z[:12], z, z, z, np.zeros((66, 12), dtype=np.uint64), curve=CURVE)
    assert e.value.code == 36


def test_every_class_at_every_position(gpu, vk2, key2, pool):
    """65-proof batches, mode 0: every case class lands on every position once over 48 batches (batch t puts class (i + t) mod 16 at the
    positions i = t mod 3, so (t mod 16, t mod 3) runs through all pairs); the other positions hold valid proofs, and each special flips only
    its byte.  Mode 1: every class at the positions 0, 31 and 64, one batch per class"""
    good, _ = pool
    classes = gc.classes_for(key2)
    assert len(classes) == 16
    rng = ecc.SplitMix64(55)
    sp = gc.Batch(key2, [gc.special_proof(key2, rng, k) for k in classes])
    for i in range(16):                                  # the oracle's product on every special, and on eight valid ones in the pool fixture
        assert gc.oracle_verdict(sp, i) == sp.expect[i], classes[i]
    seen = set()
    for t in range(48):
        b = gc.take(good, range(65))
        for i in range(t % 3, 65, 3):
            k = (i + t) % 16
            seen.add((i, k))
            for n in NAMES:
                getattr(b, n)[i] = getattr(sp, n)[k]
        got = run(vk2, b, 0)
        assert np.array_equal(got, b.expect), (t, np.nonzero(got != b.expect)[0].tolist())
    assert len(seen) == 65 * 16
    for k in range(16):
        b = gc.take(good, range(65))
        for i in (0, 31, 64):
            for n in NAMES:
                getattr(b, n)[i] = getattr(sp, n)[k]
        got = run(vk2, b, 1)
        assert np.array_equal(got, b.expect), (classes[k], np.nonzero(got != b.expect)[0].tolist())
        # (an input that is not below r takes its proof out of the combination, which then accepts the others: no second pass)
        accepted = sp.expect[k] or classes[k] in ("input_r", "input_r1")
        assert gpu.groth16_verify_last()[0] == ("combined accepted" if accepted else "combined then each"), classes[k]
    pair = gc.Batch(key2, list(gc.swapped_pair(key2, rng)))
    b = gc.take(good, range(65))
    for n in NAMES:
        getattr(b, n)[[9, 40]] = getattr(pair, n)
    assert pair.expect.tolist() == [0, 0] and np.array_equal(run(vk2, b, 0), b.expect)


def test_exponents(gpu):
    """celo_amd_groth16_draw_exponents (one draw for both curves) equals the restated rule"""
    for m in (1, 2, 65, 300):
        assert co.limbs_to_ints(gpu.groth16_draw_exponents(KEY8, m), 2) == gc.exponents_ref(KEY8, m)


def test_combined_cancelling_pair(gpu, vk2, key2, pool):
    """(C_1 + D, C_2 - D) among valid proofs: the unweighted sum would pass; with drawn exponents the combination is rejected, and then each
    of the two fails alone"""
    good, _ = pool
    pair = gc.Batch(key2, list(gc.cancelling_pair(key2, ecc.SplitMix64(13))))
    b = gc.take(good, range(10))
    for n in NAMES:
        getattr(b, n)[[2, 7]] = getattr(pair, n)
    assert b.expect.tolist() == [1, 1, 0, 1, 1, 1, 1, 0, 1, 1]
    for key in (KEY8, None):
        assert np.array_equal(run(vk2, b, 1, key=key), b.expect) and gpu.groth16_verify_last()[0] == "combined then each"
    only = gc.take(b, [2, 7])
    assert run(vk2, only, 1).tolist() == [0, 0] and gpu.groth16_verify_last()[0] == "combined then each"
    assert run(vk2, only, 0).tolist() == [0, 0]


def test_serialized_entry(gpu, vk2, key2, pool):
    """65 proofs through verify_serialized give the verdicts of the limb entry; a proof whose A has an x no point has, one whose B is on the
    curve and off the subgroup and one whose C ends in an invalid flag byte get verdict 0, each alone; VK bytes and limb VK agree"""
    good, bad = pool
    b = gc.take(bad, range(65))
    ser = bytearray(b.serialize())
    assert len(ser) == 65 * 192
    for mode in (0, 1):
        assert np.array_equal(vk2.verify_serialized(bytes(ser), b.inputs, mode=mode, key=KEY8), run(vk2, b, mode))
    want = b.expect.copy()
    assert want[[7, 8, 9, 19, 20, 21, 28, 29, 30, 32, 33, 34, 39, 40, 41]].all()      # the damaged proofs and their neighbours are valid ones
    off2 = gc.off_subgroup_point(True, 6)
    ser[192 * 8:192 * 8 + 48] = gc.non_residue_x(9).to_bytes(48, "little"); want[8] = 0                  # A: no point has this x
    ser[192 * 20 + 48:192 * 20 + 144] = ecc.ser_point(ecc.E2_377, off2); want[20] = 0                    # B on the curve, off the subgroup
    ser[192 * 29 + 191] |= 0xC0; want[29] = 0                                                            # C: both flags - no encoding
    off1 = gc.off_subgroup_point(False, 5)
    ser[192 * 33:192 * 33 + 48] = ecc.ser_point(ecc.E1_377, off1); want[33] = 0                          # A off the subgroup
    ser[192 * 40 + 144:192 * 40 + 192] = ecc.ser_point(ecc.E1_377, None); want[40] = 0                   # C at infinity: decodes, does not verify
    assert b.expect[40] == 1
    k_ser = gpu.VerifyingKey.from_serialized(key2.serialize(), curve=CURVE)
    try:
        for mode in (0, 1):
            got = vk2.verify_serialized(bytes(ser), b.inputs, mode=mode, key=KEY8)
            assert np.array_equal(got, want), (mode, np.nonzero(got != want)[0].tolist())
            assert np.array_equal(k_ser.verify_serialized(bytes(ser), b.inputs, mode=mode, key=KEY8), got)
            assert np.array_equal(k_ser.verify(b.a, b.b, b.c, b.inputs, mode=mode, key=KEY8), b.expect)
        g = gc.take(good, range(12))
        assert vk2.verify_serialized(g.serialize(), g.inputs, mode=1, key=KEY8).tolist() == [1] * 12
        assert gpu.groth16_verify_last()[0] == "combined accepted" and gpu.groth16_verify_last()[2][0] > 0      # decoding was timed
    finally:
        k_ser.release()


# ---- end to end: the library's own setup, prover and proof writer in front of the verifier
def domain_consts(log_n):
    p = gs.FIELDS[CURVE]
    k = gp.domain_constants(log_n, gs.root_of_unity(CURVE, log_n), gs.coset_generator(p), p)
    return {name: co.to_mont([v], p)[0] for name, v in k.items()}


@pytest.mark.parametrize("size", ["toy", "chain_62"])
def test_end_to_end_through_the_librarys_prover(gpu, size):
    """groth16_setup_r1cs_bls12_377 -> prove_r1cs -> groth16_serialize_proof_bls12_377 -> both verify entries in both modes: the true public
    inputs are accepted, one changed input and the proof of an unsatisfying assignment are rejected; the 192 bytes are the oracle's"""
    case = rc.toy(CURVE) if size == "toy" else rc.chain(CURVE, 62)
    p, log_n = case.p, case.log_n()
    z = gs.toy_witness(7, p) if size == "toy" else gs.squaring_witness(case.m, 7, p)
    rng = random.Random(11)
    tau, toxic = rng.randrange(2, p), [rng.randrange(1, p) for _ in range(4)]
    r = gpu.R1CS.load(case.curve, case.m, case.n_vars, case.n_inputs, case.csr())
    try:
        out = gpu.groth16_setup_r1cs(r, log_n, rc.mont([gs.root_of_unity(CURVE, log_n)], p)[0], rc.mont([tau], p)[0], rc.mont(toxic, p),
                                     gs.pack(CURVE, 1, [ecc.G1_377])[0][0], gs.pack(CURVE, 2, [ecc.G2_377])[0][0], want_rows=False, want_key=True)
        key, v = out["key"], out["vk"]
        vk = gpu.VerifyingKey(v["alpha_g1"], v["beta_g2"], v["gamma_g2"], v["delta_g2"], v["gamma_abc_g1"], curve=CURVE)
        try:
            assert vk.n_inputs == case.n_inputs - 1
            consts = domain_consts(log_n)
            bad = list(z)
            bad[3] = (bad[3] + 1) % p
            assert r.check(rc.mont(z, p)) == -1 and r.check(rc.mont(bad, p)) >= 0
            jac = [key.prove_r1cs(r, rc.mont(w, p), log_n, consts) for w in (z, bad)]
            ser = [gpu.groth16_serialize_proof(*j, curve=CURVE) for j in jac]
            pts = [tuple(co.jac_to_affine(o, k) for o, k in zip(j, ("g1_377", "g2_377", "g1_377"))) for j in jac]
            for s, (A, B, Cp) in zip(ser, pts):
                assert s == ecc.ser_point(ecc.E1_377, A) + ecc.ser_point(ecc.E2_377, B) + ecc.ser_point(ecc.E1_377, Cp)
            # three proofs in one call: (true proof, true inputs), (true proof, one changed input), (proof of the unsatisfying assignment, true inputs)
            pub = list(z[1:case.n_inputs])
            wrong = [(pub[0] + 1) % p] + pub[1:]
            x = co.ints_to_limbs(pub + wrong + pub, 4).reshape(3, vk.n_inputs, 4)
            a = np.concatenate([co.pack_g1_377([pts[i][0]])[0] for i in (0, 0, 1)])
            b = np.concatenate([co.pack_g2_377([pts[i][1]])[0] for i in (0, 0, 1)])
            c = np.concatenate([co.pack_g1_377([pts[i][2]])[0] for i in (0, 0, 1)])
            for mode in (0, 1):
                assert vk.verify(a, b, c, x, mode=mode, key=KEY8).tolist() == [1, 0, 0]
                assert vk.verify_serialized(ser[0] + ser[0] + ser[1], x, mode=mode, key=KEY8).tolist() == [1, 0, 0]
                assert vk.verify_serialized(ser[0], x[:1], mode=mode, key=KEY8).tolist() == [1]
                assert gpu.groth16_verify_last()[0] == ("each", "combined accepted")[mode]
        finally:
            vk.release()
            key.release()
    finally:
        r.release()


def test_handles(gpu, vk2, key2, pool):
    good, bad = pool
    b = gc.take(bad, range(20))
    single = [run(vk2, b, mode) for mode in (0, 1)]
    assert all(np.array_equal(s, b.expect) for s in single)
    out = {}

    def work(name, mode):
        gpu.use_device(0)
        out[name] = [run(vk2, b, mode) for _ in range(3)]
    th = [threading.Thread(target=work, args=("t%d" % i, i % 2)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert len(out) == 2 and all(np.array_equal(r, single[int(name[1:]) % 2]) for name, v in out.items() for r in v)
    # a freed handle and a pointer that never was one are refused
    k = load(gpu, key2)
    h = C.c_void_p(k.h.value)
    assert k.release() == 0
    res = np.full(b.m, 7, dtype=np.uint8)
    args = [co._p(b.a), None, co._p(b.b), None, co._p(b.c), None, co._p(np.ascontiguousarray(b.inputs)), C.c_size_t(b.m), C.c_int(0), None, co._p(res)]
    lib = gpu.lib()
    assert lib.groth16_verify_batch_bls12_377(h, *args) == 2 and lib.groth16_vk_free(h) == 2
    foreign = np.zeros(64, dtype=np.uint64)
    assert lib.groth16_verify_batch_bls12_377(co._p(foreign), *args) == 2 and lib.groth16_vk_free(co._p(foreign)) == 2
    # m == 0 returns 0 and touches nothing
    args0 = list(args)
    args0[7] = C.c_size_t(0)
    assert lib.groth16_verify_batch_bls12_377(vk2.h, *args0) == 0 and (res == 7).all()
    # a handle of the other curve: 2 from either side, limb and serialized entries, before anything is read
    key761 = gc761.Key(2, 0x6116)
    k761 = gpu.VerifyingKey(key761.alpha, key761.beta, key761.gamma, key761.delta, key761.abc)
    try:
        assert lib.groth16_verify_batch_bls12_377(k761.h, *args) == 2
        assert lib.groth16_verify_batch_bw6_761(vk2.h, *args) == 2
        ser = np.zeros(288 * b.m, dtype=np.uint8)
        tail = [co._p(np.ascontiguousarray(b.inputs)), C.c_size_t(b.m), C.c_int(0), None, co._p(res)]
        assert lib.groth16_verify_batch_bls12_377_serialized(k761.h, co._p(ser), *tail) == 2
        assert lib.groth16_verify_batch_bw6_761_serialized(vk2.h, co._p(ser), *tail) == 2
        assert (res == 7).all()
        # ... and each handle still serves its own curve, in turn
        b761 = gc761.batch_with(key761, 3, {1: gc761.special_proof(key761, ecc.SplitMix64(1), "wrong_c")}, 2)
        for mode in (0, 1):
            assert np.array_equal(run(vk2, b, mode), b.expect)
            assert np.array_equal(k761.verify(b761.a, b761.b, b761.c, b761.inputs, mode=mode, key=KEY8), b761.expect)
    finally:
        k761.release()
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
