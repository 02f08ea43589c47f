"""GPU (-m gpu): wide BLS12-377 verifying keys (groth16_vk_load_bls12_377_wide: up to 1024 public inputs), the many-lane input sum
k_g16_inputs_lanes<G16Bls> at every width, and groth16_hash_helper_verify_bls12_377 - on proofs whose verdict is known by construction
(tests/groth16_verify377_cases.py: an accepted valid proof proves the whole input sum), and end to end behind the library's own setup and
prover at 18 epochs, the first size the narrow loaders refuse.

Mutation pairs: a lane that skips its last input, or a fold round that drops a partner -> every valid proof of test_every_width is rejected;
slots of one proof overlapping the next proof's in a shared workgroup -> the m = 64 / L +- 1 cases; the fold's doubling or cancelling branch
taken for a general addition -> test_fold_branches_on_the_device; the range test lost in a lane other than 0 -> its input >= r cases."""
import ctypes as C
import random
import threading
import numpy as np
import pytest
import torch  # noqa: F401  (before the library: both must share one HIP runtime)
from oracle.py import ecc
from oracle import cpu_oracle as co
from tests import groth16_verify377_cases as gc
from tests import groth16_wide_cases as wc
import hashbits_cases as hc
import hashbits_ref as hr

pytestmark = pytest.mark.gpu
R = gc.R
KEY8 = np.array([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0, 0x082EFA98, 0xEC4E6C89], dtype=np.uint32)
NAMES = ("a", "a_inf", "b", "b_inf", "c", "c_inf", "inputs", "expect")
CURVE = "bls12_377"


def load(gpu, key, wide=True):
    return gpu.VerifyingKey(key.alpha, key.beta, key.gamma, key.delta, key.abc, curve=CURVE, wide=wide)


def run(vk, b, mode=0, key=KEY8):
    return vk.verify(b.a, b.b, b.c, b.inputs, mode=mode, key=key, a_inf=b.a_inf, b_inf=b.b_inf, c_inf=b.c_inf)


def put(b, i, src, k):
    """proof k of the batch src at position i of b"""
    for n in NAMES:
        getattr(b, n)[i] = getattr(src, n)[k]


@pytest.fixture(autouse=True)
def the_rule_afterwards(gpu):
    yield
    gpu.groth16_set_input_lanes(0)


@pytest.fixture(scope="module")
def key1024():
    """one key of 1024 inputs; every smaller wide key of this module is a prefix of it (wc.sub_key)"""
    return gc.Key(1024, 0x61DE)


@pytest.fixture(scope="module")
def loaded(gpu, key1024):
    """the loaded handle of the prefix key of n_in inputs, kept for the module"""
    made = {}

    def get(n_in):
        if n_in not in made:
            key = wc.sub_key(key1024, n_in)
            made[n_in] = (key, load(gpu, key))
        return made[n_in]
    yield get
    for _, vk in made.values():
        vk.release()


def wrong_last_input(key, p):
    q = gc.Proof(p.s, p.t, p.c, p.x, "wrong_input")
    q.x[-1] = (q.x[-1] + 1) % R
    return q


@pytest.fixture(scope="module")
def pools(key1024):
    """per input count: 66 valid proofs and the same proofs with their LAST input moved by one (a lane other than 0 for every L >= 2)"""
    made = {}

    def get(n_in):
        if n_in not in made:
            key = wc.sub_key(key1024, n_in)
            good = gc.batch_with(key, 66, {}, 900 + n_in)
            bad = gc.Batch(key, [wrong_last_input(key, p) for p in good.proofs])
            assert good.expect.all() and not bad.expect.any()
            assert gc.oracle_verdict(good, 0) == 1 and gc.oracle_verdict(bad, 0) == 0
            made[n_in] = (good, bad)
        return made[n_in]
    return get


@pytest.mark.parametrize("n_in", [65, 70, 71, 128, 129, 221, 222, 381, 382, 642, 643, 1024])
def test_borders_of_the_window_rule(gpu, key1024, n_in):
    """either side of every border of the window rule up to the limit: a valid proof with random inputs, one with the edge inputs (all
    2^252 - 1 among them: the carry runs through every window of every base), one with one input changed; the window bits and the lanes of
    the last record are the restated rules'"""
    key = wc.sub_key(key1024, n_in)
    rng = ecc.SplitMix64(500 + n_in)
    edge = [gc.EDGE_INPUTS[j % len(gc.EDGE_INPUTS)] for j in range(n_in)]
    moved = gc.valid_proof(key, rng)
    moved.x[n_in // 2] = (moved.x[n_in // 2] + 1) % R
    b = gc.Batch(key, [gc.valid_proof(key, rng), gc.valid_proof(key, rng, x=edge), moved])
    assert b.expect.tolist() == [1, 1, 0]
    vk = load(gpu, key)
    try:
        for mode in (0, 1):
            assert run(vk, b, mode).tolist() == [1, 1, 0], (n_in, mode)
            assert gpu.groth16_verify_last()[1] == wc.window_bits_wide(n_in)
            assert gpu.groth16_inputs_last() == (wc.pick_lanes(n_in, 3), n_in)
    finally:
        vk.release()


@pytest.mark.parametrize("n_in", [65, 509])
@pytest.mark.parametrize("L", wc.LANES)
def test_every_width(gpu, loaded, pools, n_in, L):
    """every forced width on both sides of the proofs-per-workgroup border (64 / L proofs share a workgroup below 64 lanes): the verdicts are
    the construction's with one invalid proof at the first and at the last position"""
    key, vk = loaded(n_in)
    good, bad = pools(n_in)
    gpu.groth16_set_input_lanes(L)
    per = 64 // L
    for m in sorted({1, per - 1, per, per + 1} - {0}) if L < 64 else (1, 2, 3):
        for spots in ((), (0,), (m - 1,)) if m == 1 else ((0,), (m - 1,)):
            b = gc.take(good, range(m))
            for i in spots:
                put(b, i, bad, i)
            got = run(vk, b)
            assert np.array_equal(got, b.expect) and b.expect.sum() == m - len(spots), (L, m, spots, got.tolist())
            assert gpu.groth16_inputs_last() == (L, n_in)


def test_every_class_at_every_position(gpu, loaded, pools):
    """n_in = 65 under the rule: every case class on every position of a 9-proof batch in mode 0; in mode 1 three positions a batch, every
    position over three batches per class, with the path the record names; the cancelling pair"""
    key, vk = loaded(65)
    good, _ = pools(65)
    classes = gc.classes_for(key)
    rng = ecc.SplitMix64(56)
    sp = gc.Batch(key, [gc.special_proof(key, rng, k) for k in classes])
    for i in range(len(classes)):                        # the oracle's product of the four pairs on every special
        assert gc.oracle_verdict(sp, i) == sp.expect[i], classes[i]
    n = len(classes)
    for t in range(n):                                   # batch t: class (i + t) mod n at position i - every class at every position over n batches
        b = gc.take(good, range(9))
        for i in range(9):
            put(b, i, sp, (i + t) % n)
        got = run(vk, b, 0)
        assert np.array_equal(got, b.expect), (t, got.tolist())
        assert gpu.groth16_verify_last()[0] == "each" and gpu.groth16_inputs_last() == (wc.pick_lanes(65, 9), 65)
    seen = set()
    for k in range(n):                                   # mode 1: class k at the positions r, r + 3, r + 6 for r = 0, 1, 2 - every position again
        for r in range(3):
            b = gc.take(good, range(9))
            for i in (r, r + 3, r + 6):
                put(b, i, sp, k)
                seen.add((k, i))
            got = run(vk, b, 1)
            assert np.array_equal(got, b.expect), (classes[k], r, got.tolist())
            accepted = sp.expect[k] or classes[k] in ("input_r", "input_r1")
            assert gpu.groth16_verify_last()[0] == ("combined accepted" if accepted else "combined then each"), (classes[k], r)
    assert len(seen) == 9 * n
    pair = gc.Batch(key, list(gc.cancelling_pair(key, ecc.SplitMix64(13))))
    b = gc.take(good, range(9))
    put(b, 2, pair, 0)
    put(b, 7, pair, 1)
    assert b.expect.tolist() == [1, 1, 0, 1, 1, 1, 1, 0, 1]
    assert np.array_equal(run(vk, b, 1), b.expect) and gpu.groth16_verify_last()[0] == "combined then each"
    assert np.array_equal(run(vk, b, 0), b.expect)


@pytest.mark.parametrize("L", [4, 256])
def test_fold_branches_on_the_device(gpu, loaded, L):
    """valid proofs over the inputs that make two partials equal, opposite or the identity (tests/groth16_wide_cases.py): accepted, so the
    fold gave the sum; the same proofs with one more on a base are rejected.  An input >= r in lane 0, in the last lane and in the last input
    takes out that proof alone"""
    key, vk = loaded(L + 1)
    cases = wc.fold_branch_inputs(key, L)
    names = sorted(cases)
    rng = ecc.SplitMix64(700 + L)
    proofs = [gc.valid_proof(key, rng, x=cases[k], kind=k) for k in names]
    off = [gc.Proof(p.s, p.t, p.c, [(v + 1) % R if j == 1 else v for j, v in enumerate(p.x)], "moved") for p in proofs]
    big = []
    for j in (0, L - 1, L):                              # lane 0, the last lane, the last input (lane 0's second)
        p = gc.valid_proof(key, rng, x=[0 if k == j else 3 + k for k in range(L + 1)], kind="input_r")
        p.x[j] = R
        big.append(p)
    gpu.groth16_set_input_lanes(L)
    b = gc.Batch(key, proofs + off + big + [gc.valid_proof(key, rng)])
    assert b.expect.tolist() == [1] * len(names) + [0] * len(names) + [0, 0, 0, 1]
    for mode in (0, 1):
        got = run(vk, b, mode)
        assert np.array_equal(got, b.expect), (L, mode, [(proofs + off + big)[i].kind for i in np.nonzero(got != b.expect)[0] if i < b.m - 1])
    assert gpu.groth16_inputs_last() == (L, L + 1)
    for p in big:                                        # the range test, not the sum: the same proof with the input below r verifies
        q = gc.Batch(key, [gc.Proof(p.s, p.t, p.c, [v % R for v in p.x])])
        assert q.expect.tolist() == [1] and run(vk, q).tolist() == [1]


def test_narrow_key_with_a_forced_width(gpu):
    """three inputs over 2, 4 and 8 lanes (lanes without inputs carry the identity), through the OLD loader: the verdicts of one lane"""
    key = gc.Key(3, 0x333)
    rng = ecc.SplitMix64(34)
    proofs = [gc.valid_proof(key, rng) for _ in range(20)] + [gc.special_proof(key, rng, k) for k in ("wrong_input", "input_r", "edge_ones", "edge_rm1", "inf_a_accept")]
    b = gc.Batch(key, proofs)
    vk = load(gpu, key, wide=False)
    try:
        one = run(vk, b)
        assert gpu.groth16_inputs_last() == (1, 3) and np.array_equal(one, b.expect)
        for L in (2, 4, 8):
            gpu.groth16_set_input_lanes(L)
            for mode in (0, 1):
                assert np.array_equal(run(vk, b, mode), one), (L, mode)
            assert gpu.groth16_inputs_last() == (L, 3)
    finally:
        vk.release()


def test_loaders_and_handles(gpu, key1024, loaded, pools):
    """the serialized wide loader gives the limb loader's verdicts; a key of 64 inputs gives the same verdicts through either loader and keeps
    the one-lane kernel; 1025 inputs are refused with 36 by both wide loaders and 65 by both old ones; a BW6-761 entry refuses a wide handle"""
    key, vk = loaded(65)
    good, bad = pools(65)
    b = gc.take(good, range(9))
    put(b, 4, bad, 4)
    ser = gpu.VerifyingKey.from_serialized(key.serialize(), curve=CURVE, wide=True)
    try:
        assert ser.n_inputs == 65
        for mode in (0, 1):
            want = run(vk, b, mode)
            assert np.array_equal(want, b.expect) and np.array_equal(run(ser, b, mode), want)
            assert np.array_equal(ser.verify_serialized(b.serialize(), b.inputs, mode=mode, key=KEY8), want)
    finally:
        ser.release()
    key64 = wc.sub_key(key1024, 64)
    rng = ecc.SplitMix64(64)
    b64 = gc.Batch(key64, [gc.valid_proof(key64, rng), gc.special_proof(key64, rng, "wrong_input"), gc.special_proof(key64, rng, "edge_ones")])
    old, new = load(gpu, key64, wide=False), load(gpu, key64, wide=True)
    try:
        for mode in (0, 1):
            assert run(old, b64, mode).tolist() == [1, 0, 1] == run(new, b64, mode).tolist()
            assert gpu.groth16_inputs_last() == (1, 64) and gpu.groth16_verify_last()[1] == 9
    finally:
        old.release()
        new.release()
    reps = np.concatenate([key1024.abc, key1024.abc[:1]])            # 1026 rows: 1025 inputs
    for make in (lambda: gpu.VerifyingKey(key.alpha, key.beta, key.gamma, key.delta, reps, curve=CURVE, wide=True),
                 lambda: gpu.VerifyingKey.from_serialized(key.serialize(reps), curve=CURVE, wide=True),
                 lambda: load(gpu, key, wide=False),
                 lambda: gpu.VerifyingKey.from_serialized(key.serialize(), curve=CURVE, wide=False)):
        with pytest.raises(gpu.VerifyError) as e:
            make()
        assert e.value.code == gpu.VK_ERR_INPUTS == 36
    z = np.zeros((1, 24), dtype=np.uint64)
    out = np.zeros(1, dtype=np.uint8)
    p = co._p
    assert gpu.lib().groth16_verify_batch_bw6_761(vk.h, p(z), None, p(z), None, p(z), None, p(np.zeros((1, 65, 6), dtype=np.uint64)), C.c_size_t(1), C.c_int(0), None, p(out)) == 2
    assert gpu.lib().groth16_verify_batch_bw6_761_serialized(vk.h, p(np.zeros(288, dtype=np.uint8)), p(np.zeros((1, 65, 6), dtype=np.uint64)), C.c_size_t(1), C.c_int(0), None,
                                                             p(out)) == 2
    assert run(vk, gc.take(good, range(2))).tolist() == [1, 1]       # ... and still serves


def test_two_threads_on_one_wide_handle(gpu, loaded, pools):
    """two threads verify on one handle, one under a forced width; the setter at 0 restores the rule"""
    key, vk = loaded(509)
    good, bad = pools(509)
    b = gc.take(good, range(5))
    put(b, 3, bad, 3)
    gpu.groth16_set_input_lanes(16)
    got, errs = {}, []

    def work(t):
        try:
            gpu.use_device(0)
            got[t] = [run(vk, b, mode=t % 2).tolist() for _ in range(3)]
        except Exception as e:                       # noqa: BLE001
            errs.append(e)
    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs and got[0] == got[1] == [b.expect.tolist()] * 3
    assert gpu.groth16_inputs_last() == (16, 509)
    gpu.groth16_set_input_lanes(0)
    assert np.array_equal(run(vk, b), b.expect) and gpu.groth16_inputs_last() == (wc.pick_lanes(509, 5), 509)


# ---- end to end at 18 epochs: 65 public inputs, the first size the narrow loaders refuse
def test_end_to_end_helper_proof_of_18_epochs(gpu):
    """hash_to_bits_r1cs_load -> setup -> the helper proof in one call -> its 192 bytes -> groth16_hash_helper_verify_bls12_377, which makes
    the inputs from the rows itself: (proof, rows), (proof, rows of other messages), (proof of other messages, rows), (other, other) give
    [1, 0, 0, 1], as verify_serialized on the wide key with hash_to_bits_public_inputs does; one flipped row byte is rejected; a key of
    another input count is refused with 2.  Both bit orders."""
    m = 18
    c = hc.Circuit(gpu, m)
    v = c.vk_rows
    vk = gpu.VerifyingKey(v["alpha_g1"], v["beta_g2"], v["gamma_g2"], v["delta_g2"], v["gamma_abc_g1"], curve=CURVE, wide=True)
    k61 = gc.Key(61, 0x17)                                           # the input count of 17 epochs
    vk61 = load(gpu, k61)
    try:
        assert vk.n_inputs == c.sizes["n_inputs"] - 1 == 65
        rows, other = hc.rows_for(m, 5), hc.rows_for(m, 6)
        for order in (0, 1):
            ser = gpu.groth16_serialize_proof(*gpu.hash_helper_prove(c.key, c.r, rows, order, c.log_n, c.consts)[:3], curve=CURVE)
            ser_other = gpu.groth16_serialize_proof(*gpu.hash_helper_prove(c.key, c.r, other, order, c.log_n, c.consts)[:3], curve=CURVE)
            proofs = ser + ser + ser_other + ser_other
            all_rows = np.concatenate([rows, other, rows, other])
            for mode in (0, 1):
                got = gpu.hash_helper_verify(vk, all_rows, m, proofs, bit_order=order, mode=mode, key=KEY8)
                assert got.tolist() == [1, 0, 0, 1], (order, mode)
                assert gpu.groth16_inputs_last() == (wc.pick_lanes(65, 4), 65)
            x = gpu.hash_to_bits_public_inputs(all_rows, 4, m, order)
            assert np.array_equal(x[0], co.ints_to_limbs(hr.instance(rows, order)[1:], 4))
            assert vk.verify_serialized(proofs, x, mode=0, key=KEY8).tolist() == [1, 0, 0, 1]
            assert gpu.hash_helper_verify(vk, all_rows, m, proofs, bit_order=1 - order).tolist() == [0, 0, 0, 0]       # the other bit order: other inputs
            flipped = rows.copy()
            flipped[m - 1, 47] ^= 0x80
            assert gpu.hash_helper_verify(vk, np.concatenate([flipped, rows]), m, ser + ser, bit_order=order).tolist() == [0, 1]
        with pytest.raises(gpu.VerifyError) as e:
            gpu.hash_helper_verify(vk61, rows, m, ser)
        assert e.value.code == 2
        with pytest.raises(gpu.VerifyError) as e:
            gpu.hash_helper_verify(vk, rows[:17], 17, ser)
        assert e.value.code == 2
    finally:
        vk.release()
        vk61.release()
        c.release()
