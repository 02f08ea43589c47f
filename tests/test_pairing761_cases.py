"""CPU (-m "not gpu"): the inputs of the BW6-761 pairing tests (tests/pairing761_cases.py) are what they claim to be, checked WITHOUT
the code under test: on small batches built the Python way the oracle (oracle/cpu: the arkworks restatement) returns exactly the verdict
each product was constructed to have, for every product class.  Measured: the C oracle takes about 16 ms for a one-pair product and
30 ms for four pairs, the Python scalar multiplication about 1 ms per 64-bit scalar, so the ~150 products below cost a few seconds."""
import numpy as np
import pytest
from oracle.py import ecc
from oracle import cpu_oracle as co
from tests import pairing761_cases as pc

SEED = 0x761C0DE


@pytest.fixture(scope="module")
def pts():
    return pc.python_points(140, SEED)


def test_points_are_the_generator_multiples(pts):
    A, B = pc.generators()
    assert ecc.E1_761.in_subgroup(A) and ecc.E2_761.in_subgroup(B)
    for i in (0, 1, 57, 139):
        k = pc.scalar(SEED, i)
        assert k & 1 and k < 1 << 64
        assert np.array_equal(pts.P[i], co.pack_761([ecc.E1_761.mul(A, k)])[0][0])
        assert np.array_equal(pts.Q[i], co.pack_761([ecc.E2_761.mul(B, k)])[0][0])
    g1, g2 = pc.python_rows(SEED, [57, 3])
    assert np.array_equal(g1, pts.P[[57, 3]]) and np.array_equal(g2, pts.Q[[57, 3]])
    assert len({pc.scalar(SEED, i) for i in range(140)}) == 140             # distinct scalars: a mismatched couple is never 1


@pytest.mark.parametrize("variant", pc.VARIANTS)
def test_every_product_class_has_its_constructed_verdict(pts, variant):
    """every variant at every pair count 0 ... 9 (the flagged / foreign pair moved through the positions by the base index)"""
    specs = [pc.product(pts, c, variant, 11 * c + 3 * r) for c in range(pc.MAX_PAIRS + 1) for r in range(2)]
    batch = pc.layout(pts, specs)
    g1, i1, g2, i2, offs, expect = batch
    assert offs[0] == 0 and offs[-1] == g1.shape[0] == g2.shape[0] == i1.size == i2.size
    for p, s in enumerate(specs):
        assert int(offs[p + 1] - offs[p]) == len(s) == p // 2
        gt, one = pc.oracle_gt(batch, p)
        assert bool(one) == bool(expect[p]) == bool(s.expect), (variant, s.kind, p)
    kinds = {s.kind for s in specs}
    assert "empty" in kinds and (variant in kinds)


def test_flags_decide_and_flagged_rows_are_never_read(pts):
    """the same products with the flags cleared change verdict where a flag switched a live pair off (so the flags are what decides), and
    the oracle's value does not depend on what a flagged row holds"""
    s = pc.product(pts, 3, "accept", 4)                # a couple and a flagged unrelated pair (its rows kept): 1; with the pair live: not 1
    b = pc.layout(pts, [s])
    assert pc.oracle_gt(b, 0)[1] and int(b[1].sum() + b[3].sum()) == 1 and b[0].any(axis=1).all() and b[2].any(axis=1).all()
    assert not co.pairing_product_761(b[0], None, b[2], None)[1]
    for pos in range(3):
        sp = pc.product(pts, 3, "accept", 8, flag_pos=pos)
        assert (np.array(sp.f1) | np.array(sp.f2)).tolist() == [int(t == pos) for t in range(3)]
        assert pc.oracle_gt(pc.layout(pts, [sp]), 0)[1]
    h = pc.product(pts, 2, "half_off", 16)
    bh = pc.layout(pts, [h])
    assert not pc.oracle_gt(bh, 0)[1]
    assert co.pairing_product_761(bh[0], None, bh[2], None)[1]              # the couple itself, flags ignored: 1
    # both flag arrays occur, and both zero rows and stale valid rows stand behind flagged points
    specs = [pc.product(pts, 3, "accept", base) for base in range(0, 16)]
    bb = pc.layout(pts, specs)
    assert bb[1].any() and bb[3].any()
    flagged1 = bb[0][bb[1] == 1]
    assert any(not r.any() for r in flagged1) and any(r.any() for r in flagged1)


def test_ragged_batch_layout_and_verdicts(pts):
    counts = [0, 3, 0, 9, 1, 2, 4, 0, 5, 8, 7, 6, 0]                  # empty products at the start, in the middle, at the end
    batch = pc.ragged_batch(pts, counts, seed=5, first=4)
    g1, i1, g2, i2, offs, expect = batch
    assert np.diff(offs.astype(np.int64)).tolist() == counts and offs[0] == 0 and g1.shape == (sum(counts), 24)
    for p in range(len(counts)):
        assert bool(pc.oracle_gt(batch, p)[1]) == bool(expect[p]), p
    assert 0 < int(expect.sum()) < len(counts)
    again = pc.ragged_batch(pts, counts, seed=5, first=4)
    assert all(np.array_equal(a, b) for a, b in zip(batch, again))


def test_groth16_shaped_accepts_and_rejects(pts):
    acc4 = pc.product(pts, 4, "accept", 20)
    rej4 = pc.product(pts, 4, "mismatch", 30)
    assert len({*acc4.i1} - {pts.NEG_A}) == 2                                # two couples with different i
    b = pc.layout(pts, [acc4, rej4])
    assert pc.oracle_gt(b, 0)[1] and not pc.oracle_gt(b, 1)[1]
    one = co.pairing_product_761(b[0][:0], None, b[2][:0], None)[0]
    assert np.array_equal(pc.oracle_gt(b, 0)[0], one)                       # the GT value of an accepting product IS the packed one


def test_reference_vector_and_its_tampered_forms(pts, golden):
    ref = pc.reference_products(golden)
    assert [r[3] for r in ref] == ["reference", "reference_bad_input", "reference_bad_c"]
    pts, at = pts.with_rows(np.concatenate([r[0] for r in ref]), np.concatenate([r[1] for r in ref]))       # a copy: the fixture stays as it is
    specs = [pc.fixed_product((at[0] + 4 * t, at[1] + 4 * t), 4, want, name) for t, (_, _, want, name) in enumerate(ref)]
    b = pc.layout(pts, [pc.product(pts, 2, "accept", 0)] + specs)
    assert b[5].tolist() == [1, 1, 0, 0]
    for p in range(4):
        assert bool(pc.oracle_gt(b, p)[1]) == bool(b[5][p]), p


def test_miller_wrapper_is_anchored_by_the_textbook_final_exponentiation(pts):
    """co.miller_loop_761 is what the GPU tests and the host twins compare Miller values with, bit for bit.  Its anchor outside the C oracle's
    own final exponentiation: raised to (q^3 - 1)(q + 1)(R0(x) + q R1(x)) by the Python flat-field square-and-multiply (ark-ec's BW6 exponent,
    as in tests/test_oracle_golden.py) it is the GT value co.pairing_product_761 returns - on single pairs of distinct points, on a product of
    three unrelated pairs, on an accepting couple (the power is one) and with a flagged pair."""
    from oracle.py import pairing as pp
    F, x, q = pp.F6_761, ecc.X, ecc.Q761
    R0 = -103 * x**7 + 70 * x**6 + 269 * x**5 - 197 * x**4 - 314 * x**3 - 73 * x**2 - 263 * x - 220
    R1 = 103 * x**9 - 276 * x**8 + 77 * x**7 + 492 * x**6 - 445 * x**5 - 65 * x**4 + 452 * x**3 - 181 * x**2 + 34 * x + 229
    e = (q**3 - 1) * (q + 1) * (R0 + q * R1)
    assert e > 0
    specs = [pc.product(pts, 1, "unrelated", 3), pc.product(pts, 1, "unrelated", 50), pc.product(pts, 3, "unrelated", 60),
             pc.product(pts, 2, "accept", 70), pc.product(pts, 3, "accept", 80, flag_pos=1, which=2, keep_rows=True)]
    b = pc.layout(pts, specs)
    seen = set()
    for p, s in enumerate(specs):
        ml = pc.oracle_miller(b, p)
        gt, one = pc.oracle_gt(b, p)
        assert F.pow(co.gt761_to_flat(ml), e) == co.gt761_to_flat(gt), p
        assert bool(one) == bool(s.expect) == (co.gt761_to_flat(gt) == F.one())
        seen.add(ml.tobytes())
    assert len(seen) == len(specs)
