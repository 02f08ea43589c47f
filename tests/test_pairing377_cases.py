"""CPU (-m "not gpu"): the inputs of the BLS12-377 pairing tests (tests/pairing377_cases.py) are what they claim to be, checked WITHOUT
the code under test: on small batches built the Python way the oracle (oracle/cpu: the arkworks restatement) returns exactly the verdict
each product was constructed to have, for every product class - the three kinds the BLS12-377 paths add included (first-pair flag, the
couple family over another shared point with its mismatch, the swapped product).  Measured: the C oracle takes about 13 ms for a four-pair
product, the Python scalar multiplication about 1 ms per 64-bit scalar.

The anchor of co.miller_loop_377 outside the C oracle's own final exponentiation is here too (oracle/py has a flat BLS12-377 Fq12), and so
are the sample conditions of the large GPU calls, asserted on the very seeded batches tests/test_pairing377_paths_gpu.py uses."""
import numpy as np
import pytest
from oracle.py import ecc
from oracle import cpu_oracle as co
from tests import pairing377_cases as pc

SEED = 0x377C0DE


@pytest.fixture(scope="module")
def pts():
    return pc.python_points(140, SEED)


@pytest.fixture(scope="module")
def one_gt():
    z1, z2 = np.zeros((0, 12), dtype=np.uint64), np.zeros((0, 24), dtype=np.uint64)
    gt, one = co.pairing_product_377(z1, None, z2, None)
    assert one
    return gt


def test_points_are_the_generator_multiples(pts):
    A, B = pc.CURVE.generators()
    assert (A, B) == (ecc.G1_377, ecc.G2_377) and ecc.E1_377.in_subgroup(A) and ecc.E2_377.in_subgroup(B)
    assert pts.P.shape == (140, 12) and pts.Q.shape == (140, 24)
    for i in (0, 1, 57, 139):
        k = pc.scalar(SEED, i)
        assert k & 1 and k < 1 << 64
        assert np.array_equal(pts.P[i], co.pack_g1_377([ecc.E1_377.mul(A, k)])[0][0])
        assert np.array_equal(pts.Q[i], co.pack_g2_377([ecc.E2_377.mul(B, k)])[0][0])
    g1, g2 = pc.python_rows(SEED, [57, 3])
    assert np.array_equal(g1, pts.P[[57, 3]]) and np.array_equal(g2, pts.Q[[57, 3]])
    assert len({pc.scalar(SEED, i) for i in range(140)}) == 140             # distinct scalars: a mismatched couple is never 1
    # the fixed rows, and the negated row a second couple family needs
    assert np.array_equal(pts.table1[pts.NEG_A], co.pack_g1_377([ecc.E1_377.neg(A)])[0][0]) and not pts.table1[pts.ZERO1].any()
    assert np.array_equal(pts.table2[pts.B], co.pack_g2_377([B])[0][0]) and not pts.table2[pts.ZERO2].any()
    q, fam = pc.family_over(pts, 57)
    assert np.array_equal(q.table1[fam.neg], co.pack_g1_377([ecc.E1_377.neg(ecc.E1_377.mul(A, pc.scalar(SEED, 57)))])[0][0])
    assert fam.shared == 57 and q.table1.shape[0] == pts.table1.shape[0] + 1 and q.table2.shape == pts.table2.shape
    assert the_library_generators_are_the_oracles()


def the_library_generators_are_the_oracles():
    """device_points multiplies the library's own constants: they are the oracle's generators"""
    from celo_bls_snark_rs_amd import synthetic as syn, bls
    return tuple(syn.G1_GENERATOR) == tuple(ecc.G1_377) and tuple(map(tuple, bls.G2_GENERATOR)) == tuple(map(tuple, ecc.G2_377))


@pytest.mark.parametrize("family", ["B", "Q_J"])
@pytest.mark.parametrize("variant", pc.VARIANTS)
def test_every_product_class_has_its_constructed_verdict(pts, one_gt, variant, family):
    """every variant at every pair count 0 ... 9 (the flagged / foreign pair moved through the positions by the base index), over the
    couple family (B, -A) and over (Q_J, -P_J)"""
    fam = None
    if family == "Q_J":
        pts, fam = pc.family_over(pts, 131)
    specs = [pc.product(pts, c, variant, 11 * c + 3 * r, family=fam) for c in range(pc.MAX_PAIRS + 1) for r in range(2)]
    batch = pc.layout(pts, specs)
    g1, i1, g2, i2, offs, expect = batch
    assert offs[0] == 0 and offs[-1] == g1.shape[0] == g2.shape[0] == i1.size == i2.size and g1.shape[1] == 12 and g2.shape[1] == 24
    for p, s in enumerate(specs):
        assert int(offs[p + 1] - offs[p]) == len(s) == p // 2
        gt, one = pc.oracle_gt(batch, p)
        assert bool(one) == bool(expect[p]) == bool(s.expect) == np.array_equal(gt, one_gt), (variant, s.kind, p)
        if fam is not None:
            assert pts.B not in s.i2 and pts.NEG_A not in s.i1
    kinds = {s.kind for s in specs}
    assert "empty" in kinds and (variant in kinds)
    if variant == "first_off":
        for s in specs:
            if s.kind == "first_off":
                assert (s.f1[0] | s.f2[0]) == 1 and s.i2[0] == (pts.B if fam is None else fam.shared) and s.expect == 0


def test_verify_shaped_products_and_the_swapped_one(pts, one_gt):
    """every kind of verify-shaped product, through inf1 and inf2, zero rows and stale rows, over both families: the constructed verdict,
    the first G2 row shared; the swapped product has the same verdict and the same GT value but another first row"""
    q, famj = pc.family_over(pts, 99)
    for fam in (None, famj):
        specs, base = [], 0
        for which in (1, 2):
            for keep in (True, False):
                for kind in pc.VERIFY_KINDS:
                    specs.append(pc.verify_product(q, 2, kind, base, base + 1, which, keep, fam)); base += 2
                for kind in ("live", "off"):
                    specs.append(pc.verify_product(q, 1, kind, base, None, which, keep, fam)); base += 1
                specs.append(pc.verify_product(q, 0, "empty", base))
        assert pc.first_rows_shared(q, specs, fam)
        batch = pc.layout(q, specs)
        assert batch[1].any() and batch[3].any()
        for p, s in enumerate(specs):
            gt, one = pc.oracle_gt(batch, p)
            assert bool(one) == bool(s.expect) == np.array_equal(gt, one_gt), (p, s.kind)
            assert s.expect == (1 if s.kind in ("accept", "both_off", "off", "empty") else 0)
            if len(s) == 2:
                t = pc.swapped(s)
                assert not pc.first_rows_shared(q, [t], fam) and t.expect == s.expect and t.i2 == s.i2[::-1] and t.f1 == s.f1[::-1]
                gs, ones = pc.oracle_gt(pc.layout(q, [t]), 0)
                assert np.array_equal(gs, gt) and bool(ones) == bool(one), (p, s.kind)
        # a first-pair flag leaves the shared row in place whichever array carries it
        firsts = [s for s in specs if s.kind == "first_off"]
        assert len(firsts) == 4 and {(s.f1[0], s.f2[0]) for s in firsts} == {(1, 0), (0, 1)}
    # the two families give calls of identical shape that differ in the shared row only by what the rows hold
    a = pc.layout(q, pc.split_specs(q, 20, seed=3, first=10))
    b = pc.layout(q, pc.split_specs(q, 20, seed=3, first=10, family=famj))
    assert np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
    assert not np.array_equal(a[2][0], b[2][0]) and 0 < int(a[5].sum()) < 20
    for p in range(20):
        assert bool(pc.oracle_gt(a, p)[1]) == bool(a[5][p]) and bool(pc.oracle_gt(b, p)[1]) == bool(b[5][p]), p


def test_verify_shaped_specs_keep_the_first_row_invariant(pts):
    counts = [2, 0, 1, 2, 2, 0, 2, 1, 1, 2, 2, 2, 0, 2, 1, 2, 2, 2, 2, 0]
    specs = pc.verify_shaped_specs(pts, counts, seed=9, first=20)
    assert [len(s) for s in specs] == counts and pc.first_rows_shared(pts, specs)
    batch = pc.layout(pts, specs)
    shared = pts.table2[pts.B]
    for p, c in enumerate(counts):
        if c:
            assert np.array_equal(batch[2][int(batch[4][p])], shared), p
        assert bool(pc.oracle_gt(batch, p)[1]) == bool(batch[5][p]), (p, specs[p].kind)
    assert not pc.first_rows_shared(pts, specs[:3] + [pc.swapped(specs[3])] + specs[4:])
    again = pc.layout(pts, pc.verify_shaped_specs(pts, counts, seed=9, first=20))
    assert all(np.array_equal(x, y) for x, y in zip(batch, again))


def test_flags_decide_and_flagged_rows_are_never_read(pts):
    """the same products with the flags cleared change verdict where a flag switched a live pair off (so the flags are what decides), and
    the oracle's value does not depend on what a flagged row holds"""
    s = pc.product(pts, 3, "accept", 4)                # a couple and a flagged unrelated pair (its rows kept): 1; with the pair live: not 1
    b = pc.layout(pts, [s])
    assert pc.oracle_gt(b, 0)[1] and int(b[1].sum() + b[3].sum()) == 1 and b[0].any(axis=1).all() and b[2].any(axis=1).all()
    assert not co.pairing_product_377(b[0], None, b[2], None)[1]
    for pos in range(3):
        sp = pc.product(pts, 3, "accept", 8, flag_pos=pos)
        assert (np.array(sp.f1) | np.array(sp.f2)).tolist() == [int(t == pos) for t in range(3)]
        assert pc.oracle_gt(pc.layout(pts, [sp]), 0)[1]
    for variant in ("half_off", "first_off"):
        h = pc.product(pts, 2, variant, 16, keep_rows=True)
        bh = pc.layout(pts, [h])
        assert not pc.oracle_gt(bh, 0)[1]
        assert co.pairing_product_377(bh[0], None, bh[2], None)[1]              # the couple itself, flags ignored: 1
    # a stale row behind a flag and a zero row give the same value
    for which in (1, 2):
        kept = pc.layout(pts, [pc.verify_product(pts, 2, "second_off", 30, which=which, keep_rows=True)])
        zero = pc.layout(pts, [pc.verify_product(pts, 2, "second_off", 30, which=which, keep_rows=False)])
        assert not np.array_equal(kept[0] if which == 1 else kept[2], zero[0] if which == 1 else zero[2])
        assert np.array_equal(pc.oracle_gt(kept, 0)[0], pc.oracle_gt(zero, 0)[0])
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
    assert np.diff(offs.astype(np.int64)).tolist() == counts and offs[0] == 0 and g1.shape == (sum(counts), 12) and g2.shape == (sum(counts), 24)
    for p in range(len(counts)):
        assert bool(pc.oracle_gt(batch, p)[1]) == bool(expect[p]), p
    assert 0 < int(expect.sum()) < len(counts)
    again = pc.ragged_batch(pts, counts, seed=5, first=4)
    assert all(np.array_equal(a, b) for a, b in zip(batch, again))


def test_accepting_gt_is_the_packed_one(pts, one_gt):
    acc4 = pc.product(pts, 4, "accept", 20)
    rej4 = pc.product(pts, 4, "mismatch", 30)
    assert len({*acc4.i1} - {pts.NEG_A}) == 2                                # two couples with different i
    b = pc.layout(pts, [acc4, rej4])
    assert pc.oracle_gt(b, 0)[1] and not pc.oracle_gt(b, 1)[1]
    assert np.array_equal(pc.oracle_gt(b, 0)[0], one_gt)                    # the GT value of an accepting product IS the packed one
    assert co.from_mont(one_gt.reshape(12, 6), ecc.Q377) == [1] + [0] * 11


def test_miller_wrapper_is_anchored_by_the_textbook_final_exponentiation(pts):
    """co.miller_loop_377 is what the GPU tests compare Miller values with, bit for bit.  Its anchor outside the C oracle's own final
    exponentiation: raised to 3 (q^12 - 1) / r by the Python flat-field square-and-multiply (oracle/py/pairing.py F12_377 = Fq[w] / (w^12 + 5);
    the factor 3 is ark-ec's BLS12 hard part, the convention tests/test_oracle_golden.py pins against the textbook pairing) it is the GT
    value co.pairing_product_377 returns - on a single pair, on three unrelated pairs, on an accepting couple (the power is one) and
    with a flagged first pair.  (The Miller values themselves differ from the textbook loop's by Fq2 factors of the projective lines, which
    the exponentiation kills: that is why the comparison is made after it.)"""
    from oracle.py import pairing as pp
    F = pp.F12_377
    e = 3 * ((ecc.Q377**12 - 1) // ecc.R377)
    assert (ecc.Q377**12 - 1) % ecc.R377 == 0
    specs = [pc.product(pts, 1, "unrelated", 3), pc.product(pts, 3, "unrelated", 60), pc.product(pts, 2, "accept", 70),
             pc.product(pts, 2, "first_off", 80, which=2)]
    b = pc.layout(pts, specs)
    seen = set()
    for p, s in enumerate(specs):
        ml = pc.oracle_miller(b, p)
        gt, one = pc.oracle_gt(b, p)
        assert F.pow(co.gt377_to_flat(ml), e) == co.gt377_to_flat(gt), p
        assert bool(one) == bool(s.expect) == (co.gt377_to_flat(gt) == F.one())
        seen.add(ml.tobytes())
    assert len(seen) == len(specs)


class _Indices(pc.Points):
    """points whose rows hold their own index: the sample conditions depend on the specs alone (pair counts, classes, flags)"""

    def __init__(self, n):
        self.curve, self.n, self.seed = pc.CURVE, n, 0
        self.A, self.NEG_A, self.ZERO1, self.B, self.ZERO2 = n, n + 1, n + 2, n, n + 1
        self.table1 = np.arange(n + 3, dtype=np.uint64)[:, None]
        self.table2 = np.arange(n + 2, dtype=np.uint64)[:, None]


def test_sample_conditions_on_the_seeded_batches_of_the_gpu_tests():
    """section "how much of a large call may go unchecked": at most 400 products per large call, 64 seeded ones, the first and the last,
    9 / 10 / 11, both sides of every threshold, the last block, one per (pair count, class), every flagged product, filled to the cap"""
    idx = _Indices(pc.N_BIG)
    specs = pc.threshold_specs(idx)
    flagged = [s for s in specs if pc.has_flag(s)]
    kinds = {(len(s), s.kind) for s in specs}
    print("ragged 16421: %d flagged in %d (count, class) combinations, %d accepting, %d classes" % (
        len(flagged), len({(len(s), s.kind) for s in flagged}), sum(s.expect for s in specs), len(kinds)))
    assert {c for c, _ in kinds} == {0, 1, 2, 3, 4} and {k for _, k in kinds} >= set(pc.VARIANTS) | {"empty"} and max(len(s) for s in specs) == 4
    assert 150 < len(flagged) < 300 and any(any(s.f1) for s in flagged) and any(any(s.f2) for s in flagged)
    assert 3000 < sum(s.expect for s in specs) < 12000
    for m in (pc.SHARED_MIN, pc.M_BIG):
        pick = pc.sample(specs[:m], 16386, thresholds=(pc.SHARED_MIN,))
        assert len(pick) == pc.SAMPLE_CAP
        pc.check_sample(specs[:m], pick, 16386, thresholds=(pc.SHARED_MIN,))
    vs = pc.verify_threshold_specs(idx)
    counts = [len(s) for s in vs]
    assert set(counts) == {0, 1, 2} and counts[0] == 2 and counts[1] == 0 and {s.kind for s in vs} == set(pc.VERIFY_KINDS) | {"live", "off", "empty"}
    vf = [s for s in vs if pc.has_flag(s)]
    assert any(s.f1[0] for s in vf) and any(s.f2[0] for s in vf) and any(len(s) == 2 and s.f1[1] for s in vf) and any(len(s) == 2 and s.f2[1] for s in vf)
    pick = pc.sample(vs, 16392, thresholds=(pc.SHARED_MIN,))
    assert len(pick) == pc.SAMPLE_CAP
    pc.check_sample(vs, pick, 16392, thresholds=(pc.SHARED_MIN,))
    fe = pc.final_exp_specs(idx)
    assert len(fe) == 5121 and max(len(s) for s in fe) == 4 and any(len(s) == 4 for s in fe[:769]) and any(len(s) != 2 for s in fe[:769])
    pick = pc.sample(fe, 5123, thresholds=(768, 3072, 5120))
    pc.check_sample(fe, pick, 5123, thresholds=(768, 3072, 5120))
    ws = pc.wide_specs(idx, pc.WIDE_MAX)
    assert max(len(s) for s in ws) == 3 and len(ws[0]) == len(ws[384]) == len(ws[767]) == 0 and any(any(s.f1) for s in ws) and any(any(s.f2) for s in ws)
    pick = pc.sample(ws, 320 + pc.WIDE_MAX, thresholds=(pc.WIDE_MAX,))
    assert 300 < len(pick) <= pc.SAMPLE_CAP              # (every flagless accepting product of two or three pairs is in: there are no more)
    pc.check_sample(ws, pick, 320 + pc.WIDE_MAX, thresholds=(pc.WIDE_MAX,))
    sp_all = pc.split_threshold_specs(idx)
    for m in (769, 3072, 3073, 5120, 5121):
        sp = sp_all[:m]
        assert all(len(s) == 2 for s in sp) and {s.kind for s in sp} == set(pc.VERIFY_KINDS)
        assert {(s.kind, s.f1[0], s.f2[0], s.f1[1], s.f2[1]) for s in sp if pc.has_flag(s)} >= {
            ("first_off", 1, 0, 0, 0), ("first_off", 0, 1, 0, 0), ("second_off", 0, 0, 1, 0), ("second_off", 0, 0, 0, 1)}
        pick = pc.sample(sp, 7100 + m, thresholds=(768, 3072, 5120))
        pc.check_sample(sp, pick, 7100 + m, thresholds=(768, 3072, 5120))
