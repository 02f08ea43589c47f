"""CPU (-m "not gpu"): the inputs of the batched small-MSM tests (tests/batch_cases.py) are what they claim to be, checked WITHOUT the code
under test.  Every Horner branch builder's expected point equals the big-integer definition (ecc.*.msm); the signed digits of its scalars,
recoded by the plain definition, put its points into the buckets and its window sums into the Horner chain in the way that reaches the
branch it names (bucket_trace: 'double', 'cancel', a chain that goes on from the identity, window sums empty by cancellation, a chain that
ends at the identity with every window live); expected_dispatch is pinned on rows worked out by hand from DESIGN.md section 6."""
import numpy as np
import pytest
from oracle.py import ecc
from oracle import cpu_oracle as co
from tests import batch_cases as bc

G1, G2, W1, W2 = "bls12_377_g1", "bls12_377_g2", "bw6_761_g1", "bw6_761_g2"
# every window on the 8-word group; the ends of the range on the two wide ones (their Python arithmetic is the slow part)
BUILDER_CASES = [(G1, c) for c in (3, 4, 5, 6, 7)] + [(g, c) for g in (G2, W1) for c in (3, 5)] + [(W2, 3)]


@pytest.fixture(scope="module")
def some_points():
    return {g: bc.GROUPS[g].multiples([3, 0x1234567, 0xDEADBEEFCAFE]) for g in bc.GROUPS}


def test_group_table(some_points):
    from celo_bls_snark_rs_amd import synthetic as syn, ffi
    assert bc.GROUPS[W1].generator() == syn.BW6_G1_POINT and bc.GROUPS[W2].generator() == syn.BW6_G2_POINT    # what device_points multiplies
    assert bc.GROUPS[G1].generator() == syn.G1_GENERATOR and bc.GROUPS[G1].generator() == ecc.G1_377 and bc.GROUPS[G2].generator() == ecc.G2_377
    for name, g in bc.GROUPS.items():
        A, S, O = ffi.GROUP_SHAPE[name]
        assert (g.rows, g.limbs, g.words) == (A, S, 2 * S) and g.coords * g.coord_limbs == g.rows
        assert g.scalar_bits == g.order.bit_length() and g.scalar_bits <= 32 * g.words
        assert g.curve.in_subgroup(g.generator())
        P, Q, _ = some_points[name]
        rows, inf = g.pack([P, None, Q])
        assert rows.shape == (3, g.rows) and inf.tolist() == [0, 1, 0]
        neg = g.neg_rows(rows)
        assert np.array_equal(neg, g.pack([g.curve.neg(P), None, g.curve.neg(Q)])[0])
        assert co.jac_to_affine(np.concatenate([rows[0], co.to_mont([1] + [0] * (g.coords // 2 - 1), g.q).reshape(-1)]), g.kind) == P
    assert [e for e in bc.ENTRIES if e[1]] == [(G2, True)] and {e[0] for e in bc.ENTRIES} == set(bc.GROUPS)


def kernel_digits(k, c, nw):
    """k_batch_sort's formulation, restated: raw window bits plus the carry; a digit above 2^(c-1) is taken negative and carries"""
    B, carry, out = 1 << (c - 1), 0, []
    for w in range(nw):
        d = ((k >> (w * c)) & ((1 << c) - 1)) + carry
        neg = d > B
        out.append(-((1 << c) - d) if neg else d)
        carry = 1 if neg else 0
    return out, carry


@pytest.mark.parametrize("c", [3, 4, 5, 6, 7])
def test_recode_is_the_signed_digit_definition(c):
    rng = ecc.SplitMix64(0xD161 + c)
    ks = [0, 1, (1 << c) - 1, 1 << (c - 1), (1 << (c - 1)) + 1, (1 << 252) - 1, (1 << 376) - 1, ecc.R377 - 1, ecc.R761 - 1]
    ks += [ecc.random_scalar(rng, 1 << b) for b in (20, 64, 136, 252, 376) for _ in range(8)]
    for k in ks:
        bits = max(1, k.bit_length())
        nw = (bits + c) // c
        d = bc.recode(k, c, nw)
        assert len(d) == nw and all(-(1 << (c - 1)) < x <= 1 << (c - 1) for x in d)
        assert sum(x << (c * w) for w, x in enumerate(d)) == k
        assert (d, 0) == kernel_digits(k, c, nw)
        assert bc.recode(k, c, nw + 2) == d + [0, 0]
    with pytest.raises(AssertionError):
        bc.recode((1 << (2 * c)) - 1, c, 2)        # a scalar of 2c bits needs three windows: the top digit carries


@pytest.mark.parametrize("group,c", BUILDER_CASES)
def test_builders_reach_the_branch_they_name(some_points, group, c):
    g = bc.GROUPS[group]
    E = g.curve
    P, R, _ = some_points[group]
    k = bc.full_scalar(group, 0xA11C + c)
    assert k.bit_length() == g.scalar_bits - 1 and k < g.order
    half = 1 << (c - 1)

    def trace(points, scalars, expect):
        bits = max(s.bit_length() for s in scalars)
        got = bc.expected_dispatch(group, [len(points)], bits)
        assert got[0] == 3 and got[3] == 1                                  # alone, the instance gets the smallest window ...
        nw = (bits + c) // c                                                # ... the builder's c is the window of the call it is put into
        for s in scalars:
            assert all(-half < d <= half for d in bc.recode(s, c, nw))
        assert E.msm(points, scalars) == expect and all(E.on_curve(Q) for Q in points)
        t = bc.bucket_trace(group, points, scalars, c, nw)
        assert t["result"] == expect
        return t, nw

    pts, sc, exp = bc.build("doubling", group, c, P, R, k)
    assert exp == E.mul(P, 2 << c) and exp is not None
    t, nw = trace(pts, sc, exp)
    assert nw == 2 and bc.recode(sc[0], c, 2) == [0, 1] and bc.recode(sc[1], c, 2) == [1, 0]
    assert t["events"] == [(1, "load"), (0, "double")] and t["wsum"] == [pts[1], P]

    pts, sc, exp = bc.build("cancel_and_go_on", group, c, P, R, k)
    assert exp == R and R is not None
    t, nw = trace(pts, sc, exp)
    assert nw == 3 and [bc.recode(s, c, 3) for s in sc] == [[0, 0, 1], [0, 1, 0], [1, 0, 0]]
    assert t["events"] == [(2, "load"), (1, "cancel"), (0, "load")]          # the chain reaches the identity at window 1 and loads R after it

    pts, sc, exp = bc.build("all_cancel", group, c, P, R, k)
    assert exp is None and pts[1] == E.neg(P) and sc[0] == sc[1] == k
    t, nw = trace(pts, sc, exp)
    digits = bc.recode(k, c, nw)
    live = [w for w in range(nw) if digits[w]]
    assert len(live) > nw // 2 and nw == (g.scalar_bits - 1 + c) // c
    for w in live:                                                           # every bucket in use holds the pair and nothing else
        assert list(t["buckets"][w]) == [abs(digits[w])] and sorted(t["buckets"][w][abs(digits[w])]) == sorted([P, E.neg(P)])
    assert t["wsum"] == [None] * nw and t["events"] == []

    pts, sc, exp = bc.build("live_identity", group, c, P, R, k)
    assert exp is None and pts == [P, P] and sc[0] + sc[1] == g.order and 0 < sc[0] < g.order
    t, nw = trace(pts, sc, exp)
    L = bc.live_identity_scalars(g.order, c)[2]
    assert nw - 1 <= L <= nw and all(W is not None for W in t["wsum"][:L])   # every window up to the top digit of r is live
    assert t["events"][0] == (L - 1, "load") and t["events"][-1] == (0, "cancel") and all(e[1] in ("add", "double") for e in t["events"][1:-1])
    assert len(t["events"]) == L


@pytest.mark.parametrize("group", [G1, G2])
def test_short_identity_instance(some_points, group):
    g = bc.GROUPS[group]
    P = some_points[group][0]
    a, b = bc.scalar_of_bits(135, 1), bc.scalar_of_bits(135, 2)
    pts, sc, exp = bc.live_identity_short(group, P, a, b)
    assert exp is None and max(s.bit_length() for s in sc) == 136 and g.curve.msm(pts, sc) is None
    t = bc.bucket_trace(group, pts, sc, 3, (136 + 3) // 3)
    assert t["result"] is None and sum(W is not None for W in t["wsum"]) >= 10      # (a window is empty wherever a_w + b_w needs no carry)
    # the base-x digits of a + b are not the digit-wise sums (carries): the images psi^j do not cancel image by image
    x = ecc.X
    dig = lambda k: [k % x, k // x % x, k // x // x]
    assert [u + v for u, v in zip(dig(a), dig(b))] != dig(a + b)


def test_expected_dispatch_rows_worked_out_by_hand():
    ed = bc.expected_dispatch
    # the window: 3 below 128 points, one more at 128, 256, 512 and 1024
    assert [bc.window_for(n) for n in (0, 1, 127, 128, 255, 256, 257, 511, 512, 513, 1023, 1024)] == [3, 3, 3, 4, 4, 5, 5, 5, 6, 6, 6, 7]
    assert [bc.window_for(300, f) for f in (1, 3, 4, 7, 9)] == [3, 3, 4, 7, 7]
    assert ed(G1, [1, 17, 256, 0, 300, 64], 136) == (5, 28, 6 * 28 * 16, 1)
    assert ed(G1, [127], 252) == (3, 85, 340, 1) and ed(G1, [128], 252) == (4, 64, 512, 1)
    assert ed(G1, [256], 252) == (5, 51, 51 * 16, 1) and ed(G1, [512], 252) == (6, 43, 43 * 32, 1)
    assert ed(G1, [1, 1024, 0, 1023, 7], 252) == (7, 37, 5 * 37 * 64, 1)
    assert ed(G1, [9], 0) == (3, 1, 4, 1) and ed(G1, [9], 1) == (3, 1, 4, 1) and ed(G1, [9], 3) == (3, 2, 8, 1)
    # bits from SCALAR_BITS up do not count
    assert ed(G1, [1024], 256) == ed(G1, [1024], 253) == (7, 37, 37 * 64, 1)
    assert ed(W1, [40], 384) == ed(W1, [40], 377) == (3, 126, 126 * 4, 1) and ed(W2, [1024], 376) == (7, 54, 54 * 64, 1)
    # forced windows
    assert ed(G1, [40], 252, forced_c=7) == (7, 37, 37 * 64, 1) and ed(W1, [600], 376, forced_c=3) == (3, 126, 126 * 4, 1)
    # the split: only on the subgroup entry of G2, by bit class, and only while the expanded instance fits 1024 points
    assert ed(G2, [300], 136) == (5, 28, 28 * 16, 1) and ed(G1, [300], 136, subgroup=True) == (5, 28, 28 * 16, 1)
    assert ed(G2, [300], 64, subgroup=True) == (5, 13, 13 * 16, 1) and ed(G2, [300], 65, subgroup=True) == (6, 11, 11 * 32, 2)
    assert ed(G2, [256] * 4096, 136, subgroup=True) == (6, 11, 4096 * 11 * 32, 3)       # config 3: 768 points, 11 windows of 6 bits
    assert ed(G2, [341], 136, subgroup=True) == (6, 11, 11 * 32, 3) and ed(G2, [342], 136, subgroup=True) == (5, 28, 28 * 16, 1)
    assert ed(G2, [256], 252, subgroup=True) == (7, 10, 10 * 64, 4) and ed(G2, [257], 252, subgroup=True) == (5, 51, 51 * 16, 1)
    assert ed(G2, [512], 100, subgroup=True) == (7, 10, 10 * 64, 2) and ed(G2, [513], 100, subgroup=True) == (6, 17, 17 * 32, 1)
    assert ed(G2, [100], 126, subgroup=True)[3] == 2 and ed(G2, [100], 127, subgroup=True)[3] == 3
    assert ed(G2, [100], 189, subgroup=True)[3] == 3 and ed(G2, [100], 190, subgroup=True)[3] == 4
    assert ed(G2, [40], 255, subgroup=True) == ed(G2, [40], 253, subgroup=True) == (4, 17, 17 * 8, 4)
    # the large pipeline, instance by instance
    assert ed(G1, [1025, 0, 3], 252) == "side" and ed(W1, [0, 0, 0], 0) == "side" and ed(G1, [], 0) == "side"


def test_calls_in_row_form(some_points):
    for group in (G1, W2):
        g = bc.GROUPS[group]
        table = g.pack(g.multiples(range(5, 31)))[0]
        call = bc.mixed_call(group, table, [1, 12, 0, 9, 3], 97, 7)
        assert call.sizes == [1, 12, 0, 9, 3] and call.bits() == 97 and call.rows.shape == (25, g.rows) and call.scalars.shape == (25, g.limbs)
        ints = co.limbs_to_ints(call.scalars, g.limbs)
        assert ints[1 + 4] == (1 << 97) - 1 and max(ints) == ints[5]
        for lo in (1, 13):
            assert call.inf[lo:lo + 9].tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 0] and ints[lo] == 0 and ints[lo + 1] == 1
            assert np.array_equal(call.rows[lo + 5], call.rows[lo + 6]) and ints[lo + 5] == ints[lo + 6]
            assert np.array_equal(call.rows[lo + 7], g.neg_rows(call.rows[lo + 2])[0]) and ints[lo + 7] == ints[lo + 2] != 0
        assert not call.inf[[0, 22, 23, 24]].any() and np.array_equal(call.rows[22:], table[22:25])
        assert bc.mixed_call(group, table, [3, 2], 20, 1, top_at=4).scalars[4, 0] == (1 << 20) - 1
        # a filler that cancels bucket by bucket, and hand-built instances joined into a call
        rows, inf, sc = bc.cancelling_filler(group, table, 6, 136, 3)
        assert np.array_equal(rows[1::2], g.neg_rows(rows[0::2])) and np.array_equal(sc[0::2], sc[1::2]) and bc.longest(sc) <= 136 and not inf.any()
        inst = bc.pack_instance(group, [some_points[group][0], None], [5, 6])
        call = bc.concat_call(group, [inst, (rows, inf, sc), bc.pack_instance(group, [], [])])
        assert call.sizes == [2, 6, 0] and call.inf.tolist() == [0, 1] + [0] * 6 and call.scalars[:2, 0].tolist() == [5, 6]
        assert bc.concat_call(group, []).sizes == [] and bc.concat_call(group, []).rows.shape == (0, g.rows)
    sc = co.ints_to_limbs([(1 << 256) - 1, (1 << 255) | 5, 7], 4)
    assert co.limbs_to_ints(bc.clear_from(sc, 253), 4) == [(1 << 253) - 1, 5, 7] and bc.longest(sc) == 256 and bc.longest(sc[2:]) == 3
    assert co.limbs_to_ints(bc.clear_from(co.ints_to_limbs([(1 << 384) - 1], 6), 377), 6) == [(1 << 377) - 1]
    for bits in (1, 7, 8, 9, 63, 64, 65, 136, 252, 256):
        r = bc.random_scalars(200, 4, bits, bits)
        assert bits - 6 <= bc.longest(r) <= bits
