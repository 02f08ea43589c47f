"""Inputs for the BLS12-377 pairing tests, every product with a verdict known BY CONSTRUCTION (no GPU import at module level).  The
curve-independent machinery (Spec, product, layout, ragged_specs, ...) is tests/pairing761_cases.py's; this module binds it to BLS12-377
(rows of 12 / 24 words, pack_g1_377 / pack_g2_377, the oracle's pairing_product_377 / miller_loop_377) and adds what the BLS12-377 dispatch
paths need.

Points.  A = ecc.G1_377, B = ecc.G2_377 (the generators: r-torsion); k_i = splitmix64_at(seed, i) | 1, the scalar the library's point
generator uses; P_i = k_i A, Q_i = k_i B.  python_points (the Python oracle's scalar multiplication) and device_points (the generator
kernel, synthetic.device_points("bls12_377_g1" / "bls12_377_g2")) give the same rows for the same (seed, n).

Products.  With g = e(A, B), a generator of the order-r subgroup of GT (r is 253 bits), every product is g^E for a known exponent E:
  couple(i)            e(P_i, B) e(-A, Q_i)               E = k_i - k_i = 0                                   -> 1
  mismatch(i, j)       e(P_i, B) e(-A, Q_j), j != i       E = k_i - k_j, 0 < |E| < 2^64                       -> not 1
  unrelated            e(P_a, Q_b) ...  (c <= 64 pairs)   E = sum k_a k_b, 0 < E < 64 * 2^128 < 2^135         -> not 1
  half a couple        e(P_i, B) or e(-A, Q_i), the other pair switched off by a flag: E = k_i or -k_i        -> not 1
  couple over Q_J      e(P_i, Q_J) e(-P_J, Q_i)           E = k_i k_J - k_J k_i = 0                           -> 1
  its mismatch         e(P_i, Q_J) e(-P_J, Q_l), l != i   E = k_J (k_i - k_l), 0 < |E| < 2^128                -> not 1
  half of it           e(P_i, Q_J) or e(-P_J, Q_i)        E = k_i k_J or -k_J k_i, 0 < |E| < 2^128            -> not 1
All |E| are far below r ~ 2^253, a pair switched off by inf1 or inf2 contributes 1, and a product never mixes a mismatch with an
unrelated pair, so every verdict is exact, not "with high probability".

What the BLS12-377 paths add (csrc/pairing.h run_staged):
  verify order     the prepared-lines kernels evaluate every product's FIRST pair on the lines of one shared G2 row, so a two-pair product
                   is laid out [(P_i, S), (-N, Q_j)] un-rotated and a one-pair product is (P_i, S): verify_product / verify_shaped_specs
  first_off        the FIRST pair switched off (its G2 row stays the shared row: the dispatch compares rows, not flags): e(-N, Q_i) remains
  family           (S, N) = (B, -A) or (Q_J, -P_J): two calls of identical shape that differ in the shared row
  swapped          [(-N, Q_i), (P_i, S)]: the same value, but the first G2 row is not the shared one"""
import numpy as np
from oracle.py import ecc
from oracle import cpu_oracle as co
from tests import pairing761_cases as pc
from tests.pairing761_cases import (Spec, Points, scalar, resolve_variant, flag_defaults, fixed_product, layout, has_flag,  # noqa: F401
                                    slice_of, MAX_PAIRS)

CURVE = pc.Curve("bls12_377", 12, 24, ecc.Q377, ecc.E1_377, ecc.E2_377, lambda: (ecc.G1_377, ecc.G2_377), co.pack_g1_377, co.pack_g2_377,
                 ("bls12_377_g1", "bls12_377_g2"), lambda *a: co.pairing_product_377(*a), lambda *a: co.miller_loop_377(*a))
VARIANTS = pc.VARIANTS + ("first_off",)
VERIFY_KINDS = ("accept", "mismatch", "second_off", "first_off", "both_off")      # of a two-pair verify-shaped product


def python_rows(seed, indices):
    return CURVE.python_rows(seed, indices)


def python_points(n, seed):
    return CURVE.python_points(n, seed)


def device_points(n, seed):
    return CURVE.device_points(n, seed)


def oracle_gt(batch, p):
    return pc.oracle_gt(batch, p, CURVE)


def oracle_miller(batch, p):
    return pc.oracle_miller(batch, p, CURVE)


class Family:
    """the shared G2 row S (an index into table2) and the G1 row -N it is coupled with (an index into table1)"""

    def __init__(self, shared, neg, name):
        self.shared, self.neg, self.name = shared, neg, name


def family_b(pts):
    return Family(pts.B, pts.NEG_A, "B")


def family_over(pts, j):
    """-> (a copy of pts with the row -P_j appended to table1, the family (Q_j, -P_j))"""
    q, at = pts.with_rows(CURVE.neg_g1_rows(pts.P[j]), np.zeros((0, CURVE.w2), dtype=np.uint64))
    return q, Family(j, at[0], "Q_%d" % j)


def _into_family(pts, s, fam):
    if fam is not None and fam.shared != pts.B:
        s.i2 = [fam.shared if r == pts.B else r for r in s.i2]
        s.i1 = [fam.neg if r == pts.NEG_A else r for r in s.i1]
    return s


def product(pts, c, variant, base, flag_pos=None, which=None, keep_rows=None, family=None):
    """pc.product, plus the variant first_off (c >= 2: accepting couples whose very first pair is switched off, un-rotated; an odd pair out
    is flagged too) and the couples taken over `family` instead of (B, -A)"""
    if variant == "first_off" and c >= 2:
        d = flag_defaults(base, c)
        which = d["which"] if which is None else which
        keep = d["keep_rows"] if keep_rows is None else keep_rows
        s = pc.product(pts, c, "accept", base, flag_pos=c - 1 if c % 2 else 1, which=which, keep_rows=keep)       # rotation 0
        assert s.i2[0] == pts.B and not s.f1[0] and not s.f2[0]
        s.f1[0], s.f2[0] = (1, 0) if which == 1 else (0, 1)
        if which == 1 and not keep:
            s.i1[0] = pts.ZERO1              # (the G2 row of the first pair stays the shared row whatever the flag)
        s.kind, s.expect = "first_off", 0
    else:
        s = pc.product(pts, c, "all_off" if variant == "first_off" else variant, base, flag_pos, which, keep_rows)
    return _into_family(pts, s, family)


def verify_product(pts, c, kind, i, j=None, which=1, keep_rows=True, family=None):
    """a verify-shaped product of c in {0, 1, 2} pairs over the indices i (and j: the foreign Q of a mismatch), first pair (P_i, S):
      c = 2: accept, mismatch, second_off, first_off, both_off        c = 1: live (E = k_i: not 1), off (1)        c = 0: empty
    which: 1 / 2 = the flag(s) go through inf1 / inf2; keep_rows: a flagged point keeps a valid row (the shared row is always kept)."""
    fam = family_b(pts) if family is None else family
    s = Spec(kind if c else "empty")
    if c == 0:
        s.expect = 1
        return s
    off1 = kind in ("first_off", "both_off", "off")
    off2 = kind in ("second_off", "both_off")
    s.pair(i if (keep_rows or not (off1 and which == 1)) else pts.ZERO1, fam.shared, which if off1 else 0)
    if c == 2:
        q = (i if j is None else j) if kind == "mismatch" else i
        assert kind != "mismatch" or q != i
        if off2 and not keep_rows:
            s.pair(pts.ZERO1 if which == 1 else fam.neg, pts.ZERO2 if which == 2 else q, which)
        else:
            s.pair(fam.neg, q, which if off2 else 0)
    else:
        assert kind in ("live", "off")
    s.expect = 1 if kind in ("accept", "both_off", "off") else 0
    return s


def swapped(s):
    """the same two-pair product with its pairs exchanged: same value, another first G2 row"""
    import copy
    t = copy.deepcopy(s)
    assert len(t) == 2
    t.permute([1, 0])
    t.kind = s.kind + "_swapped"
    return t


def first_rows_shared(pts, specs, family=None):
    """every non-empty product's first G2 row IS the shared row (compared as rows, the way the dispatch does)"""
    fam = family_b(pts) if family is None else family
    row = pts.table2[fam.shared]
    return all(np.array_equal(pts.table2[s.i2[0]], row) for s in specs if len(s))


def verify_shaped_specs(pts, counts, seed, first=0, family=None, flag_share=None):
    """one verify-shaped product per entry of counts (each 0, 1 or 2), kinds, flag array and row kind drawn by a seeded generator; product p
    takes the point indices first + 2 p and first + 2 p + 1.  flag_share: as in ragged_specs.  The first-row invariant is asserted."""
    rng = np.random.default_rng(seed)
    m = len(counts)
    assert all(0 <= c <= 2 for c in counts) and first + 2 * m <= pts.n, "not enough points for distinct products"
    draw = rng.integers(0, 60, size=m)
    keep = rng.random(m)
    specs = []
    for p, (c, v) in enumerate(zip(counts, draw)):
        c, v = int(c), int(v)
        kind = VERIFY_KINDS[v % 5] if c == 2 else ("live", "off")[v % 2] if c == 1 else "empty"
        flagged = kind in ("second_off", "first_off", "both_off", "off")
        if flag_share is not None and flagged and keep[p] >= flag_share:
            kind = ("accept", "mismatch")[v % 2] if c == 2 else "live"
        specs.append(verify_product(pts, c, kind, first + 2 * p, first + 2 * p + 1, which=1 + (v // 5) % 2, keep_rows=bool((v // 10) % 2), family=family))
    assert first_rows_shared(pts, specs, family)
    return specs


def ragged_specs(pts, counts, seed, first=0, flag_share=None, family=None):
    build = product if family is None else (lambda *a: product(*a, family=family))
    return pc.ragged_specs(pts, counts, seed, first, flag_share, variants=VARIANTS, build=build)


def ragged_batch(pts, counts, seed, first=0):
    return layout(pts, ragged_specs(pts, counts, seed, first))


# ---- how much of a large call goes to the oracle (the rule the GPU tests and the CPU test of the inputs both apply)
SAMPLE_CAP = 400


def sample(specs, seed, fixed=(), thresholds=(), groups=10, cap=SAMPLE_CAP):
    """The products of a large call that go to the oracle: 64 seeded ones; the first and the last; products 9, 10, 11; both sides of every
    threshold the call touches; the last block (of `groups` products); `fixed`; one product per (pair count, class); EVERY product with a
    flag; then flagless accepting products of two or more pairs, in order, up to the cap."""
    m = len(specs)
    want = [0, m - 1, 9, 10, 11] + [t + d for t in thresholds for d in (-1, 0)] + list(range(m - 1 - (m - 1) % groups, m)) + list(fixed)
    seen = {}
    for p, s in enumerate(specs):
        seen.setdefault((len(s), s.kind), p)
    want += sorted(seen.values())
    want += [p for p, s in enumerate(specs) if has_flag(s)]
    want += np.random.default_rng(seed).choice(m, size=min(64, m), replace=False).tolist()
    pick = list(dict.fromkeys(int(p) for p in want if 0 <= p < m))
    assert len(pick) <= cap, (len(pick), cap)
    have = set(pick)
    pick += [p for p, s in enumerate(specs) if s.expect == 1 and len(s) >= 2 and not has_flag(s) and p not in have][:cap - len(pick)]
    return pick


def check_sample(specs, pick, seed, thresholds=(), groups=10, cap=SAMPLE_CAP):
    """the conditions of sample(), stated independently of how it was put together"""
    m, have = len(specs), set(pick)
    assert len(pick) == len(have) <= cap and all(0 <= p < m for p in pick)
    assert have >= set(np.random.default_rng(seed).choice(m, size=min(64, m), replace=False).tolist())
    assert have >= {p for p in (0, m - 1, 9, 10, 11) if p < m}
    assert all(t - 1 in have and (t >= m or t in have) for t in thresholds if 0 < t <= m)
    assert have >= set(range(m - 1 - (m - 1) % groups, m))
    assert {(len(specs[p]), specs[p].kind) for p in pick} == {(len(s), s.kind) for s in specs}
    assert have >= {p for p, s in enumerate(specs) if has_flag(s)}
    rest = [p for p, s in enumerate(specs) if s.expect == 1 and len(s) >= 2 and not has_flag(s) and p not in have]
    assert len(pick) == cap or not rest, "not filled to the cap"


# ---- the seeded batches of tests/test_pairing377_paths_gpu.py (built here so that the CPU test can assert on exactly these)
SHARED_MIN = 16384               # PairingEngine::SHARED_MIN_PRODUCTS
M_BIG = SHARED_MIN + 37          # 16384 = 10 * 1638 + 4; 16421 = 10 * 1642 + 1
N_BIG = 5 * M_BIG + 64           # points of the `big` fixture: the ragged 16421-batch strides by five


WIDE_MAX = 768                   # WideProduct<PP377>::MAX_PRODUCTS


def wide_counts(m):
    """m pair counts 0 ... 3: empty products at the start, in the middle and at the end"""
    c = np.random.default_rng(300 + m).integers(0, 4, size=m)
    c[[0, m // 2, m - 1]] = 0
    c[[1, m - 2]] = 3
    return [int(x) for x in c]


def wide_specs(pts, m, first=0):
    """m distinct products of 0 ... 3 pairs (the latency path's shape); above 300 products only about 60 % of the flagged ones stay
    flagged, so that all of them fit the oracle sample"""
    return ragged_specs(pts, wide_counts(m), seed=310 + m, first=first, flag_share=0.6 if m > 300 else None)


def threshold_counts():
    """16421 pair counts 0 ... 4, the draw of the BW6-761 threshold batch"""
    counts = np.random.default_rng(16384).integers(0, 5, size=M_BIG)
    counts[[0, 1, 2, 3, 4]] = [4, 0, 3, 2, 1]
    counts[[SHARED_MIN - 1, SHARED_MIN, M_BIG - 1]] = [4, 3, 4]
    return [int(c) for c in counts]


def threshold_specs(pts):
    return ragged_specs(pts, threshold_counts(), seed=16385, flag_share=0.03)


def verify_threshold_counts():
    """16421 counts 0 ... 2 of a verify-shaped batch: mostly two pairs, product 0 non-empty, empties and one-pair products throughout"""
    counts = np.random.default_rng(16390).choice([0, 1, 2, 2, 2, 2, 2, 2], size=M_BIG)
    counts[[0, 1, 2, 3]] = [2, 0, 1, 2]
    counts[[SHARED_MIN - 1, SHARED_MIN, M_BIG - 2, M_BIG - 1]] = [2, 1, 0, 2]
    return [int(c) for c in counts]


def verify_threshold_specs(pts, family=None):
    return verify_shaped_specs(pts, verify_threshold_counts(), seed=16391, family=family, flag_share=0.03)


def final_exp_counts():
    """5121 counts 0 ... 4 whose every prefix from 769 on holds a four-pair product (so no prefix is the latency or the split path)"""
    counts = np.random.default_rng(5121).integers(0, 5, size=5121)
    counts[[0, 1, 2, 3]] = [4, 0, 3, 1]
    counts[[3071, 3072, 5119, 5120]] = [2, 3, 4, 2]
    return [int(c) for c in counts]


def final_exp_specs(pts):
    return ragged_specs(pts, final_exp_counts(), seed=5122, flag_share=0.03)


def split_specs(pts, m, seed, first=0, family=None, flag_share=0.04):
    """m verify-shaped products of exactly two pairs"""
    return verify_shaped_specs(pts, [2] * m, seed, first, family, flag_share)


SPLIT_MAX = 5120                 # PairingEngine::SPLIT_MAX_PRODUCTS
SPLIT_SEED = 7000


def split_threshold_specs(pts):
    """5121 distinct verify-shaped two-pair products: the prefixes 769, 3072, 3073, 5120 take the split path, all 5121 leave it"""
    return split_specs(pts, SPLIT_MAX + 1, SPLIT_SEED)
