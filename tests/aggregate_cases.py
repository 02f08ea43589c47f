"""The cases of the masked segmented point sums (aggregate_by_bitmap_*, csrc/aggregate.h), shared by tests/test_aggregate_bitmap_host.py (the
host twin under bounds tracking) and tests/test_aggregate_bitmap_gpu.py.  Expected sums come from oracle/py/ecc.py: the selected points added
one after the other with Curve.add, computed once per (key list, bitmap) and kept."""
import functools
import numpy as np
from oracle.py import ecc
from oracle import cpu_oracle as co

GROUPS = ("bls12_377_g1", "bls12_377_g2")
LANES = (1, 2, 4, 8, 16, 32, 64)
SET_SIZES = (0, 1, 2, 7, 8, 9, 63, 64, 65, 100, 257, 1025)
SEAL_COUNTS = (1, 2, 63, 64, 65, 257)
_CURVES = {"bls12_377_g1": (0, ecc.E1_377, ecc.G1_377, co.pack_g1_377, 12), "bls12_377_g2": (1, ecc.E2_377, ecc.G2_377, co.pack_g2_377, 24)}


class Group:
    def __init__(self, name):
        self.name = name
        self.gid, self.E, self.gen, self.pack, self.aw = _CURVES[name]


@functools.lru_cache(None)
def group(name):
    return Group(name)


@functools.lru_cache(None)
def keys(name, n, seed=7):
    """n distinct subgroup points P_j = (a + j b) G, as a tuple of affine points"""
    g = group(name)
    rng = ecc.SplitMix64(seed)
    P, step = g.E.mul(g.gen, ecc.random_scalar(rng, ecc.R377)), g.E.mul(g.gen, ecc.random_scalar(rng, ecc.R377))
    out = []
    for _ in range(n):
        out.append(P)
        P = g.E.add(P, step)
    return tuple(out)


def patterns(n):
    """[(label, (n,) uint8)]: the bitmaps every set size is summed under.  half and half +- 1 straddle the side rule (a tie sums the ones,
    one more one than zeros takes the complement); 'bytes' has set bytes that are not 1."""
    rng = np.random.default_rng(1000 + n)
    z = lambda: np.zeros(n, dtype=np.uint8)
    out = [("none", z()), ("all", np.ones(n, dtype=np.uint8))]
    if n == 0:
        return out
    first, last, alt, but_one = z(), z(), z(), np.ones(n, dtype=np.uint8)
    first[0], last[-1] = 1, 1
    alt[::2] = 1
    but_one[n // 3] = 0
    out += [("first only", first), ("last only", last), ("alternating", alt), ("all but one", but_one)]
    for label, ones in (("half - 1", n // 2 - 1), ("half", n // 2), ("half + 1", n // 2 + 1)):
        if 0 <= ones <= n:
            b = z()
            b[rng.permutation(n)[:ones]] = 1
            out.append((label, b))
    b = z()
    where = rng.permutation(n)[:(2 * n + 2) // 3]
    b[where] = rng.choice(np.array([2, 0x80, 0xFF, 1, 3], dtype=np.uint8), size=where.size)
    out.append(("bytes", b))
    return out


_SUMS = {}


def oracle_sum(name, pts, bits):
    """the sum of the points of `pts` (a tuple; None = the identity, a flagged row) under the non-zero bytes of bits, by oracle/py/ecc.py"""
    key = (name, tuple(pts), bytes(np.asarray(bits, dtype=np.uint8) != 0))
    if key not in _SUMS:
        E, acc = group(name).E, None
        for P, b in zip(pts, bits):
            if b:
                acc = E.add(acc, P)
        _SUMS[key] = acc
    return _SUMS[key]


def expected(name, pts, bitmaps):
    """(rows, flags, counts) of one seal per bitmap over the key list pts"""
    g = group(name)
    rows, inf = g.pack([oracle_sum(name, pts, b) for b in bitmaps])
    return rows, inf, np.array([int(np.count_nonzero(b)) for b in bitmaps], dtype=np.uint32)


@functools.lru_cache(None)
def special_key_lists(name):
    """[(label, points, bitmap, the sum is the identity)]: key lists that meet the doubling and cancelling branches in both phases.  With L
    lanes, rows j and j + L meet in a lane's own mixed additions; rows of different lanes meet in the fold."""
    g = group(name)
    P, Q, S = keys(name, 3, seed=11)
    neg, dbl = g.E.neg, lambda X: g.E.add(X, X)
    ones = lambda k: np.ones(k, dtype=np.uint8)
    out = [("duplicate adjacent keys", (P, P, Q), ones(3), False), ("P and -P", (P, neg(P)), ones(2), True),
           ("P, P, -2P", (P, P, neg(dbl(P))), ones(3), True), ("a selected flagged row", (P, None, Q), ones(3), False),
           ("only flagged rows", (None, None), ones(2), True),
           # P twice with an unselected row ahead: at L = 4 lane 0 has nothing, takes P from lane 2 in the fold's first round and meets lane 1's
           # P in the second (the doubling branch on a point that came out of the buffer)
           ("P, P behind a gap", (Q, P, P, S), np.array([0, 1, 1, 0], dtype=np.uint8), False),
           ("P, -P behind a gap", (Q, P, neg(P), S), np.array([0, 1, 1, 0], dtype=np.uint8), True)]
    # the same key 9 and 66 times: every lane's partial and every fold round doubles
    out += [("P x 9", (P,) * 9, ones(9), False), ("P x 66", (P,) * 66, ones(66), False)]
    # 64 keys and their negatives, interleaved so that lanes cancel in the fold (L <= 64) or inside a lane
    many = keys(name, 64)
    out.append(("64 keys and their negatives", tuple(many) + tuple(neg(X) for X in many), ones(128), True))
    return out


def pack_keys(name, pts):
    return group(name).pack(list(pts))
