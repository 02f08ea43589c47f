"""The cases of the batched variable-base scalar multiplication (scalar_mul_batch_*, csrc/var_base.h), shared by tests/test_scalar_mul_cases.py
(which proves in Python that they are what they claim), tests/test_scalar_mul_host.py (the host twins under bounds tracking) and
tests/test_scalar_mul_gpu.py.  The expected rows come from the CPU oracle: orc_mul_* per row, then orc_normalize_*."""
import ctypes as C
import functools
import random
import numpy as np
from oracle.py import ecc
from oracle import cpu_oracle as co
import groth16_setup_ref as gs

X2 = ecc.X * ecc.X                       # the GLV split point of BLS12-377 G1: k = k0 + k1 x^2
WINDOWS = tuple(range(2, 9))             # the widths celo_amd_scalar_mul_set_window accepts (csrc/var_base.h VB_MIN_C .. VB_MAX_C)
GROUPS = sorted(gs.GROUPS)


class Group:
    def __init__(self, name):
        self.name = name
        self.gid, self.curve, self.g, self.sw, self.aw = gs.GROUPS[name]
        self.r, E1, E2, self.q, _, _ = gs.CURVES[self.curve]
        self.E = E1 if self.g == 1 else E2
        self.bits = self.r.bit_length()
        suffix = "bw6_761" if self.curve == "bw6_761" else name
        self.orc_mul, self.orc_normalize = "orc_mul_" + suffix, "orc_normalize_" + suffix

    @property
    def gen(self):
        return gs.generators(self.curve)[self.g - 1]

    def pack(self, pts):
        return gs.pack(self.curve, self.g, pts)


@functools.lru_cache(None)
def group(name):
    return Group(name)


# ---- the recoding of csrc/fixed_base.h, restated: signed c-bit digits in (-2^(c-1), 2^(c-1)], bottom window first
def windows(bits, c):
    return (bits + 1 + c - 1) // c


def recode(k, bits, c):
    """(digits, carries): digits[j] and the carry INTO window j, for j < windows(bits, c); the carry out of the top window is asserted 0"""
    H, digits, carries, carry = 1 << (c - 1), [], [], 0
    for j in range(windows(bits, c)):
        carries.append(carry)
        d = ((k >> (j * c)) & ((1 << c) - 1)) + carry
        carry = 1 if d > H else 0
        digits.append(d - (carry << c))
    assert carry == 0 and sum(d << (j * c) for j, d in enumerate(digits)) == k
    return digits, carries


def top_window(r, c):
    """the highest window a scalar below r can have a nonzero digit in"""
    return ((r - 1).bit_length() - 1) // c


def all_half_digits(r, c):
    """the longest scalar below r whose signed digits are all +2^(c-1)"""
    k, j = 0, 0
    while k + ((1 << (c - 1)) << (c * j)) < r:
        k += (1 << (c - 1)) << (c * j)
        j += 1
    return k


def carry_into_top(r, c):
    """2^(c t) - 1: digit -1 at the bottom, then a carry through every window into the top one, t"""
    return (1 << (c * top_window(r, c))) - 1


def mid_zero_windows(r, c):
    """1 at the bottom, 1 in window t - 1, zero windows between"""
    return 1 + (1 << (c * (top_window(r, c) - 1)))


def edge_scalars(r):
    top = 1 << ((r - 1).bit_length() - 1)
    return [("0", 0), ("1", 1), ("2", 2), ("3", 3), ("r-1", r - 1), ("r-2", r - 2), ("(r-1)/2", (r - 1) // 2), ("2^64-1", (1 << 64) - 1),
            ("2^64", 1 << 64), ("2^127-1", (1 << 127) - 1), ("2^127", 1 << 127), ("2^128", 1 << 128), ("top power of two", top),
            ("all ones below r", top - 1)]


def window_scalars(r):
    out = []
    for c in WINDOWS:
        out += [("c=%d all +half" % c, all_half_digits(r, c)), ("c=%d carry into top" % c, carry_into_top(r, c)), ("c=%d mid zeros" % c, mid_zero_windows(r, c))]
    return out


def uniform_scalars(r, seed, n=32):
    rng = random.Random(seed)
    return [("uniform %d" % i, rng.randrange(r)) for i in range(n)]


def glv_scalars():
    r = ecc.R377
    return [("x^2-1", X2 - 1), ("x^2", X2), ("x^2+1", X2 + 1), ("2x^2", 2 * X2), ("3x^2", 3 * X2), ("(2^60+7)x^2", ((1 << 60) + 7) * X2),
            ("floor(r/x^2) x^2", (r // X2) * X2), ("12345 < x^2", 12345), ("2^126 < x^2", 1 << 126), ("r-1 (127-bit k1)", r - 1)]


def glv_split(k):
    return k % X2, k // X2


@functools.lru_cache(None)
def scalar_list(name):
    """[(label, k)] for a group: edges, the window cases of every accepted width, 32 seeded uniform values; for BLS12-377 the GLV cases too
    (the subgroup entry runs the same list, and the plain entries lose nothing by them)"""
    g = group(name)
    out = edge_scalars(g.r) + window_scalars(g.r) + uniform_scalars(g.r, 1000 + g.gid + g.g)
    if g.curve == "bls12_377":
        out += glv_scalars()
    return out


# ---- points
def low_order_points(name):
    """[(label, point, order or None)]: curve points outside the prime-order subgroup, for the plain entries only"""
    if name == "bls12_377_g1":
        return [("(-1, 0) order 2", (ecc.Q377 - 1, 0), 2), ("(0, 1) order 3", (0, 1), 3)]
    if name == "bw6_761_g1":
        return [("(1, 0) order 2", (1, 0), 2)]
    if name == "bw6_761_g2":
        return [("(0, 2) order 3", (0, 2), 3)]
    # BLS12-377 G2: no point of small order is found (the cofactor of E'(Fq2) has no prime factor below 2000: g2_377_small_order_point), so
    # identity table entries are NOT covered for this group; a curve point outside the subgroup (order None = not small) still is
    P = g2_377_small_order_point()
    return [("[N/%d]Q order %d" % (P[1], P[1]), P[0], P[1])] if P else [("curve point outside the subgroup", g2_377_curve_point(), None)]


@functools.lru_cache(None)
def g2_377_curve_point():
    q, f2, rng = ecc.Q377, ecc.F2_377, random.Random(3772)
    while True:
        x = (rng.randrange(q), rng.randrange(q))
        y = f2.sqrt(f2.add(f2.mul(f2.sqr(x), x), ecc.B2_377))
        if y is not None:
            return (x, y)


def _isqrt_exact(n):
    import math
    s = math.isqrt(n)
    return s if s * s == n else None


@functools.lru_cache(None)
def g2_377_small_order_point():
    """(point, prime order) on E'(Fq2) of BLS12-377, or None if a few tries find none.  N = #E'(Fq2) is the sextic-twist order divisible by r,
    confirmed by [N]Q = O for a random Q; l is a small prime factor of N / r, the point [N / l]Q."""
    q, r, E, f2 = ecc.Q377, ecc.R377, ecc.E2_377, ecc.F2_377
    t = q + 1 - ecc.H1_377 * r
    t2 = t * t - 2 * q
    f = _isqrt_exact((4 * q * q - t2 * t2) // 3)
    if f is None:
        return None
    rng = random.Random(377)

    def random_point():
        while True:
            x = (rng.randrange(q), rng.randrange(q))
            y = f2.sqrt(f2.add(f2.mul(f2.sqr(x), x), ecc.B2_377))
            if y is not None:
                return (x, y)
    Q = random_point()
    for tr in ((t2 + 3 * f) // 2, (t2 - 3 * f) // 2, (-t2 + 3 * f) // 2, (-t2 - 3 * f) // 2, t2, -t2):
        N = q * q + 1 - tr
        if N % r == 0 and E.mul(Q, N) is None:
            break
    else:
        return None
    cof = N // r
    primes = [l for l in range(2, 2000) if all(l % d for d in range(2, int(l ** 0.5) + 1)) and cof % l == 0]
    for l in primes:
        for _ in range(3):
            P = E.mul(random_point(), N // l)
            if P is not None and E.on_curve(P) and E.mul(P, l) is None:
                return P, l
    return None


@functools.lru_cache(None)
def subgroup_points(name, count=6):
    g = group(name)
    rng = random.Random(50 + g.gid + g.g)
    return [g.gen, g.E.mul(g.gen, 0xC0FFEE)] + [g.E.mul(g.gen, rng.randrange(1, g.r)) for _ in range(count - 2)]


class Batch:
    """rows (points, flags, scalars) with their labels; plain_only marks rows that must not go through the subgroup entry"""
    def __init__(self, name, pts, ks, labels, plain_only):
        g = group(name)
        self.name, self.pts, self.ks, self.labels, self.plain_only = name, pts, ks, labels, plain_only
        self.xy, self.inf = g.pack(pts)
        self.sc = co.ints_to_limbs(ks, g.sw)
        self.n = len(ks)

    def take(self, idx):
        idx = list(idx)
        return Batch(self.name, [self.pts[i] for i in idx], [self.ks[i] for i in idx], [self.labels[i] for i in idx], [self.plain_only[i] for i in idx])


@functools.lru_cache(None)
def case_batch(name, subgroup_only=False):
    """every scalar of scalar_list on a rotation of subgroup points with the identity flag on every 11th row, and (plain entries) every
    low-order point under the small scalars, the near-order ones and a few uniform ones"""
    g = group(name)
    pts, ks, labels, plain = [], [], [], []
    sub = subgroup_points(name)
    for i, (lab, k) in enumerate(scalar_list(name)):
        P = None if i % 11 == 7 else sub[i % len(sub)]
        pts.append(P); ks.append(k); labels.append("%s on %s" % (lab, "identity" if P is None else "subgroup point %d" % (i % len(sub)))); plain.append(False)
    if not subgroup_only:
        rng = random.Random(9)
        for plab, P, order in low_order_points(name):
            for lab, k in edge_scalars(g.r)[:7] + [("4", 4), ("5", 5), ("6", 6)] + [("uniform", rng.randrange(g.r)) for _ in range(4)]:
                pts.append(P); ks.append(k); labels.append("%s on %s" % (lab, plab)); plain.append(True)
    return Batch(name, pts, ks, labels, plain)


# ---- expected rows by the CPU oracle
def oracle_rows(name, xy, inf, sc):
    """orc_mul_* per row (a flagged row is the identity), then orc_normalize_* over all of them: (rows, flags), zero rows for identities"""
    g = group(name)
    lib = co.lib()
    xy = np.ascontiguousarray(xy, dtype=np.uint64).reshape(-1, g.aw)
    sc = np.ascontiguousarray(sc, dtype=np.uint64).reshape(-1, g.sw)
    n = xy.shape[0]
    jw = 3 * g.aw // 2
    jac = np.zeros((n, jw), dtype=np.uint64)
    mul = getattr(lib, g.orc_mul)
    for i in range(n):
        if inf is not None and inf[i]:
            continue                       # Z = 0: the identity
        k = np.ascontiguousarray(sc[0 if sc.shape[0] == 1 else i])
        row = np.ascontiguousarray(xy[i])
        assert mul(row.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p), jac[i].ctypes.data_as(C.c_void_p)) == 0
    out = np.zeros((n, g.aw), dtype=np.uint64)
    oinf = np.zeros(n, dtype=np.uint8)
    assert getattr(lib, g.orc_normalize)(jac.ctypes.data_as(C.c_void_p), C.c_size_t(n), out.ctypes.data_as(C.c_void_p), oinf.ctypes.data_as(C.c_void_p)) == 0
    out[oinf != 0] = 0
    return out, oinf


_EXPECTED = {}


def expected(name):
    """the oracle's rows of case_batch(name), computed once"""
    if name not in _EXPECTED:
        b = case_batch(name)
        _EXPECTED[name] = oracle_rows(name, b.xy, b.inf, b.sc)
    return _EXPECTED[name]


@functools.lru_cache(None)
def seeded_batch(name, n, seed):
    """n rows of uniform scalars on subgroup points (a few edge scalars and flagged rows among them)"""
    g = group(name)
    rng = random.Random(seed)
    sub = subgroup_points(name)
    ks = [rng.randrange(g.r) for _ in range(n)]
    for i, k in enumerate([0, 1, g.r - 1, X2 if g.curve == "bls12_377" else 2][:n]):
        ks[(i * 5) % n] = k
    pts = [None if (n > 8 and i % 13 == 4) else sub[rng.randrange(len(sub))] for i in range(n)]
    return Batch(name, pts, ks, ["seeded %d" % i for i in range(n)], [False] * n)


_SEEDED_EXPECTED = {}


def seeded_expected(name, n, seed):
    """the oracle's rows of seeded_batch(name, n, seed), computed once"""
    if (name, n, seed) not in _SEEDED_EXPECTED:
        b = seeded_batch(name, n, seed)
        _SEEDED_EXPECTED[name, n, seed] = oracle_rows(name, b.xy, b.inf, b.sc)
    return _SEEDED_EXPECTED[name, n, seed]
