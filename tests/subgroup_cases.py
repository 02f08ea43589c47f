"""The cases of the bulk point validator (check_points_*, csrc/check.h) and of the BW6-761 subgroup test by endomorphism
(csrc/wire761.h w761_in_subgroup_endo), shared by tests/test_subgroup_cases.py (which proves every expected status with the oracle: the
curve equation and a full mul(P, r)), tests/test_subgroup_host.py (the host twins under bounds tracking) and tests/test_check_points_gpu.py.

A case is a ROW as the entry points take it (arkworks Montgomery limbs, 12 or 24 u64), its identity flag and the statuses expected at
level 1 (curve equation) and level 2 (curve and subgroup): 0 good, 1 the flag is set, 2 a coordinate is not below q or the point is off the
curve, 3 on the curve outside the subgroup."""
import functools
import math
import random
import numpy as np
from oracle.py import ecc
from oracle import cpu_oracle as co
import groth16_setup_ref as gs

GROUPS = ("bls12_377_g1", "bls12_377_g2", "bw6_761_g1", "bw6_761_g2")
X = ecc.X
# the endomorphism a + b phi of norm r (csrc/wire761.h), and the better-known short vector of norm 3 r that is NOT used
ENDO_A = (2 * X ** 3 - 2 * X ** 2 - X + 1) // 3
ENDO_B = (X ** 3 - X ** 2 - 2 * X - 1) // 3
SHORT_A, SHORT_B = X + 1, X ** 3 - X ** 2 + 1


class Group:
    def __init__(self, name):
        self.name = name
        self.gid = GROUPS.index(name)
        self.curve = "bw6_761" if name.startswith("bw6") else "bls12_377"
        self.g = 1 if name.endswith("g1") else 2
        self.q = ecc.Q761 if self.curve == "bw6_761" else ecc.Q377
        self.r = ecc.R761 if self.curve == "bw6_761" else ecc.R377
        self.E = {"bls12_377_g1": ecc.E1_377, "bls12_377_g2": ecc.E2_377, "bw6_761_g1": ecc.E1_761, "bw6_761_g2": ecc.E2_761}[name]
        self.words = 12 if name == "bls12_377_g1" else 24
        self.limbs = 12 if self.curve == "bw6_761" else 6               # u64 per base-field element
        self.gen = gs.generators(self.curve)[self.g - 1]

    def pack(self, pts):
        return gs.pack(self.curve, self.g, pts)[0]

    def components(self, row):
        """the row's base-field elements as the integers its limbs hold (Montgomery form, possibly not below q)"""
        return co.limbs_to_ints(np.ascontiguousarray(row, dtype=np.uint64).reshape(-1, self.limbs), self.limbs)

    def point_of(self, row):
        """the affine point a row with canonical components stands for"""
        rinv = pow(1 << (64 * self.limbs), -1, self.q)
        c = [v * rinv % self.q for v in self.components(row)]
        return (c[0], c[1]) if len(c) == 2 else ((c[0], c[1]), (c[2], c[3]))

    def random_curve_point(self, rng):
        q, E = self.q, self.E
        while True:
            if E.f2:
                x = (rng.randrange(q), rng.randrange(q))
                y = E.f2.sqrt(E.f2.add(E.f2.mul(E.f2.sqr(x), x), E.b))
            else:
                x = rng.randrange(q)
                y = ecc.sqrt_fp((x * x * x + E.b) % q, q)
            if y is not None:
                return (x, y)


@functools.lru_cache(None)
def group(name):
    return Group(name)


# ---- BW6-761: the two cube roots of unity, the group orders and the cofactors
@functools.lru_cache(None)
def betas():
    """(g^((q-1)/3), its square) for the smallest g that gives a primitive cube root: the beta of G1 and of G2 in csrc/wire761.h"""
    q, g = ecc.Q761, 2
    while pow(g, (q - 1) // 3, q) == 1:
        g += 1
    b = pow(g, (q - 1) // 3, q)
    return b, b * b % q


def phi(beta, P):
    return None if P is None else (beta * P[0] % ecc.Q761, P[1])


def endo_image(E, beta, P, a=ENDO_A, b=ENDO_B):
    """[a]P + [b]phi(P)"""
    return E.add(E.mul(P, a), E.mul(phi(beta, P), b))


@functools.lru_cache(None)
def order_761(name):
    """#E(Fq) of a BW6-761 group's curve: 4 q = t^2 + 3 f^2 (Cornacchia), the order is q + 1 - trace for one of the six traces of the
    curves with j = 0 - the one that kills two random points"""
    g, q = group(name), ecc.Q761
    s = ecc.sqrt_fp((-3) % q, q)
    s = s if s % 2 else q - s
    a, b, lim = 2 * q, s, math.isqrt(4 * q)
    while b > lim:
        a, b = b, a % b
    t = b
    f = math.isqrt((4 * q - t * t) // 3)
    assert t * t + 3 * f * f == 4 * q
    rng = random.Random(7610 + g.g)
    P, Q = g.random_curve_point(rng), g.random_curve_point(rng)
    found = [n for n in {q + 1 - tr for tr in (t, -t, (t + 3 * f) // 2, -(t + 3 * f) // 2, (t - 3 * f) // 2, -(t - 3 * f) // 2)}
             if g.E.mul(P, n) is None and g.E.mul(Q, n) is None]
    assert len(found) == 1 and found[0] % g.r == 0
    return found[0]


def cofactor_761(name):
    return order_761(name) // group(name).r


@functools.lru_cache(None)
def order13_point():
    """a point of order 13 on the BW6-761 G2 curve: [h2 r / 13] of a random point, skipping the identity"""
    g, n = group("bw6_761_g2"), order_761("bw6_761_g2")
    assert n % 13 == 0
    rng = random.Random(13)
    while True:
        P = g.E.mul(g.random_curve_point(rng), n // 13)
        if P is not None:
            assert g.E.mul(P, 13) is None
            return P


# ---- the points
@functools.lru_cache(None)
def subgroup_points(name, count=3):
    g = group(name)
    rng = random.Random(900 + g.gid)
    return [g.gen] + [g.E.mul(g.gen, rng.randrange(2, g.r)) for _ in range(count - 1)]


@functools.lru_cache(None)
def curve_points(name, count=3):
    """random points of the curve (a random x that has a y; no cofactor clearing): outside the subgroup"""
    g = group(name)
    rng = random.Random(910 + g.gid)
    return [g.random_curve_point(rng) for _ in range(count)]


@functools.lru_cache(None)
def low_order_points(name):
    """[(label, point)]: points of small order and their sums with a subgroup point - on the curve, outside the subgroup"""
    g = group(name)
    E, G, q = g.E, g.gen, g.q
    if name == "bls12_377_g1":
        small = [("(-1, 0) order 2", (q - 1, 0)), ("(0, 1) order 3", (0, 1))]
    elif name == "bw6_761_g1":
        b1, b2 = betas()
        small = [("(1, 0) order 2", (1, 0)), ("(beta, 0) order 2", (b1, 0)), ("(beta^2, 0) order 2", (b2, 0))]
    elif name == "bw6_761_g2":
        T = (0, 2)
        return [("(0, 2) order 3", T), ("(0, -2) order 3", (0, q - 2)), ("G + (0, 2)", E.add(G, T)), ("G - (0, 2)", E.add(G, E.neg(T))),
                ("order 13", order13_point()), ("G + order 13", E.add(G, order13_point()))]
    else:
        return []                                                        # BLS12-377 G2: no point of small order is known (scalar_mul_cases.py)
    return small + [("G + " + label, E.add(G, P)) for label, P in small]


@functools.lru_cache(None)
def on_curve_cases(name):
    """[(label, point, in the subgroup)]: every case that is a finite point of the curve - what the serialized decoders can be given too"""
    g = group(name)
    E = g.E
    out = []
    for i, P in enumerate(subgroup_points(name)):
        out += [("subgroup %d" % i, P, True), ("-subgroup %d" % i, E.neg(P), True)]
    for i, P in enumerate(curve_points(name)):
        out.append(("curve point %d" % i, P, False))
    C = E.mul(curve_points(name)[0], g.r)                                # a pure cofactor point
    if C is not None:
        out.append(("r * curve point 0", C, False))
    out += [(label, P, False) for label, P in low_order_points(name)]
    return out


class Cases:
    def __init__(self, name, labels, rows, inf, want1, want2):
        self.name, self.labels = name, labels
        self.xy = np.ascontiguousarray(rows, dtype=np.uint64)
        self.inf = np.array(inf, dtype=np.uint8)
        self.want = {1: np.array(want1, dtype=np.uint8), 2: np.array(want2, dtype=np.uint8)}
        self.n = len(labels)

    def take(self, idx):
        idx = list(idx)
        return Cases(self.name, [self.labels[i] for i in idx], self.xy[idx], self.inf[idx], self.want[1][idx], self.want[2][idx])

    def first_bad(self, level):
        bad = np.nonzero(self.want[level] >= 2)[0]
        return int(bad[0]) if bad.size else self.n


@functools.lru_cache(None)
def cases(name):
    g = group(name)
    q, L = g.q, g.limbs
    labels, rows, inf, w1, w2 = [], [], [], [], []

    def put(label, row, flag, s1, s2):
        labels.append(label); rows.append(np.array(row, dtype=np.uint64)); inf.append(flag); w1.append(s1); w2.append(s2)
    on = on_curve_cases(name)
    packed = g.pack([P for _, P, _ in on])
    for (label, _, member), row in zip(on, packed):
        put(label, row, 0, 0, 0 if member else 3)
    good = packed[0]
    # off the curve
    P = subgroup_points(name)[1]
    y1 = (((P[1][0] + 1) % q, P[1][1]) if g.E.f2 else (P[1] + 1) % q)
    put("(x, y + 1)", g.pack([(P[0], y1)])[0], 0, 2, 2)
    put("(0, 0) without the flag", np.zeros(g.words, dtype=np.uint64), 0, 2, 2)
    # a coordinate that is no field element: q itself, 2^(64 L) - 1 (the limbs hold these values as they are)
    q_limbs, ones = co.ints_to_limbs([q], L)[0], np.full(L, ~np.uint64(0), dtype=np.uint64)
    ncomp = g.words // L
    for c in range(ncomp):
        r1 = good.copy(); r1[c * L:(c + 1) * L] = q_limbs
        put("component %d == q" % c, r1, 0, 2, 2)
        r2 = good.copy(); r2[c * L:(c + 1) * L] = ones
        put("component %d == 2^%d - 1" % (c, 64 * L), r2, 0, 2, 2)
    # flagged rows: the identity, whatever the coordinates hold
    put("flag, zero row", np.zeros(g.words, dtype=np.uint64), 1, 1, 1)
    put("flag, all-ones row", np.full(g.words, ~np.uint64(0), dtype=np.uint64), 1, 1, 1)
    put("flag, off-curve row", rows[len(on)], 1, 1, 1)
    put("flag, subgroup row", good, 7, 1, 1)                             # any nonzero flag byte
    put("flag, curve point row", packed[2 * len(subgroup_points(name))], 1, 1, 1)
    return Cases(name, labels, np.stack(rows), inf, w1, w2)


@functools.lru_cache(None)
def seeded_curve_points(name, n, seed):
    """n seeded random curve points, every fourth pushed into the subgroup by the cofactor where that is known (BW6-761), else replaced by a
    multiple of the generator: [(point, in the subgroup)] by the oracle's mul(P, r)"""
    g = group(name)
    rng = random.Random(seed)
    out = []
    for i in range(n):
        if i % 4 == 3:
            P = g.E.mul(g.random_curve_point(rng), cofactor_761(name)) if g.curve == "bw6_761" else g.E.mul(g.gen, rng.randrange(1, g.r))
        else:
            P = g.random_curve_point(rng)
        if P is not None:
            out.append((P, g.E.mul(P, g.r) is None))
    return out
