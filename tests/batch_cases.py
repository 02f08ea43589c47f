"""Inputs for the batched small-MSM tests (csrc/msm_batch.h, MsmEngine::run_batch), with the dispatch each call must take and the Horner
branch each hand-built instance must reach known BY CONSTRUCTION (no GPU import at module level).

Group table.  GROUPS binds the four msm_batch_* groups to their row width (u64 words per affine point), scalar container (u64 limbs, 32-bit
words), SCALAR_BITS (the bit length of the scalar field's modulus: bits from there up are ignored), the oracle's result kind, the Python
curve and a generator: the group generators of BLS12-377, alpha_g1 / beta_g2 of the golden Groth16 verifying key for BW6-761 (the points
synthetic.device_points multiplies on the GPU side).

Dispatch.  expected_dispatch restates the rule of DESIGN.md section 6 / include/celo_bls_amd.h (the msm_batch_* block):
  side path   an instance above 1024 points, or no point at all: every instance goes through the large pipeline
  bits        the length of the longest scalar present, bits from SCALAR_BITS up not counted; at least 1
  nd          subgroup entry of G2 only: 1 up to 64 bits, 2 up to 126, 3 up to 189, else 4 - and 1 wherever nd * max_n > 1024
  c           3, raised while 16 << c <= nd * max_n, at most 7 (a forced window is clamped to 3..7)
  windows     (eff_bits + c) // c with eff_bits = 64 on a split call, bits otherwise
  buckets     m * windows * 2^(c-1)

Signed digits.  recode is the plain definition of what k_batch_sort computes: window w of a scalar is d_w in (-2^(c-1), 2^(c-1)], a digit
above 2^(c-1) becoming d - 2^c with a carry into the next window.  bucket_trace replays an instance on those digits with the Python curve:
the buckets, the window sums and the Horner chain acc <- 2^c acc + W_w from the top window down, naming what every addition is
('load' into an identity accumulator, 'add', 'double' when acc == W_w, 'cancel' when acc == -W_w).

Horner branch builders (each for the window c the instance will get; P, R any points):
  doubling          [P, 2^c P] x [2^c, 1]               W_1 = P, W_0 = 2^c P: the last addition adds a point to itself    -> 2^(c+1) P
  cancel_and_go_on  [P, -2^c P, R] x [2^2c, 2^c, 1]     the chain reaches the identity at window 1 and goes on            -> R
  all_cancel        [P, -P] x [k, k]                    every bucket holds a cancelling pair: every window sum is empty   -> identity
  live_identity     [P, P] x [k, r - k]                 every window up to r's top digit non-empty, the sum is r P        -> identity
  live_identity_short  [P, P, -P] x [a, b, a + b]       the same with short scalars (the G2 subgroup entry splits them)   -> identity"""
import json
import os
import numpy as np
from oracle.py import ecc
from oracle import cpu_oracle as co

BATCH_MAX_N = 1024
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_VK = {}


def _golden_vk():
    if not _VK:
        from oracle.py import epoch as ep
        with open(os.path.join(_ROOT, "tests", "golden", "reference_vectors.json")) as f:
            _VK.update(ep.parse_vk(bytes.fromhex(json.load(f)["groth16_bw6_761"]["vk"])))
    return _VK


class Group:
    """rows: u64 words per affine point; limbs / words: the scalar container in u64 / u32; kind: what co.jac_to_affine calls the result"""

    def __init__(self, name, rows, limbs, scalar_bits, kind, curve, order, pack, generator, coord_limbs, coords):
        self.name, self.rows, self.limbs, self.words, self.scalar_bits, self.kind = name, rows, limbs, 2 * limbs, scalar_bits, kind
        self.curve, self.order, self.pack, self.generator = curve, order, pack, generator
        self.coord_limbs, self.coords = coord_limbs, coords        # u64 limbs per base-field element, base-field elements per point

    @property
    def q(self):
        return self.curve.p

    def neg_rows(self, rows):
        """the rows of -P for rows of P (Montgomery limbs: -(y R) = q - y R for every base-field element of y); a zero row stays zero"""
        rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, self.rows)
        half = self.rows // 2
        y = co.limbs_to_ints(rows[:, half:], self.coord_limbs)
        out = rows.copy()
        out[:, half:] = co.ints_to_limbs([(self.q - v) % self.q for v in y], self.coord_limbs).reshape(-1, half)
        return out

    def multiples(self, ks):
        """Python-oracle multiples k * generator (a handful: the hand-built cases)"""
        G = self.generator()
        return [self.curve.mul(G, k) for k in ks]


GROUPS = {
    "bls12_377_g1": Group("bls12_377_g1", 12, 4, 253, "g1_377", ecc.E1_377, ecc.R377, co.pack_g1_377, lambda: ecc.G1_377, 6, 2),
    "bls12_377_g2": Group("bls12_377_g2", 24, 4, 253, "g2_377", ecc.E2_377, ecc.R377, co.pack_g2_377, lambda: ecc.G2_377, 6, 4),
    "bw6_761_g1": Group("bw6_761_g1", 24, 6, 377, "761", ecc.E1_761, ecc.R761, co.pack_761, lambda: _golden_vk()["alpha_g1"], 12, 2),
    "bw6_761_g2": Group("bw6_761_g2", 24, 6, 377, "761", ecc.E2_761, ecc.R761, co.pack_761, lambda: _golden_vk()["beta_g2"], 12, 2),
}
# (group, subgroup entry): the five msm_batch_* entry points
ENTRIES = [("bls12_377_g1", False), ("bls12_377_g2", False), ("bls12_377_g2", True), ("bw6_761_g1", False), ("bw6_761_g2", False)]


# ---- the dispatch rule ---------------------------------------------------------------------------------------------------------
def window_for(n, forced_c=0):
    if forced_c:
        return min(7, max(3, forced_c))
    c = 3
    while c < 7 and (16 << c) <= n:
        c += 1
    return c


def gls_digits(group, max_n, bits, subgroup):
    if not subgroup or group != "bls12_377_g2" or bits <= 64:
        return 1
    nd = 2 if bits <= 126 else 3 if bits <= 189 else 4
    return nd if nd * max_n <= BATCH_MAX_N else 1


def expected_dispatch(group, sizes, bits, subgroup=False, forced_c=0):
    """-> (c, windows, buckets, nd), or "side" for a call that goes through the large pipeline instance by instance.  bits: the length of
    the longest scalar of the call."""
    g = GROUPS[group]
    m, max_n = len(sizes), max(sizes, default=0)
    if max_n > BATCH_MAX_N or sum(sizes) == 0:
        return "side"
    bits = max(1, min(bits, g.scalar_bits))
    nd = gls_digits(group, max_n, bits, subgroup)
    c = window_for(nd * max_n, forced_c)
    nw = ((64 if nd > 1 else bits) + c) // c
    return c, nw, m * nw * (1 << (c - 1)), nd


# ---- signed digits and the replay of an instance ----------------------------------------------------------------------------------
def recode(k, c, nw):
    """the nw signed base-2^c digits of k, d_w in (-2^(c-1), 2^(c-1)]"""
    half, out = 1 << (c - 1), []
    for _ in range(nw):
        d = k & ((1 << c) - 1)
        k >>= c
        if d > half:
            d -= 1 << c
            k += 1
        out.append(d)
    assert k == 0, "nw windows do not hold the scalar"
    return out


def bucket_trace(group, points, scalars, c, nw):
    """-> dict(buckets: per window {magnitude: [signed points]}, wsum: the nw window sums, events: [(window, what)], result)"""
    E = GROUPS[group].curve
    buckets = [dict() for _ in range(nw)]
    for P, k in zip(points, scalars):
        if P is None:
            continue
        for w, d in enumerate(recode(k, c, nw)):
            if d:
                buckets[w].setdefault(abs(d), []).append(P if d > 0 else E.neg(P))
    wsum = []
    for w in range(nw):
        acc = None
        for mag, members in buckets[w].items():
            s = None
            for Q in members:
                s = E.add(s, Q)
            acc = E.add(acc, E.mul(s, mag))
        wsum.append(acc)
    acc, events = None, []
    for w in range(nw - 1, -1, -1):
        for _ in range(c):
            acc = E.add(acc, acc)
        W = wsum[w]
        if W is not None:
            events.append((w, "load" if acc is None else "double" if acc == W else "cancel" if acc == E.neg(W) else "add"))
        acc = E.add(acc, W)
    return {"buckets": buckets, "wsum": wsum, "events": events, "result": acc}


# ---- the builders: (points, scalars, expected point) -------------------------------------------------------------------------------
def doubling(group, c, P):
    E = GROUPS[group].curve
    Q = E.mul(P, 1 << c)
    return [P, Q], [1 << c, 1], E.add(Q, Q)


def cancel_and_go_on(group, c, P, R):
    E = GROUPS[group].curve
    return [P, E.neg(E.mul(P, 1 << c)), R], [1 << (2 * c), 1 << c, 1], R


def all_cancel(group, c, P, k):
    E = GROUPS[group].curve
    return [P, E.neg(P)], [k, k], None


def live_identity_scalars(order, c):
    """k and order - k such that window w of the two together is non-empty for every w below the digit count of `order` written with the
    digits 1..2^c (the bijective base-2^c numeral: every positive integer has exactly one, and it has no zero digit): s_w of them split as
    a_w = ceil(s_w / 2), b_w = floor(s_w / 2), both in [0, 2^(c-1)], so a_w and b_w ARE the signed digits of k = sum a_w 2^(cw) and of
    order - k, and window w holds (a_w + b_w) P = s_w P, which is not the identity (0 < s_w <= 2^c < order).  -> (k, order - k, digit count)"""
    s, n = [], order
    while n > 0:
        d = n & ((1 << c) - 1)
        if d == 0:
            d = 1 << c
        s.append(d)
        n = (n - d) >> c
    k = sum(((d + 1) // 2) << (c * w) for w, d in enumerate(s))
    return k, order - k, len(s)


def live_identity(group, c, P):
    g = GROUPS[group]
    k, k2, _ = live_identity_scalars(g.order, c)
    return [P, P], [k, k2], None


def live_identity_short(group, P, a, b):
    E = GROUPS[group].curve
    return [P, P, E.neg(P)], [a, b, a + b], None


BUILDERS = ("doubling", "cancel_and_go_on", "all_cancel", "live_identity")


def build(name, group, c, P, R, k):
    """the builder `name` for window c: P its point, R the survivor of cancel_and_go_on, k the scalar of all_cancel"""
    if name == "doubling":
        return doubling(group, c, P)
    if name == "cancel_and_go_on":
        return cancel_and_go_on(group, c, P, R)
    if name == "all_cancel":
        return all_cancel(group, c, P, k)
    if name == "live_identity":
        return live_identity(group, c, P)
    raise KeyError(name)


def scalar_of_bits(bits, seed):
    """a seeded scalar of exactly `bits` bits"""
    rng = ecc.SplitMix64(seed)
    k = 0
    for _ in range((bits + 63) // 64):
        k = (k << 64) | rng.next()
    return (k & ((1 << bits) - 1)) | (1 << (bits - 1))


def full_scalar(group, seed):
    """a scalar of exactly SCALAR_BITS - 1 bits (252 / 376: below the modulus)"""
    return scalar_of_bits(GROUPS[group].scalar_bits - 1, seed)


# ---- calls in row form (the GPU tests: points from the generator kernel) -----------------------------------------------------------------
def random_scalars(n, limbs, bits, seed):
    """n uniform scalars below 2^bits, canonical limbs (n, limbs) uint64"""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, size=(n, 8 * limbs), dtype=np.uint8)
    raw[:, (bits + 7) // 8:] = 0
    if bits % 8:
        raw[:, (bits - 1) // 8] &= (1 << (bits % 8)) - 1
    return raw.view(np.uint64).reshape(n, limbs).copy()


def set_scalar(sc, i, k):
    sc[i] = co.ints_to_limbs([k], sc.shape[1])[0]


def longest(sc):
    """bit length of the longest scalar of (n, limbs) uint64 rows"""
    if sc.shape[0] == 0:
        return 0
    top = 0
    for j in range(sc.shape[1] - 1, -1, -1):
        v = int(np.bitwise_or.reduce(sc[:, j]))
        if v:
            top = 64 * j + v.bit_length()
            break
    return top


class Call:
    """one msm_batch call: rows (tot, A), inf (tot), scalars (tot, S), offsets (m + 1)"""

    def __init__(self, group, rows, inf, scalars, offsets):
        self.group, self.rows, self.inf, self.scalars, self.offsets = group, rows, inf, scalars, np.asarray(offsets, dtype=np.uint32)

    @property
    def sizes(self):
        return [int(b) - int(a) for a, b in zip(self.offsets[:-1], self.offsets[1:])]

    def bits(self):
        return longest(self.scalars)


def mix_instance(g, rows, inf, sc, lo, k):
    """what tests/test_batch_gpu.py's _check_batch mixes into an instance of 8 points or more - an identity-flagged base, a repeated
    (point, scalar) pair, the scalars 0 and 1 - and an opposite pair with equal scalars (rows 2 and 7)"""
    if k < 8:
        return
    inf[lo + 3] = 1
    rows[lo + 5] = rows[lo + 6]
    sc[lo + 5] = sc[lo + 6]
    sc[lo + 0] = 0
    sc[lo + 1] = 0
    sc[lo + 1, 0] = 1
    rows[lo + 7] = g.neg_rows(rows[lo + 2])[0]
    sc[lo + 7] = sc[lo + 2]


def mixed_call(group, table, sizes, bits, seed, top_at=None):
    """instances of the given sizes over the first rows of `table` (distinct points), uniform scalars below 2^bits with the mix of
    mix_instance in every instance of 8 points or more; one scalar is exactly 2^bits - 1 (at flat index top_at; default: row 4 of the
    largest instance, which the mix leaves alone, or its last row), so the longest scalar of the call has `bits` bits by construction"""
    g = GROUPS[group]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    tot = int(offs[-1])
    assert tot <= table.shape[0]
    rows = np.array(table[:tot], dtype=np.uint64).reshape(tot, g.rows)
    inf = np.zeros(tot, dtype=np.uint8)
    sc = random_scalars(tot, g.limbs, bits, seed)
    for p, k in enumerate(sizes):
        mix_instance(g, rows, inf, sc, int(offs[p]), k)
    if tot:
        if top_at is None:
            p = int(np.argmax(sizes))
            top_at = int(offs[p]) + (4 if sizes[p] >= 8 else sizes[p] - 1)
        set_scalar(sc, top_at, (1 << bits) - 1)
        inf[top_at] = 0
    return Call(group, rows, inf, sc, offs)


def pack_instance(group, points, scalars):
    """a hand-built instance in row form: (rows, inf, scalars)"""
    g = GROUPS[group]
    rows, inf = g.pack(points)
    return rows, inf, co.ints_to_limbs(scalars, g.limbs)


def concat_call(group, instances):
    """instances [(rows, inf, scalars)] -> Call"""
    g = GROUPS[group]
    offs = np.concatenate([[0], np.cumsum([r.shape[0] for r, _, _ in instances])]).astype(np.uint32)
    rows = np.concatenate([np.asarray(r, dtype=np.uint64).reshape(-1, g.rows) for r, _, _ in instances] + [np.zeros((0, g.rows), dtype=np.uint64)])
    inf = np.concatenate([np.asarray(i, dtype=np.uint8) for _, i, _ in instances] + [np.zeros(0, dtype=np.uint8)])
    sc = np.concatenate([np.asarray(s, dtype=np.uint64).reshape(-1, g.limbs) for _, _, s in instances] + [np.zeros((0, g.limbs), dtype=np.uint64)])
    return Call(group, rows, inf, sc, offs)


def cancelling_filler(group, table, k, bits, seed):
    """k rows (k even) whose sum is the identity BUCKET BY BUCKET: k / 2 distinct points of `table`, each followed by its negative under
    the same scalar below 2^bits - so an instance made of a builder's rows and this filler has the builder's window sums"""
    g = GROUPS[group]
    assert k % 2 == 0
    rows = np.empty((k, g.rows), dtype=np.uint64)
    rows[0::2] = table[:k // 2]
    rows[1::2] = g.neg_rows(table[:k // 2])
    sc = np.repeat(random_scalars(k // 2, g.limbs, bits, seed), 2, axis=0)
    return rows, np.zeros(k, dtype=np.uint8), sc


def clear_from(sc, bit):
    """a copy of the scalars with every bit from `bit` up cleared"""
    out = sc.copy()
    j, r = divmod(bit, 64)
    if j < out.shape[1]:
        out[:, j] &= np.uint64((1 << r) - 1)
        out[:, j + 1:] = 0
    return out
