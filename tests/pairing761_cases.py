"""Inputs for the BW6-761 pairing tests, every product with a verdict known BY CONSTRUCTION (no GPU import at module level).

Points.  A = synthetic.BW6_G1_POINT, B = synthetic.BW6_G2_POINT (alpha_g1 / beta_g2 of the reference's Groth16 key, both r-torsion);
k_i = splitmix64_at(seed, i) | 1, the scalar the library's point generator uses; P_i = k_i A, Q_i = k_i B.  Two routes to the same rows for
the same (seed, n): python_points (the Python oracle's scalar multiplication) and device_points (the generator kernel); the GPU tests compare
a sample of the second with the first before they rely on it.

Products.  With g = e(A, B), a generator of the order-r subgroup of GT, every product below is g^E for an exponent E that is known:
  couple(i)        e(P_i, B) e(-A, Q_i)            E = k_i - k_i = 0                                    -> 1
  mismatch(i, j)   e(P_i, B) e(-A, Q_j), j != i    E = k_i - k_j, 0 < |E| < 2^64                        -> not 1
  unrelated        e(P_a, Q_b) ...  (c pairs)      E = sum k_a k_b, 0 < E < c 2^128 < r (377 bits)      -> not 1
  half a couple    e(P_i, B) with its partner switched off by an infinity flag: E = k_i                 -> not 1
and a pair switched off by inf1 or inf2 contributes 1, so products of flagged pairs only and empty products are 1.  A product never
mixes a mismatch with an unrelated pair (E could then cancel in principle), so every verdict is exact, not "with high probability"."""
import numpy as np
from oracle.py import ecc
from oracle import cpu_oracle as co
from tests import helpers as H

MAX_PAIRS = 9          # pair counts of the ragged batches: 0 ... 9
VARIANTS = ("accept", "mismatch", "extra_live", "unrelated", "all_off", "half_off")


class Curve:
    """what binds the cases to a curve: the row widths, the generators A / B and their groups, the packers, the library's generator
    kernel groups and the two oracle calls.  Everything else in this module is curve-independent (tests/pairing377_cases.py binds BLS12-377)."""

    def __init__(self, name, w1, w2, q, E1, E2, generators, pack1, pack2, device_groups, gt, miller):
        self.name, self.w1, self.w2, self.q, self.E1, self.E2 = name, w1, w2, q, E1, E2
        self.generators, self.pack1, self.pack2, self.device_groups, self.gt, self.miller = generators, pack1, pack2, device_groups, gt, miller

    def python_rows(self, seed, indices):
        """rows of P_i and Q_i for the given i, by the Python oracle's scalar multiplication"""
        A, B = self.generators()
        g1, _ = self.pack1([self.E1.mul(A, scalar(seed, i)) for i in indices])
        g2, _ = self.pack2([self.E2.mul(B, scalar(seed, i)) for i in indices])
        return g1, g2

    def python_points(self, n, seed):
        return Points(*self.python_rows(seed, range(n)), seed, self)

    def device_points(self, n, seed):
        """the same rows from the library's generator kernel (needs the GPU)"""
        from celo_bls_snark_rs_amd import synthetic as syn
        P = syn.device_points(self.device_groups[0], n, seed).view(n, self.w1).cpu().numpy().view(np.uint64)
        Q = syn.device_points(self.device_groups[1], n, seed).view(n, self.w2).cpu().numpy().view(np.uint64)
        return Points(P, Q, seed, self)

    def neg_g1_rows(self, rows):
        """the rows of -P for G1 rows of P (Montgomery limbs: -(y R) = q - y R); a zero row stays zero"""
        rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, self.w1)
        n = self.w1 // 2
        y = co.limbs_to_ints(rows[:, n:], n)
        out = rows.copy()
        out[:, n:] = co.ints_to_limbs([(self.q - v) % self.q for v in y], n)
        return out


def generators():
    from celo_bls_snark_rs_amd import synthetic as syn        # (imports torch: kept out of module level)
    return syn.BW6_G1_POINT, syn.BW6_G2_POINT


def _pack_761(points):
    return co.pack_761(points)


CURVE = Curve("bw6_761", 24, 24, ecc.Q761, ecc.E1_761, ecc.E2_761, generators, _pack_761, _pack_761, ("bw6_761_g1", "bw6_761_g2"),
              lambda *a: co.pairing_product_761(*a), lambda *a: co.miller_loop_761(*a))


def scalar(seed, i):
    return H.splitmix64_at(seed, i) | 1


class Points:
    """P (n, w1), Q (n, w2): arkworks Montgomery rows of P_i, Q_i; table1 / table2 add the fixed rows A, -A, B, an all-zero row (what
    the packers write for a point at infinity) and any rows added later (the reference vector's)."""

    def __init__(self, P, Q, seed, curve=None):
        self.curve = curve = CURVE if curve is None else curve
        A, B = curve.generators()
        self.n, self.seed = P.shape[0], seed
        fixed1, _ = curve.pack1([A, curve.E1.neg(A), None])
        fixed2, _ = curve.pack2([B, None])
        self.table1 = np.concatenate([np.ascontiguousarray(P, dtype=np.uint64).reshape(-1, curve.w1), fixed1])
        self.table2 = np.concatenate([np.ascontiguousarray(Q, dtype=np.uint64).reshape(-1, curve.w2), fixed2])
        self.A, self.NEG_A, self.ZERO1 = self.n, self.n + 1, self.n + 2
        self.B, self.ZERO2 = self.n, self.n + 1

    @property
    def P(self):
        return self.table1[:self.n]

    @property
    def Q(self):
        return self.table2[:self.n]

    def with_rows(self, g1rows, g2rows):
        """a COPY of these points with rows (a product of fixed points) appended to both tables, and the (index in table1, index in
        table2) of the first appended row; the points a fixture shares stay as they are"""
        import copy
        q = copy.copy(self)
        at = (self.table1.shape[0], self.table2.shape[0])
        q.table1 = np.concatenate([self.table1, np.asarray(g1rows, dtype=np.uint64).reshape(-1, self.curve.w1)])
        q.table2 = np.concatenate([self.table2, np.asarray(g2rows, dtype=np.uint64).reshape(-1, self.curve.w2)])
        return q, at


def python_rows(seed, indices):
    return CURVE.python_rows(seed, indices)


def python_points(n, seed):
    return CURVE.python_points(n, seed)


def device_points(n, seed):
    return CURVE.device_points(n, seed)


class Spec:
    """one product: rows of table1 / table2 per pair, the two flag lists, the verdict, and what it was built as"""

    def __init__(self, kind):
        self.i1, self.i2, self.f1, self.f2, self.kind, self.expect = [], [], [], [], kind, None

    def pair(self, r1, r2, off=0):
        self.i1.append(r1); self.i2.append(r2); self.f1.append(1 if off == 1 else 0); self.f2.append(1 if off == 2 else 0)

    def __len__(self):
        return len(self.i1)

    def permute(self, order):
        for name in ("i1", "i2", "f1", "f2"):
            v = getattr(self, name)
            setattr(self, name, [v[j] for j in order])


def _off(pts, s, i, j, which, keep_rows):
    """a pair switched off through inf1 (which = 1) or inf2 (2); the flagged point's row is zeros, or - keep_rows - a stale valid point"""
    r1 = i if (keep_rows or which == 2) else pts.ZERO1
    r2 = j if (keep_rows or which == 1) else pts.ZERO2
    s.pair(r1, r2, which)


def resolve_variant(c, variant):
    """the variant a product of c pairs is built as: one that the count cannot carry is replaced, and Spec.kind names the result"""
    if c == 0:
        return "empty"
    if variant == "mismatch" and c < 2:
        return "unrelated"                  # no couple to give a foreign Q
    if variant == "half_off" and c < 2:
        return "all_off"
    if variant == "extra_live" and c % 2 == 0:
        return "half_off"                   # no odd pair out: half a couple switched off instead (not 1 either)
    return variant


def flag_defaults(base, c):
    """what product() takes from the base index when the caller does not say: which flag array (1 = inf1, 2 = inf2, in turn), whether the
    flagged point keeps a stale valid row (or is zeros, as pack_761 writes infinity), and the rotation of the pairs - so that over a batch
    with consecutive bases both arrays, both row kinds and every position occur"""
    return {"which": 1 + ((base // 2) & 1), "keep_rows": bool((base // 4) & 1), "rot": (base // 3) % max(c, 1)}


def product(pts, c, variant, base, flag_pos=None, which=None, keep_rows=None):
    """A product of c pairs over the point indices base, base + 1, ... (at most c + 1 of them), built as resolve_variant(c, variant).
    flag_pos: the position of the `special` pair (the flagged one, else the foreign-Q pair, else the live odd pair out); which: 1 / 2 =
    flags go through inf1 / inf2; keep_rows: flagged points keep a valid row.  Defaults: flag_defaults(base, c)."""
    ix = lambda t: (base + t) % pts.n
    variant = resolve_variant(c, variant)
    s = Spec(variant)
    if c == 0:
        s.expect = 1
        return s
    d = flag_defaults(base, c)
    which = d["which"] if which is None else which
    keep = d["keep_rows"] if keep_rows is None else keep_rows
    couples, extra = c // 2, c % 2
    if variant == "unrelated":
        for t in range(c):
            s.pair(ix(t), ix(t + 1))
        s.expect = 0
    elif variant == "all_off":
        for t in range(c):
            _off(pts, s, ix(t), ix(t + 1), 1 + ((which + t) & 1), keep)       # inf1 and inf2 alternate inside the product
        s.expect = 1
    else:
        for t in range(couples):
            j = ix(couples) if (variant == "mismatch" and t == 0) else ix(t)      # couple 0 takes a foreign Q
            s.pair(ix(t), pts.B)
            s.pair(pts.NEG_A, j)
        if variant == "half_off":                  # the second pair of couple 0 is switched off: e(P_i, B) remains
            s.f1[1], s.f2[1] = (1, 0) if which == 1 else (0, 1)
        if extra:
            if variant == "extra_live":
                s.pair(ix(couples), ix(couples + 1))
            else:
                _off(pts, s, ix(couples), ix(couples + 1), which, keep)
        s.expect = 1 if variant == "accept" else 0
        # pair order inside a product does not matter to its value: rotate so that the special pair sits at flag_pos
        special = c - 1 if extra else 1
        rot = d["rot"] if flag_pos is None else (flag_pos - special) % c
        s.permute([(t - rot) % c for t in range(c)])
    return s


def fixed_product(at, k, expect, kind):
    """a product over k consecutive appended rows (Points.with_rows)"""
    s = Spec(kind)
    for t in range(k):
        s.pair(at[0] + t, at[1] + t)
    s.expect = expect
    return s


def layout(pts, specs):
    """-> g1 (k, w1), i1 (k), g2 (k, w2), i2 (k), offsets (m + 1) uint32, expect (m) uint8"""
    i1 = np.array([r for s in specs for r in s.i1], dtype=np.int64)
    i2 = np.array([r for s in specs for r in s.i2], dtype=np.int64)
    f1 = np.array([r for s in specs for r in s.f1], dtype=np.uint8)
    f2 = np.array([r for s in specs for r in s.f2], dtype=np.uint8)
    offs = np.zeros(len(specs) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(s) for s in specs])
    g1 = pts.table1[i1] if i1.size else np.zeros((0, pts.curve.w1), dtype=np.uint64)
    g2 = pts.table2[i2] if i2.size else np.zeros((0, pts.curve.w2), dtype=np.uint64)
    return np.ascontiguousarray(g1), f1, np.ascontiguousarray(g2), f2, offs, np.array([s.expect for s in specs], dtype=np.uint8)


def has_flag(s):
    return any(s.f1) or any(s.f2)


def ragged_specs(pts, counts, seed, first=0, flag_share=None, variants=VARIANTS, build=None):
    """one product per entry of counts (0 ... MAX_PAIRS pairs each), variants drawn by a seeded generator, every product over point
    indices of its own (a stride of max(counts) + 1).  flag_share: keep only about that share of the products that came out with a flag
    and rebuild the others as a flagless variant of the same count (for calls whose flagged products must all go to the oracle).
    variants / build: another list of variants and the function that builds them (default: VARIANTS, product)."""
    build = product if build is None else build
    rng = np.random.default_rng(seed)
    stride = max(max(counts), 1) + 1
    assert max(counts) <= MAX_PAIRS and first + stride * len(counts) <= pts.n, "not enough points for distinct products"
    draw = rng.integers(0, len(variants), size=len(counts))
    keep = rng.random(len(counts))
    specs = []
    for p, (c, v) in enumerate(zip(counts, draw)):
        s = build(pts, int(c), variants[int(v)], first + p * stride)
        if flag_share is not None and has_flag(s) and keep[p] >= flag_share:
            flagless = ("extra_live", "unrelated") if c % 2 else ("accept", "mismatch", "unrelated")
            s = build(pts, int(c), flagless[int(v) % len(flagless)], first + p * stride)
            assert not has_flag(s)
        specs.append(s)
    return specs


def ragged_batch(pts, counts, seed, first=0):
    """g1, i1, g2, i2, offsets, expect for a ragged batch with the given pair counts"""
    return layout(pts, ragged_specs(pts, counts, seed, first))


def reference_products(golden):
    """the reference's own Groth16 check (crates/bls-snark-sys/src/snark/mod.rs:52-119) as four pairs, and its two tampered forms of
    tests/test_groth16_gpu.py (a flipped bit of a public input; the proof's C doubled): [(g1 rows, g2 rows, verdict, name)]"""
    from oracle.py import epoch as ep
    vk, pr, inputs = H.groth16_setup(golden)
    out = []
    for name, proof, inp, want in (("reference", pr, inputs, 1), ("reference_bad_input", pr, [inputs[0] ^ 1, inputs[1]], 0),
                                   ("reference_bad_c", dict(pr, c=ecc.E1_761.add(pr["c"], pr["c"])), inputs, 0)):
        pairs = ep.groth16_pairs(vk, proof, inp)
        out.append((co.pack_761([p for p, _ in pairs])[0], co.pack_761([q for _, q in pairs])[0], want, name))
    return out


def slice_of(batch, p):
    """the arrays of product p alone"""
    g1, i1, g2, i2, offs = batch[:5]
    lo, hi = int(offs[p]), int(offs[p + 1])
    return g1[lo:hi], (None if i1 is None else i1[lo:hi]), g2[lo:hi], (None if i2 is None else i2[lo:hi])


def oracle_gt(batch, p, curve=CURVE):
    return curve.gt(*slice_of(batch, p))


def oracle_miller(batch, p, curve=CURVE):
    return curve.miller(*slice_of(batch, p))
