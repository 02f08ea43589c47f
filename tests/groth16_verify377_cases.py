"""Groth16 proofs over BLS12-377 that carry their verdict BY CONSTRUCTION: tests/groth16_verify_cases.py bound to the curve of the hash-helper
proof (no GPU import at module level).

Key.  Scalars a, b, g, d, u_0 .. u_n; alpha = a G1, beta = b G2, gamma = g G2, delta = d G2, gamma_abc[j] = u_j G1, with G1 / G2 the
generators of the oracle (ecc.G1_377 / ecc.G2_377), both of prime order r (253 bits).

Proof.  A = s G1, B = t G2, C = c G1.  With e = e(G1, G2) the verifier's product
  e(A, B) e(acc, -gamma) e(C, -delta) e(-alpha, beta),   acc = gamma_abc[0] + sum_j x_j gamma_abc[j + 1]
is e^E with  E = s t - g (u_0 + sum_j x_j u_{j+1}) - c d - a b  (mod r): the proof verifies iff E == 0 and every input is below r.
Point multiples come from the C++ oracle (orc_mul_bls12_377_g1 / _g2); the verdicts are checked against the oracle's own product of the
four pairs (co.pairing_product_377) in tests/test_groth16_verify377_cases.py.

Rows: G1 12 u64, G2 24 u64 (c0 then c1 per coordinate), arkworks Montgomery limbs; inputs 4 u64, canonical.  The exponent rule, the ChaCha20
block function and the list of case classes do not depend on the curve and are the existing module's."""
import copy
import ctypes as C
import os
import numpy as np
from oracle.py import ecc
from oracle import cpu_oracle as co
from tests.groth16_verify_cases import CLASSES, INPUT_CLASSES, chacha20_block, exponents_ref  # noqa: F401  (re-exported)

R = ecc.R377
Q = ecc.Q377
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W1, W2, N64 = 12, 24, 4                 # u64 of a G1 row, of a G2 row, of an input
ALL_ONES = (1 << 252) - 1              # below r (its top set bit is 2^252): every window's digit is all ones, the carry runs through all of them
assert (1 << 252) <= R < (1 << 253) and ALL_ONES < R
EDGE_INPUTS = (0, 1, R - 1, ALL_ONES, ALL_ONES - 1, (1 << 252) - (1 << 126))
TABLE_BUDGET = 64 << 20
ENTRY_BYTES = 2 * 16 * 4               # an affine table entry: two coordinates of 14 limbs in the field's stored form of 16 words

_GENS = None


def fb_windows(bits, c):
    """csrc/fixed_base.h fb_windows: signed c-bit digits of a scalar of `bits` bits"""
    return (bits + 1 + c - 1) // c


def window_bits(n_in):
    """csrc/groth16_verify.h g16_window_bits restated for this curve: the widest of 10 .. 4 bits whose tables fit 64 MiB"""
    c = 10
    while c > 4 and n_in * fb_windows(253, c) * (1 << (c - 1)) * ENTRY_BYTES > TABLE_BUDGET:
        c -= 1
    return c


def generators():
    """(G1 row of 12 u64, G2 row of 24 u64), Montgomery limbs"""
    global _GENS
    if _GENS is None:
        _GENS = (co.pack_g1_377([ecc.G1_377])[0][0].copy(), co.pack_g2_377([ecc.G2_377])[0][0].copy())
    return _GENS


def mul_rows(gen_row, scalars):
    """rows and identity bytes of k G for every k (reduced mod r) by the C++ oracle; the group is read off the row's width"""
    g = np.ascontiguousarray(gen_row, dtype=np.uint64).reshape(-1)
    on_g2 = g.size == W2
    n = len(scalars)
    k4 = co.ints_to_limbs([int(k) % R for k in scalars], N64)
    jac = np.zeros((n, 36 if on_g2 else 18), dtype=np.uint64)
    fn = co.lib().orc_mul_bls12_377_g2 if on_g2 else co.lib().orc_mul_bls12_377_g1
    for i in range(n):
        assert fn(co._p(g), co._p(k4[i]), co._p(jac[i])) == 0
    return co.normalize("g2_377" if on_g2 else "g1_377", jac)


def row_point(row, inf=0):
    """a row -> the python point ecc takes (None: the identity)"""
    row = np.asarray(row, dtype=np.uint64).reshape(-1)
    if inf or not row.any():
        return None
    v = co.from_mont(row.reshape(-1, 6), Q)
    return (v[0], v[1]) if row.size == W1 else ((v[0], v[1]), (v[2], v[3]))


def ser_row(row, inf=0):
    row = np.asarray(row).reshape(-1)
    return ecc.ser_point(ecc.E1_377 if row.size == W1 else ecc.E2_377, row_point(row, inf))


class Key:
    """a verifying key with n_in public inputs from seeded scalars; .alpha (12 u64), .beta / .gamma / .delta (24), .abc (n_in + 1, 12)"""

    def __init__(self, n_in, seed):
        rng = ecc.SplitMix64(seed)
        nz = lambda: 1 + ecc.random_scalar(rng, R - 1)
        self.n_in = n_in
        self.a, self.b, self.g, self.d = nz(), nz(), nz(), nz()
        self.u = [nz() for _ in range(n_in + 1)]
        G1, G2 = generators()
        self.alpha = mul_rows(G1, [self.a])[0][0]
        g2 = mul_rows(G2, [self.b, self.g, self.d])[0]
        self.beta, self.gamma, self.delta = g2[0], g2[1], g2[2]
        self.abc = mul_rows(G1, self.u)[0]

    def acc_scalar(self, x):
        return (self.u[0] + sum(xj * uj for xj, uj in zip(x, self.u[1:]))) % R

    def c_for(self, s, t, x):
        return (s * t - self.a * self.b - self.g * self.acc_scalar(x)) * pow(self.d, -1, R) % R

    def residual(self, s, t, c, x):
        return (s * t - self.g * self.acc_scalar(x) - c * self.d - self.a * self.b) % R

    def serialize(self, abc=None):
        """VerifyingKey::serialize bytes of this key (compressed); abc: other gamma_abc rows"""
        abc = self.abc if abc is None else abc
        out = ser_row(self.alpha) + ser_row(self.beta) + ser_row(self.gamma) + ser_row(self.delta)
        out += len(abc).to_bytes(8, "little")
        for r in abc:
            out += ser_row(r)
        return out


class Proof:
    """scalars of A, B, C (0 = the point at infinity), the inputs, what it was built as"""

    def __init__(self, s, t, c, x, kind="valid"):
        self.s, self.t, self.c, self.x, self.kind = s % R, t % R, c % R, list(x), kind

    def expect(self, key):
        return 1 if all(0 <= v < R for v in self.x) and key.residual(self.s, self.t, self.c, self.x) == 0 else 0


def valid_proof(key, rng, x=None, kind="valid"):
    x = [ecc.random_scalar(rng, R) for _ in range(key.n_in)] if x is None else list(x)
    s, t = 1 + ecc.random_scalar(rng, R - 1), 1 + ecc.random_scalar(rng, R - 1)
    return Proof(s, t, key.c_for(s, t, x), x, kind)


def special_proof(key, rng, kind):
    """one proof of the given class (CLASSES)"""
    p = valid_proof(key, rng, kind=kind)
    if kind == "rerandomised":                       # (k A, k^-1 B, C): another proof of the same statement
        k = 2 + ecc.random_scalar(rng, R - 2)
        p.s, p.t = p.s * k % R, p.t * pow(k, -1, R) % R
    elif kind == "wrong_input":
        p.x[-1] = (p.x[-1] + 1) % R
    elif kind == "wrong_a":
        p.s = (p.s + 1) % R
    elif kind == "wrong_b":
        p.t = (p.t + 1) % R
    elif kind == "wrong_c":
        p.c = (p.c + 1) % R
    elif kind == "inf_a":
        p.s = 0
    elif kind == "inf_b":
        p.t = 0
    elif kind == "inf_c":
        p.c = 0
    elif kind == "inf_a_accept":                     # A at infinity and C chosen for it: e(A, B) = 1 and the other three pairs cancel
        p.s, p.c = 0, key.c_for(0, p.t, p.x)
    elif kind in ("input_r", "input_r1"):            # a valid proof for x mod r, presented with x + r: accepted only if the range test is dropped
        p = valid_proof(key, rng, x=[0 if kind == "input_r" else 1] + p.x[1:], kind=kind)
        p.x[0] += R
    elif kind.startswith("edge_"):
        v = {"edge_0": 0, "edge_1": 1, "edge_rm1": R - 1, "edge_ones": ALL_ONES}[kind]
        p = valid_proof(key, rng, x=[v] * key.n_in, kind=kind)
    return p


def classes_for(key):
    return [k for k in CLASSES if key.n_in or k not in INPUT_CLASSES]


def cancelling_pair(key, rng):
    """(C_1 + D, C_2 - D): each fails alone, their unweighted sum passes"""
    p, q = valid_proof(key, rng, kind="cancel"), valid_proof(key, rng, kind="cancel")
    dd = 1 + ecc.random_scalar(rng, R - 1)
    p.c, q.c = (p.c + dd) % R, (q.c - dd) % R
    return p, q


def swapped_pair(key, rng):
    """two valid proofs with their inputs exchanged (n_in >= 1)"""
    p, q = valid_proof(key, rng, kind="swapped"), valid_proof(key, rng, kind="swapped")
    p.x, q.x = q.x, p.x
    return p, q


def input_limbs(proofs, n_in):
    m = len(proofs)
    return co.ints_to_limbs([v for p in proofs for v in p.x], N64).reshape(m, n_in, N64) if n_in else np.zeros((m, 0, N64), dtype=np.uint64)


class Batch:
    """rows of m proofs: a, c (m, 12), b (m, 24) with identity bytes, inputs (m, n_in, 4) canonical u64, expect (m)"""

    def __init__(self, key, proofs, mul=None):
        """mul(generator row, scalars, on_g2) -> rows, identity bytes: another source of the multiples (default: the C++ oracle)"""
        G1, G2 = generators()
        mul = (lambda g, k, on_g2: mul_rows(g, k)) if mul is None else mul
        self.key, self.proofs, self.m = key, proofs, len(proofs)
        self.a, self.a_inf = mul(G1, [p.s for p in proofs], False)
        self.b, self.b_inf = mul(G2, [p.t for p in proofs], True)
        self.c, self.c_inf = mul(G1, [p.c for p in proofs], False)
        self.inputs = input_limbs(proofs, key.n_in)
        self.expect = np.array([p.expect(key) for p in proofs], dtype=np.uint8)

    def serialize(self):
        """m x 192 B: Proof::serialize of every proof"""
        return b"".join(ser_row(self.a[i], self.a_inf[i]) + ser_row(self.b[i], self.b_inf[i]) + ser_row(self.c[i], self.c_inf[i]) for i in range(self.m))


def batch_with(key, m, specials, seed, mul=None):
    """m proofs, valid except the given {position: Proof}"""
    rng = ecc.SplitMix64(seed)
    return Batch(key, [specials[i] if i in specials else valid_proof(key, rng) for i in range(m)], mul)


def take(batch, idx):
    """the proofs idx of a batch as a batch (rows gathered, nothing recomputed)"""
    idx = np.asarray(idx, dtype=np.int64)
    q = copy.copy(batch)
    q.proofs, q.m = [batch.proofs[i] for i in idx], len(idx)
    for name in ("a", "a_inf", "b", "b_inf", "c", "c_inf", "inputs", "expect"):
        setattr(q, name, np.ascontiguousarray(getattr(batch, name)[idx]))
    return q


def neg_row(row):
    """-P for a G1 or G2 row: every component of y negated"""
    out = np.array(row, dtype=np.uint64).reshape(-1).copy()
    if out.any():
        half = out.size // 2
        y = co.limbs_to_ints(out[half:], 6)
        out[half:] = co.ints_to_limbs([(Q - v) % Q for v in y], 6).reshape(-1)
    return out


def acc_rows(key, inputs):
    """the oracle's acc_i = abc_0 + sum_j x_ij abc_j (inputs reduced mod r: the oracle's MSM takes canonical scalars) -> rows, inf"""
    m = inputs.shape[0]
    jac = np.zeros((m, 18), dtype=np.uint64)
    for i in range(m):
        sc = np.concatenate([co.ints_to_limbs([1], N64), co.ints_to_limbs([v % R for v in co.limbs_to_ints(inputs[i], N64)], N64).reshape(-1, N64)])
        jac[i] = co.msm("bls12_377_g1", key.abc, None, sc)
    return co.normalize("g1_377", jac)


def oracle_verdict(batch, i):
    """the oracle's product over the four pairs of proof i (and the library's input rule)"""
    key = batch.key
    acc, acc_inf = acc_rows(key, batch.inputs[i:i + 1])
    g1 = np.stack([batch.a[i], acc[0], batch.c[i], neg_row(key.alpha)])
    g2 = np.stack([batch.b[i], neg_row(key.gamma), neg_row(key.delta), key.beta])
    i1 = np.array([batch.a_inf[i], acc_inf[0], batch.c_inf[i], 0], dtype=np.uint8)
    i2 = np.array([batch.b_inf[i], 0, 0, 0], dtype=np.uint8)
    in_range = all(v < R for v in co.limbs_to_ints(batch.inputs[i], N64)) if key.n_in else True
    return 1 if co.pairing_product_377(g1, i1, g2, i2)[1] and in_range else 0


def oracle_combined(batch, exps):
    """the combined equation on the oracle: prod e(r_i A_i, B_i) e(sum r_i acc_i, -gamma) e(sum r_i C_i, -delta) e(-(sum r_i) alpha, beta) == 1"""
    key, m = batch.key, batch.m
    ra = np.zeros((m, W1), dtype=np.uint64)
    ra_inf = np.zeros(m, dtype=np.uint8)
    for i in range(m):
        if not batch.a_inf[i]:
            ra[i], ra_inf[i] = (x[0] for x in mul_rows(batch.a[i], [exps[i]]))
        else:
            ra_inf[i] = 1
    acc, acc_inf = acc_rows(key, batch.inputs)
    sc = co.ints_to_limbs(exps, N64)
    tail, tinf = co.normalize("g1_377", np.stack([co.msm("bls12_377_g1", acc, acc_inf, sc), co.msm("bls12_377_g1", batch.c, batch.c_inf, sc)]))
    sa, sa_inf = mul_rows(neg_row(key.alpha), [sum(exps)])
    g1 = np.concatenate([ra, tail, sa])
    g2 = np.concatenate([batch.b, np.stack([neg_row(key.gamma), neg_row(key.delta), key.beta])])
    i1 = np.concatenate([ra_inf, tinf, sa_inf]).astype(np.uint8)
    i2 = np.concatenate([batch.b_inf, np.zeros(3, dtype=np.uint8)]).astype(np.uint8)
    return 1 if co.pairing_product_377(g1, i1, g2, i2)[1] else 0


# ---- damaged encodings for the serialized entries
def off_subgroup_point(on_g2, seed):
    """a point of the curve from a random x (random x until x^3 + b is a square): outside the prime-order subgroup, which is checked"""
    rng = ecc.SplitMix64(seed)
    E = ecc.E2_377 if on_g2 else ecc.E1_377
    while True:
        if on_g2:
            x = (ecc.random_scalar(rng, Q), ecc.random_scalar(rng, Q))
            y = ecc.F2_377.sqrt(ecc.F2_377.add(ecc.F2_377.mul(ecc.F2_377.mul(x, x), x), E.b))
        else:
            x = ecc.random_scalar(rng, Q)
            y = ecc.sqrt_fp((x * x * x + E.b) % Q, Q)
        if y is not None and E.on_curve((x, y)) and not E.in_subgroup((x, y)):
            return (x, y)


def non_residue_x(seed):
    """an x < q for which x^3 + 1 has no square root: no point of G1's curve has it"""
    rng = ecc.SplitMix64(seed)
    while True:
        x = ecc.random_scalar(rng, Q)
        if ecc.sqrt_fp((x * x * x + 1) % Q, Q) is None:
            return x
