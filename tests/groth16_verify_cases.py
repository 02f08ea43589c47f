"""Groth16 proofs over BW6-761 that carry their verdict BY CONSTRUCTION - no circuit needed (no GPU import at module level).

Key.  Scalars a, b, g, d, u_0 .. u_n; alpha = a G1, beta = b G2, gamma = g G2, delta = d G2, gamma_abc[j] = u_j G1, with G1 / G2 the
alpha_g1 / beta_g2 of the reference's own verifying key (tests/golden/reference_vectors.json), both of prime order r.

Proof.  A = s G1, B = t G2, C = c G1.  With e = e(G1, G2), a generator of the order-r subgroup of GT, the verifier's product
  e(A, B) e(acc, -gamma) e(C, -delta) e(-alpha, beta),   acc = gamma_abc[0] + sum_j x_j gamma_abc[j + 1]
is e^E with  E = s t - g (u_0 + sum_j x_j u_{j+1}) - c d - a b  (mod r): the proof verifies iff E == 0 - and every input is below r, which is
the library's rule (ark cannot represent another value).  c = (s t - a b - g (u_0 + sum x_j u_{j+1})) / d makes E zero; every other case
class moves one term.  A point at infinity is the scalar 0.  Point multiples come from the C++ oracle (orc_mul_bw6_761); the verdicts are
checked against the oracle's own product of the four pairs in tests/test_groth16_verify_cases.py.

The combined check's exponents are restated here (exponents_ref): r_i = 2^127 | low 127 bits of the first 16 bytes of ChaCha20 block i."""
import ctypes as C
import json
import os
import numpy as np
from oracle.py import ecc
from oracle.py import epoch as ep
from oracle import cpu_oracle as co

R = ecc.R761
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_ONES = (1 << 376) - 1            # below r (377 bits): every window's digit is all ones, the carry runs through all of them
EDGE_INPUTS = (0, 1, R - 1, ALL_ONES, ALL_ONES - 1, (1 << 376) - (1 << 188))
# one special proof among valid ones: class -> verdict of the special proof
CLASSES = ("valid", "rerandomised", "wrong_input", "wrong_a", "wrong_b", "wrong_c", "inf_a", "inf_b", "inf_c", "inf_a_accept", "input_r", "input_r1",
           "edge_0", "edge_1", "edge_rm1", "edge_ones")
INPUT_CLASSES = ("wrong_input", "input_r", "input_r1", "edge_0", "edge_1", "edge_rm1", "edge_ones")

_GENS = None


def generators():
    """(G1 row, G2 row): 24 u64 each, Montgomery limbs"""
    global _GENS
    if _GENS is None:
        with open(os.path.join(ROOT, "tests", "golden", "reference_vectors.json")) as f:
            vk = ep.parse_vk(bytes.fromhex(json.load(f)["groth16_bw6_761"]["vk"]))
        _GENS = (co.pack_761([vk["alpha_g1"]])[0][0].copy(), co.pack_761([vk["beta_g2"]])[0][0].copy())
    return _GENS


def mul_rows(gen_row, scalars):
    """rows (n, 24) and identity bytes of k G for every k (reduced mod r) by the C++ oracle; the identity is a zero row"""
    n = len(scalars)
    k6 = co.ints_to_limbs([int(k) % R for k in scalars], 6)
    jac = np.zeros((n, 36), dtype=np.uint64)
    g = np.ascontiguousarray(gen_row, dtype=np.uint64)
    for i in range(n):
        assert co.lib().orc_mul_bw6_761(co._p(g), co._p(k6[i]), co._p(jac[i])) == 0
    xy = np.zeros((n, 24), dtype=np.uint64)
    inf = np.zeros(n, dtype=np.uint8)
    if n:
        assert co.lib().orc_normalize_bw6_761(co._p(jac), C.c_size_t(n), co._p(xy), co._p(inf)) == 0
    xy[inf != 0] = 0
    return xy, inf


class Key:
    """a verifying key with n_in public inputs from seeded scalars; .rows: alpha, beta, gamma, delta (24 u64 each), .abc (n_in + 1, 24)"""

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

    def serialize(self):
        """VerifyingKey::serialize bytes of this key (compressed)"""
        from_rows = lambda rows: [tuple(co.from_mont(np.asarray(r).reshape(2, 12), ecc.Q761)) for r in rows]
        out = ecc.ser_point(ecc.E1_761, from_rows([self.alpha])[0])
        for r in (self.beta, self.gamma, self.delta):
            out += ecc.ser_point(ecc.E2_761, from_rows([r])[0])
        out += len(self.abc).to_bytes(8, "little")
        for p in from_rows(self.abc):
            out += ecc.ser_point(ecc.E1_761, p)
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


class Batch:
    """rows of m proofs: a, b, c (m, 24) with identity bytes, inputs (m, n_in, 6) canonical u64, expect (m)"""

    def __init__(self, key, proofs, mul=None):
        """mul(generator row, scalars, on_g2) -> rows, identity bytes: another source of the multiples (default: the C++ oracle)"""
        G1, G2 = generators()
        mul = (lambda g, k, on_g2: mul_rows(g, k)) if mul is None else mul
        self.key, self.proofs, self.m = key, proofs, len(proofs)
        self.a, self.a_inf = mul(G1, [p.s for p in proofs], False)
        self.b, self.b_inf = mul(G2, [p.t for p in proofs], True)
        self.c, self.c_inf = mul(G1, [p.c for p in proofs], False)
        self.inputs = co.ints_to_limbs([v for p in proofs for v in p.x], 6).reshape(self.m, key.n_in, 6) if key.n_in else np.zeros((self.m, 0, 6), dtype=np.uint64)
        self.expect = np.array([p.expect(key) for p in proofs], dtype=np.uint8)

    def serialize(self):
        """m x 288 B: Proof::serialize of every proof"""
        pt = lambda row, inf: None if inf else tuple(co.from_mont(np.asarray(row).reshape(2, 12), ecc.Q761))
        out = b""
        for i in range(self.m):
            out += ecc.ser_point(ecc.E1_761, pt(self.a[i], self.a_inf[i])) + ecc.ser_point(ecc.E2_761, pt(self.b[i], self.b_inf[i])) + \
                ecc.ser_point(ecc.E1_761, pt(self.c[i], self.c_inf[i]))
        return out


def batch_with(key, m, specials, seed, mul=None):
    """m proofs, valid except the given {position: Proof}"""
    rng = ecc.SplitMix64(seed)
    return Batch(key, [specials[i] if i in specials else valid_proof(key, rng) for i in range(m)], mul)


def take(batch, idx):
    """the proofs idx of a batch as a batch (rows gathered, nothing recomputed)"""
    import copy
    idx = np.asarray(idx, dtype=np.int64)
    q = copy.copy(batch)
    q.proofs, q.m = [batch.proofs[i] for i in idx], len(idx)
    for name in ("a", "a_inf", "b", "b_inf", "c", "c_inf", "inputs", "expect"):
        setattr(q, name, np.ascontiguousarray(getattr(batch, name)[idx]))
    return q


def neg_row(row):
    out = np.array(row, dtype=np.uint64).reshape(24).copy()
    if out.any():
        y = co.limbs_to_ints(out[12:], 12)[0]
        out[12:] = co.ints_to_limbs([(ecc.Q761 - y) % ecc.Q761], 12)[0]
    return out


def acc_rows(key, inputs):
    """the oracle's acc_i = abc_0 + sum_j x_ij abc_j (inputs reduced mod r: the oracle's MSM takes canonical scalars) -> rows, inf"""
    m = inputs.shape[0]
    jac = np.zeros((m, 36), dtype=np.uint64)
    for i in range(m):
        sc = np.concatenate([co.ints_to_limbs([1], 6), co.ints_to_limbs([v % R for v in co.limbs_to_ints(inputs[i], 6)], 6).reshape(-1, 6)])
        jac[i] = co.msm("bw6_761_g1", key.abc, None, sc)
    xy = np.zeros((m, 24), dtype=np.uint64)
    inf = np.zeros(m, dtype=np.uint8)
    assert co.lib().orc_normalize_bw6_761(co._p(jac), C.c_size_t(m), co._p(xy), co._p(inf)) == 0
    xy[inf != 0] = 0
    return xy, inf


def oracle_verdict(batch, i):
    """the oracle's product over the four pairs of proof i (and the library's input rule)"""
    key = batch.key
    acc, acc_inf = acc_rows(key, batch.inputs[i:i + 1])
    g1 = np.stack([batch.a[i], acc[0], batch.c[i], neg_row(key.alpha)])
    g2 = np.stack([batch.b[i], neg_row(key.gamma), neg_row(key.delta), key.beta])
    i1 = np.array([batch.a_inf[i], acc_inf[0], batch.c_inf[i], 0], dtype=np.uint8)
    i2 = np.array([batch.b_inf[i], 0, 0, 0], dtype=np.uint8)
    in_range = all(v < R for v in co.limbs_to_ints(batch.inputs[i], 6)) if key.n_in else True
    return 1 if co.pairing_product_761(g1, i1, g2, i2)[1] and in_range else 0


# ---- the exponent rule, restated
def _rotl(x, n):
    return ((x << n) | (x >> (32 - n))) & 0xFFFFFFFF


def chacha20_block(key8, counter, tail=(0, 0)):
    """RFC 7539 block function, 64-bit block counter, zero nonce (tail: the last two state words, for the RFC's own vector): 16 words"""
    s = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574] + [int(k) for k in key8] + [counter & 0xFFFFFFFF, counter >> 32, tail[0], tail[1]]
    w = list(s)

    def qr(a, b, c, d):
        w[a] = (w[a] + w[b]) & 0xFFFFFFFF; w[d] = _rotl(w[d] ^ w[a], 16)
        w[c] = (w[c] + w[d]) & 0xFFFFFFFF; w[b] = _rotl(w[b] ^ w[c], 12)
        w[a] = (w[a] + w[b]) & 0xFFFFFFFF; w[d] = _rotl(w[d] ^ w[a], 8)
        w[c] = (w[c] + w[d]) & 0xFFFFFFFF; w[b] = _rotl(w[b] ^ w[c], 7)

    for _ in range(10):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
    return [(a + b) & 0xFFFFFFFF for a, b in zip(w, s)]


def exponents_ref(key8, m):
    """r_i = 2^127 | (the low 127 bits of the first 16 bytes of block i)"""
    out = []
    for i in range(m):
        b = chacha20_block(key8, i)
        v = b[0] | (b[1] << 32) | (b[2] << 64) | (b[3] << 96)
        out.append((1 << 127) | (v & ((1 << 127) - 1)))
    return out


def oracle_combined(batch, exps):
    """the combined equation on the oracle: prod e(r_i A_i, B_i) e(sum r_i acc_i, -gamma) e(sum r_i C_i, -delta) e(-(sum r_i) alpha, beta) == 1"""
    key, m = batch.key, batch.m
    ra = np.zeros((m, 24), dtype=np.uint64)
    ra_inf = np.zeros(m, dtype=np.uint8)
    for i in range(m):
        if not batch.a_inf[i]:
            ra[i], ra_inf[i] = (x[0] for x in mul_rows(batch.a[i], [exps[i]]))
        else:
            ra_inf[i] = 1
    acc, acc_inf = acc_rows(key, batch.inputs)
    sc = co.ints_to_limbs(exps, 6)
    jac = np.stack([co.msm("bw6_761_g1", acc, acc_inf, sc), co.msm("bw6_761_g1", batch.c, batch.c_inf, sc)])
    tail = np.zeros((2, 24), dtype=np.uint64)
    tinf = np.zeros(2, dtype=np.uint8)
    assert co.lib().orc_normalize_bw6_761(co._p(jac), C.c_size_t(2), co._p(tail), co._p(tinf)) == 0
    tail[tinf != 0] = 0
    sa, sa_inf = mul_rows(neg_row(key.alpha), [sum(exps)])
    g1 = np.concatenate([ra, tail, sa])
    g2 = np.concatenate([batch.b, np.stack([neg_row(key.gamma), neg_row(key.delta), key.beta])])
    i1 = np.concatenate([ra_inf, tinf, sa_inf]).astype(np.uint8)
    i2 = np.concatenate([batch.b_inf, np.zeros(3, dtype=np.uint8)]).astype(np.uint8)
    return 1 if co.pairing_product_761(g1, i1, g2, i2)[1] else 0
