"""The reference side of the hash-to-G2 tests (tests/test_hash_g2_host.py, tests/test_hash_g2_gpu.py): try-and-increment onto the twist
E'(Fq2) of BLS12-377 restated over the Python oracle - TryAndIncrement<H, G2> and TryAndIncrementCIP22<H, G2> of the reference
(crates/bls-crypto/src/hash_to_curve/try_and_increment.rs:63-140, try_and_increment_cip22.rs:75-135), the four modes of tests/hash_ref.py:

  direct           candidate c = xof(crh(c || extra || message), 96), the Blake2s CRH with 96 in its node offset
  tail             candidate c = xof(c || extra || inner, 96)
  composite        candidate c = xof(pedersen_crh(c || extra || message), 96)
  composite_cip22  inner = pedersen_crh(message) once, then the tail

A candidate is 96 XOF bytes: c0 = bytes 0..47, c1 = bytes 48..95, both masked to 377 bits; the flags are bits 7 (y sign) and 6 (infinity) of
byte 95 - as the XOF gives them, or with compat the sign flag copied from bit 1 of byte 95 first.  The point is multiplied by the cofactor
H2 = #E'(Fq2) / r, which is DERIVED here (twist_orders / derive_h2), not written down.

Two forms of the two expensive steps: the pure-Python ones (ecc.F2_377.sqrt, ecc.E2_377.mul) are the definition; the fast ones go through
the C++ oracle (co.decompress for the root, three co.msm calls for the 502-bit multiple) and are pinned to the definition by
tests/test_hash_g2_host.py.  No tests in this file; nothing here decides what is compared."""
import math
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _d in (os.path.dirname(_HERE), _HERE):
    if _d not in sys.path:
        sys.path.insert(0, _d)

from oracle.py import ecc, hashing as hs          # noqa: E402
from oracle.py import composite as comp           # noqa: E402
from oracle import cpu_oracle as co               # noqa: E402

MODES = ("direct", "tail", "composite", "composite_cip22")
MODE_INDEX = {"direct": 0, "tail": 1, "composite": 2, "composite_cip22": 3}      # the `mode` argument of hash_to_g2_one_bls12_377
XOF_BYTES = hs.hash_length(96)                    # 96: three Blake2s blocks
Q, R = ecc.Q377, ecc.R377
E2, F2 = ecc.E2_377, ecc.F2_377


# ---- the order of the twist and its cofactor
def twist_orders():
    """The six candidates for #E'(Fq2) of a sextic twist of E: y^2 = x^3 + 1 over Fq2.  E(Fq) has trace t = x + 1; over Fq2 the trace is
    t2 = t^2 - 2 q, and with 4 q^2 - t2^2 = 3 f^2 (discriminant -3) the twists have traces +-t2, +-(t2 + 3 f) / 2, +-(t2 - 3 f) / 2."""
    t = ecc.X + 1
    t2 = t * t - 2 * Q
    f2, rem = divmod(4 * Q * Q - t2 * t2, 3)
    f = math.isqrt(f2)
    assert rem == 0 and f * f == f2 and (t2 + 3 * f) % 2 == 0
    traces = [t2, -t2, (t2 + 3 * f) // 2, -(t2 + 3 * f) // 2, (t2 - 3 * f) // 2, -(t2 - 3 * f) // 2]
    return [Q * Q + 1 - tr for tr in traces]


def random_twist_point(rng):
    """a point of E'(Fq2) with random x: almost surely outside the r-torsion"""
    while True:
        x = (int.from_bytes(rand_bytes(rng, 48), "little") % Q, int.from_bytes(rand_bytes(rng, 48), "little") % Q)
        y = F2.sqrt(F2.add(F2.mul(F2.sqr(x), x), ecc.B2_377))
        if y is not None:
            return (x, y)


def derive_h2(rng=None):
    """(H2, the group order): the one candidate order that r divides and that kills a random twist point outside the r-torsion"""
    rng = np.random.default_rng(0x42) if rng is None else rng
    P = random_twist_point(rng)
    assert E2.mul(P, R) is not None
    good = [n for n in twist_orders() if n % R == 0 and E2.mul(P, n) is None]
    assert len(good) == 1, good
    return good[0] // R, good[0]


_H2 = None


def h2():
    global _H2
    if _H2 is None:
        _H2 = derive_h2()[0]
    return _H2


# ---- one candidate
def _masked(cand96, compat):
    """(masked 96 bytes, flags): the `compat` remap, the two flag bits, both halves cut to 377 bits"""
    b = bytearray(cand96)
    assert len(b) == 96
    if compat:
        b[95] = (b[95] | 0x80) if b[95] & 2 else (b[95] & 0x7F)
    flags = b[95] & 0xC0
    b[47] &= 0x01
    b[95] &= 0x01
    return b, flags


def classify(cand96, compat=False, fast=False):
    """-> (point or None, why): why in "ok", "c0" (c0 >= q), "c1" (c1 >= q), "zero" (x = 0 with the infinity flag), "nonsquare";
    a set infinity flag with x != 0 is ignored.  fast: the root through the C++ oracle's decoder."""
    b, flags = _masked(cand96, compat)
    c0, c1 = int.from_bytes(b[:48], "little"), int.from_bytes(b[48:], "little")
    if c0 >= Q:
        return None, "c0"
    if c1 >= Q:
        return None, "c1"
    if c0 == 0 and c1 == 0 and flags & 0x40:
        return None, "zero"
    greatest = bool(flags & 0x80)
    if fast:
        b[95] |= 0x80 if greatest else 0
        xy, st = co.decompress("g2", bytes(b), check_subgroup=False)
        if st[0] != 0:
            return None, "nonsquare"
        v = co.from_mont(xy.reshape(4, 6), Q)
        return ((v[0], v[1]), (v[2], v[3])), "ok"
    x = (c0, c1)
    y = F2.sqrt(F2.add(F2.mul(F2.sqr(x), x), ecc.B2_377))
    if y is None:
        return None, "nonsquare"
    if ecc._y_is_positive(E2, y) != greatest:          # get_point_from_x(x, greatest): the root with (y < -y) ^ greatest
        y = F2.neg(y)
    return (x, y), "ok"


def infinity_flag_ignored(cand96):
    """the candidate carries the infinity flag beside an x != 0"""
    b, flags = _masked(cand96, False)
    return bool(flags & 0x40) and any(b)


def cofactor_mul(P, fast=False):
    """[H2]P; fast: as sum h_i [2^(248 i)]P over three 248-bit parts of H2, each step an MSM of the C++ oracle (plain integer arithmetic
    on the scalar's bits: it does not care that the points lie outside the r-torsion)"""
    if not fast:
        return E2.mul(P, h2())
    s248 = co.ints_to_limbs([1 << 248], 4)
    pts = [P]
    for _ in range(2):
        xy, inf = co.pack_g2_377(pts[-1:])
        pts.append(co.jac_to_affine(co.msm("bls12_377_g2", xy, inf, s248), "g2_377"))
    xy, inf = co.pack_g2_377(pts)
    parts = [(h2() >> (248 * i)) & ((1 << 248) - 1) for i in range(3)]
    return co.jac_to_affine(co.msm("bls12_377_g2", xy, inf, co.ints_to_limbs(parts, 4)), "g2_377")


def candidate_bytes(mode, domain, pre):
    """the 96 candidate bytes of one attempt; pre = counter || extra || (message or inner)"""
    if mode == "direct":
        return hs.direct_xof(domain, hs.direct_crh(domain, pre, XOF_BYTES), XOF_BYTES)
    if mode == "composite":
        return hs.direct_xof(domain, comp.composite_crh(pre), XOF_BYTES)
    return hs.direct_xof(domain, pre, XOF_BYTES)


def reference_full(mode, domain, message, extra, compat=False, fast=True):
    """-> (affine point of G2, attempt counter, the curve point before the cofactor, the winning candidate's 96 bytes)"""
    assert mode in MODES
    tail = comp.composite_crh(message) if mode == "composite_cip22" else message
    for c in range(255):
        cand = candidate_bytes(mode, domain, bytes([c]) + extra + tail)
        P, _ = classify(cand, compat, fast)
        if P is None:
            continue
        S = cofactor_mul(P, fast)
        if S is None:
            continue
        return S, c, P, cand
    raise ValueError("HashToCurveError")


def reference(mode, domain, message, extra, compat=False, fast=True):
    return reference_full(mode, domain, message, extra, compat, fast)[:2]


def sign_bits_differ(cand96):
    """bit 1 != bit 7 in byte 95: the candidate whose point `compat` negates"""
    return bool(cand96[95] & 2) != bool(cand96[95] & 0x80)


def rows_of(points):
    """affine points -> (n, 24) uint64 Montgomery limbs x.c0, x.c1, y.c0, y.c1, the layout of the library's rows"""
    return co.pack_g2_377(points)[0]


def points_of(rows):
    v = co.from_mont(np.ascontiguousarray(rows).reshape(-1, 6), Q)
    return [((v[4 * i], v[4 * i + 1]), (v[4 * i + 2], v[4 * i + 3])) for i in range(len(v) // 4)]


# ---- inputs
def rand_bytes(rng, n):
    return bytes(rng.integers(0, 256, size=n, dtype=np.uint8))


def total_length_grid(rng):
    """(message, extra) with counter || extra || message of every total length 1 ... 130 (the extra 0 ... 4 bytes of it), then the inner
    lengths of tests/hash_ref.py's tail grid with and without an extra"""
    grid = []
    for total in range(1, 131):
        e = min(total - 1, total % 5)
        grid.append((rand_bytes(rng, total - 1 - e), rand_bytes(rng, e)))
    for l in (0, 1, 15, 62, 63, 64, 65, 127, 128, 200):
        grid += [(rand_bytes(rng, l), b""), (rand_bytes(rng, l), rand_bytes(rng, 1 + l % 5))]
    return grid


# ---- whole batches on the worker pool
def _w_batch(mode, domain, msgs, extras, compat):
    pts, att = [], []
    for m, e in zip(msgs, extras):
        P, c = reference(mode, domain, m, e, compat)
        pts.append(P)
        att.append(c)
    return rows_of(pts), np.array(att, dtype=np.uint8)


class Batch:
    """reference() of every (message, extra) pair, started at once on the pool of tests/ntt_workers.py; rows() waits: (xy (n, 24) uint64,
    attempts (n,) uint8)"""
    def __init__(self, mode, domain, msgs, extras=None, compat=False, per=None):
        import ntt_workers as nw
        assert mode in MODES
        self.n = len(msgs)
        extras = [b""] * self.n if extras is None else extras
        per = per or max(1, min(64, -(-self.n // (2 * nw.workers()))))
        ex = nw.pool()
        self.futs = [ex.submit(_w_batch, mode, domain, msgs[a:a + per], extras[a:a + per], compat) for a in range(0, self.n, per)]
        self._rows = None

    def rows(self):
        if self._rows is None:
            parts = [f.result() for f in self.futs]
            self._rows = (np.concatenate([p[0] for p in parts]) if parts else np.zeros((0, 24), dtype=np.uint64),
                          np.concatenate([p[1] for p in parts]) if parts else np.zeros(0, dtype=np.uint8))
        return self._rows


# ---- the schedule of rounds (csrc/unit_hash.hip: hash_rounds), from reference counters
LANE_BUDGET_LOG, MAX_WIDTH_LOG = 17, 4


def round_widths(attempts, budget_log=LANE_BUDGET_LOG):
    """[(width, open messages, first counter)] of the rounds a call runs for messages with these attempt counters: every round gives each
    open message `width` adjacent counters from `base`, the widest power of two up to 16 with open * width <= 2^budget_log (1 when even
    that is too many); a message closes in the round that covers its counter."""
    att = np.sort(np.asarray(attempts, dtype=np.int64))
    rounds, base = [], 0
    while True:
        count = int(len(att) - np.searchsorted(att, base, side="left"))
        if count == 0 or base >= 255:
            return rounds
        log = 0
        while log < MAX_WIDTH_LOG and (count << (log + 1)) <= (1 << budget_log):
            log += 1
        rounds.append((1 << log, count, base))
        base += 1 << log
