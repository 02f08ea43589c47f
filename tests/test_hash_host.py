"""CPU (-m "not gpu"): the reference helper of the hash tests (tests/hash_ref.py) pinned to the oracle's entries, and the parts of
csrc/hash_direct.h / csrc/pedersen.h that the host build did not reach, run through host_test.cpp with every lazy-reduction bound asserted
(-DCELO_FP_TRACK): the streamed XOF mode, the Pedersen CRH over a byte source at arbitrary bit offsets, the composite mode, SF arithmetic and
the identity branch of tai_finish.

The generator table of the Pedersen tests is NOT the library's: it is built here from the oracle's generators (oracle/py/composite.py,
pinned on the reference's CRH vectors by tests/test_oracle_golden.py) for the first three windows, as g, 2g, 3g, 4g per chunk in
extended coordinates - so these tests also state, independently of csrc/seam_hash.hip, the layout k_pedersen_crh indexes.

Not covered anywhere: counter exhaustion (attempts = 255).  No findable input fails 255 counters in a row, and there is no hook to force
it."""
import ctypes as C

import numpy as np
import pytest

from oracle.py import ecc, hashing as hs, composite as comp
from oracle import cpu_oracle as co
from tests import helpers as H
import hash_ref as hr

SIG, POP = b"ULforxof", b"ULforpop"
TAI = {"direct": 0, "tail": 1, "composite": 2}
Q = ecc.Q377
TABLE_WINDOWS = 3
TABLE_CHUNKS = TABLE_WINDOWS * comp.WINDOW_SIZE            # 279 chunks = 837 bits: strings of up to 104 bytes fit
TABLE_BYTES = TABLE_CHUNKS * 3 // 8


@pytest.fixture(scope="module")
def ht():
    return C.CDLL(H.build_hosttest())


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _rand(rng, n):
    return bytes(rng.integers(0, 256, size=n, dtype=np.uint8))


# ---------------------------------------------------------------------------------------------------------------------- the helper itself
def test_reference_is_the_oracle_entry_on_64_inputs_per_mode():
    """hash_ref.reference restates the loops so that the tail has a reference at all; for the three modes the oracle has an entry for
    it must BE that entry (tests/test_oracle_golden.py pins it on the reference's vectors).  The tail, which has none, is pinned through
    the CIP22 hash it is the second half of."""
    rng = np.random.default_rng(0xA11CE)
    for mode, kw in (("direct", dict(composite=False)), ("composite", dict(composite=True)), ("composite_cip22", dict(composite=True, cip22=True))):
        for i in range(64):
            m, e, dom = _rand(rng, int(rng.integers(0, 90))), _rand(rng, int(rng.integers(0, 20))), (SIG, POP)[i & 1]
            assert hr.reference(mode, dom, m, e) == hs.hash_to_g1(dom, m, e, **kw), (mode, i)
    for i in range(64):
        m, e, dom = _rand(rng, int(rng.integers(0, 90))), _rand(rng, int(rng.integers(0, 20))), (SIG, POP)[i & 1]
        assert hr.reference("tail", dom, comp.composite_crh(m), e) == hs.hash_to_g1(dom, m, e, composite=True, cip22=True), i


def test_round_widths_follow_the_documented_rule():
    """the schedule hash_ref.round_widths predicts from counters, on hand-worked cases: 16 wide up to 8192 open messages, 8 to 16 384,
    4 to 32 768, 2 to 65 536, 1 above; and the benchmark's histogram (2^16 messages) runs 2, 4, 16 wide"""
    for n, w in ((1, 16), (8192, 16), (8193, 8), (16384, 8), (16385, 4), (32768, 4), (32769, 2), (65536, 2), (65537, 1)):
        assert hr.round_widths([0] * n) == [(w, n, 0)]
    hist = [27508, 16020, 9157, 5394, 3074, 1838, 1064, 627, 358, 228, 103, 67, 46, 23, 11, 9, 4, 2, 2, 0, 1]
    att = [c for c, k in enumerate(hist) for _ in range(k)]
    assert hr.round_widths(att) == [(2, 65536, 0), (4, 22008, 2), (16, 2545, 6)]
    assert hr.round_widths([0] * 65537 + [1, 1, 5]) == [(1, 65540, 0), (16, 3, 1)]      # base 1: not a multiple of the next width
    assert hr.round_widths([]) == []


def test_batches_on_the_pool_equal_the_serial_reference():
    rng = np.random.default_rng(77)
    msgs = [_rand(rng, int(rng.integers(0, 70))) for _ in range(40)]
    extras = [_rand(rng, int(rng.integers(0, 9))) for _ in range(40)]
    b = {mode: hr.Batch(mode, SIG, msgs, extras, per=7) for mode in hr.MODES}
    crh = hr.CrhBatch(msgs, per=9)
    for mode in hr.MODES:
        want = [hr.reference(mode, SIG, m, e) for m, e in zip(msgs, extras)]
        xy, att = b[mode].rows()
        assert np.array_equal(xy, co.pack_g1_377([P for P, _ in want])[0]) and att.tolist() == [c for _, c in want]
    assert crh.hashes() == [comp.composite_crh(m) for m in msgs]


# ------------------------------------------------------------------------------------------------------- host build under bounds tracking
def _ht_hash(ht, mode, dom, msg, extra, table=None):
    out = np.zeros(12, dtype=np.uint64)
    c = ht.ht_hash_to_g1(TAI[mode], dom, msg, C.c_size_t(len(msg)), extra, C.c_size_t(len(extra)), _p(table) if table is not None else None,
                         C.c_size_t(TABLE_CHUNKS if table is not None else 0), _p(out))
    return c, tuple(co.from_mont(out.reshape(2, 6), Q))


def test_streamed_xof_mode_under_bounds_tracking(ht):
    """TAI_XOF_ONLY (b2s_stream over the TaiBytes source, twice per attempt) on the host with bounds asserted, over the length grid of the
    GPU test, both domains: point and counter equal reference("tail")"""
    grid = hr.tail_length_grid(np.random.default_rng(0x7A11))
    for dom in (SIG, POP):
        for inner, extra in grid:
            P, wc = hr.reference("tail", dom, inner, extra)
            assert _ht_hash(ht, "tail", dom, inner, extra) == (wc, P), (dom, len(inner), len(extra))
    # and the mode argument reaches the direct loop as before
    P, wc = hr.reference("direct", SIG, b"abc", b"\x01")
    assert _ht_hash(ht, "direct", SIG, b"abc", b"\x01") == (wc, P)


@pytest.fixture(scope="module")
def small_table():
    """rows 4 ch + m = (m + 1) * generator ch, ch = 93 * window + j, generator j of a window = 16^j * its base; X, Y, Z = 1, T = X Y as
    Montgomery limbs: (279 * 4, 24) uint64.  Formed with the oracle's affine addition from the oracle's bases."""
    rows = []
    for base in comp.generators(TABLE_WINDOWS)[:TABLE_WINDOWS]:
        g = base
        for _ in range(comp.WINDOW_SIZE):
            g2 = comp.ed_add(g, g)
            g3 = comp.ed_add(g2, g)
            g4 = comp.ed_add(g3, g)
            for x, y in (g, g2, g3, g4):
                rows += [x, y, 1, x * y % Q]
            g = comp.ed_add(g4, g4)
            g = comp.ed_add(g, g)
    return co.to_mont(rows, Q).reshape(TABLE_CHUNKS * 4, 24)


def test_pedersen_crh_under_bounds_tracking_on_an_independent_table(ht, small_table):
    """pedersen_crh_src / ed_add / SF under bounds tracking for every length the three-window table covers (0 ... 104 bytes), random bytes and the
    all-ones string (every chunk: 4g, negated), against the oracle; one byte more is refused"""
    rng = np.random.default_rng(0xED)
    for l in range(TABLE_BYTES + 1):
        for msg in (_rand(rng, l), b"\xff" * l):
            out = np.zeros(48, dtype=np.uint8)
            assert ht.ht_pedersen_crh(_p(small_table), C.c_size_t(TABLE_CHUNKS), msg, C.c_size_t(l), _p(out)) == 0
            assert out.tobytes() == comp.composite_crh(msg), l
    out = np.zeros(48, dtype=np.uint8)
    assert ht.ht_pedersen_crh(_p(small_table), C.c_size_t(TABLE_CHUNKS), bytes(TABLE_BYTES + 1), C.c_size_t(TABLE_BYTES + 1), _p(out)) == -2


def test_composite_mode_under_bounds_tracking(ht, small_table):
    """TAI_COMPOSITE (a Pedersen CRH per attempt, read through TaiBytes: the counter byte shifts every later chunk) on the same table"""
    rng = np.random.default_rng(0xC0)
    for msg, extra in hr.composite_length_grid(rng):
        if 1 + len(extra) + len(msg) <= TABLE_BYTES:
            P, wc = hr.reference("composite", SIG, msg, extra)
            assert _ht_hash(ht, "composite", SIG, msg, extra, small_table) == (wc, P), (len(msg), len(extra))
    assert ht.ht_hash_to_g1(2, SIG, bytes(104), C.c_size_t(104), b"", C.c_size_t(0), _p(small_table), C.c_size_t(TABLE_CHUNKS),
                            _p(np.zeros(12, dtype=np.uint64))) == -2


# ---- tai_finish: the cofactor multiple, and the identity branch the GPU's `redo` path rests on
COFACTOR_FACTORS = {2: 92, 3: 1, 7: 2, 13: 2, 499: 2}


def _curve_point(rng):
    while True:
        x = int.from_bytes(_rand(rng, 48), "little") % Q
        y = ecc.sqrt_fp((x * x * x + 1) % Q, Q)
        if y is not None:
            return (x, y)


def _finish(ht, P):
    out = np.zeros(12, dtype=np.uint64)
    ok = ht.ht_tai_finish(_p(co.pack_g1_377([P])[0]), _p(out))
    return tuple(co.from_mont(out.reshape(2, 6), Q)) if ok else None


def test_cofactor_factorisation():
    h = 1
    for p, k in COFACTOR_FACTORS.items():
        h *= p ** k
    assert h == ecc.H1_377


def test_tai_finish_ordinary_points(ht):
    rng = np.random.default_rng(0xF1)
    for _ in range(24):
        P = _curve_point(rng)
        want = ecc.E1_377.mul(P, ecc.H1_377)
        assert want is not None and ecc.E1_377.in_subgroup(want)
        assert _finish(ht, P) == want


def test_tai_finish_returns_identity_on_the_cofactor_subgroup(ht):
    """Points whose cofactor multiple is the identity cannot be reached through the ABI with honest inputs (about 2^-125 per message), so the
    branch k_hash_finish flags for the serial loop is tested here: r * Q for curve points Q off the prime-order subgroup, and points of
    order 2, 3, 4, 7, 13 and 499, where the ladder meets s = -P or the identity in mid-run.  No bound and no assert may trip."""
    E, h, r = ecc.E1_377, ecc.H1_377, ecc.R377
    rng = np.random.default_rng(0xF2)
    torsion = []
    while len(torsion) < 6:
        T = E.mul(_curve_point(rng), r)
        if T is not None:
            torsion.append(T)
    for T in torsion:
        assert E.on_curve(T) and E.mul(T, h) is None and _finish(ht, T) is None
    assert E.on_curve((Q - 1, 0)) and E.mul((Q - 1, 0), 2) is None                # order 2: the first doubling has y = 0
    assert _finish(ht, (Q - 1, 0)) is None
    seen = {}
    for order, prime in ((3, 3), (4, 2), (7, 7), (13, 13), (499, 499)):
        for T in torsion:
            S = E.mul(T, h // prime ** COFACTOR_FACTORS[prime])              # the prime-power part of T ...
            while S is not None and E.mul(S, order) is not None:            # ... brought down to the order wanted (the part need not be cyclic)
                S = E.mul(S, prime)
            if S is not None and E.mul(S, order // prime) is not None:
                seen[order] = S
                for V in (S, E.neg(S), E.mul(S, 2)):
                    if V is not None:
                        assert _finish(ht, V) is None, (order, V)
                break
    assert sorted(seen) == [3, 4, 7, 13, 499]
    assert seen[3][0] == 0 and seen[3][1] in (1, Q - 1)                           # (0, +-1): a candidate x = 0 without the 0x40 flag selects them
    for V in ((0, 1), (0, Q - 1)):
        assert _finish(ht, V) is None
    # sums of a subgroup point and a torsion point are ordinary inputs again: the multiple loses the torsion part
    G = ecc.G1_377
    for T in torsion[:3] + [seen[3], (Q - 1, 0)]:
        P = E.add(G, T)
        assert _finish(ht, P) == E.mul(G, h)
