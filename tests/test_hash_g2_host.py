"""CPU (-m "not gpu"): hash-to-G2 without a GPU.  Three layers, each pinned on the one before:

  1. the cofactor H2 of the twist, derived (tests/hash_g2_ref.py: the one of six candidate orders that r divides and that kills a point);
  2. the reference helper, on the reference's own ten G2 vectors (crates/bls-crypto/src/hash_to_curve/mod.rs:490-513; tests/golden), in its
     pure-Python form and in the fast form the batches use;
  3. the library's host code: hash_to_g2_one_bls12_377 on the same ten vectors with the library's own generator table, and
     csrc/hash_direct.h through host_test.cpp with every lazy-reduction bound asserted (-DCELO_FP_TRACK) against the helper: all four modes
     over lengths, both flag logics, every rejection class, the identity branch of the cofactor multiple.

No faster form of the cofactor multiple ships (tai_finish_g2 runs its definition, the 502-bit ladder), so there is none to compare.
Not covered anywhere: counter exhaustion (attempts = 255) and the flagged zero point - no findable input reaches either."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from oracle.py import ecc, composite as comp
from oracle import cpu_oracle as co
from tests import helpers as H
from tests.test_oracle_golden import reference_hash_test_inputs
from tests.test_hash_host import small_table, TABLE_CHUNKS, TABLE_BYTES       # noqa: F401  (the fixture: the oracle's first three windows)
import hash_ref as hr
import hash_g2_ref as g2

SIG, POP = b"ULforxof", b"ULforpop"
TAI = {"direct": 0, "tail": 1, "composite": 2}
Q, R = ecc.Q377, ecc.R377
E2 = ecc.E2_377
H2_STATED = 0x26ba558ae9562addd88d99a6f6a829fbb36b00e1dcc40c8c505634fae2e189d693e8c36676bd09a0f3622fba094800452217cc900000000000000000000001
VECTOR_COUNTERS = [1, 0, 8, 2, 1, 0, 2, 1, 7, 4]


@pytest.fixture(scope="module")
def ht():
    return C.CDLL(H.build_hosttest())


@pytest.fixture(scope="module")
def vectors():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pts = json.load(open(os.path.join(root, "tests", "golden", "reference_vectors.json")))["hash_to_curve"]["g2_noncompat"]["points"]
    return list(zip(reference_hash_test_inputs(len(pts)), [bytes.fromhex(h) for h in pts]))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------------------------------------------------------------------- 1. H2
def test_h2_is_derived_and_is_the_cofactor_of_the_twist():
    rng = np.random.default_rng(0x112)
    h2, order = g2.derive_h2(rng)
    assert order in g2.twist_orders() and len(set(g2.twist_orders())) == 6
    assert h2 * R == order and h2 == g2.h2() == H2_STATED
    assert h2.bit_length() == 502 and bin(h2).count("1") == 196
    assert math.gcd(h2, R) == 1
    for _ in range(8):
        P = g2.random_twist_point(rng)
        assert E2.on_curve(P) and E2.mul(P, R) is not None and E2.mul(P, h2) is not None and E2.mul(P, h2 * R) is None
    # the other five orders are no order of this curve: some point survives each
    P = g2.random_twist_point(rng)
    assert [n for n in g2.twist_orders() if E2.mul(P, n) is None] == [order]


# ------------------------------------------------------------------------------------------------------- 2. the helper on the vectors
def test_helper_reproduces_the_reference_vectors_in_pure_python(vectors):
    got = [g2.reference("composite", dom, msg, extra, compat=False, fast=False) for (dom, msg, extra), _ in vectors]
    assert [c for _, c in got] == VECTOR_COUNTERS
    for (S, _), (_, want) in zip(got, vectors):
        assert ecc.ser_point(E2, S) == want
        assert E2.in_subgroup(S)


def test_fast_forms_equal_the_pure_python_forms(vectors):
    """co.decompress as the candidate map on 64 candidates (of every class but the flagged zero), three co.msm calls as the cofactor
    multiple on 16 points; and the fast loop on the vectors"""
    rng = np.random.default_rng(0xFA57)
    seen = {}
    for i in range(64):
        cand = g2.candidate_bytes("tail", SIG, bytes([i]) + g2.rand_bytes(rng, 20))
        for compat in (False, True):
            a, b = g2.classify(cand, compat, fast=False), g2.classify(cand, compat, fast=True)
            assert a == b, i
        seen[a[1]] = seen.get(a[1], 0) + 1
    assert set(seen) == {"ok", "c0", "c1", "nonsquare"}, seen
    zero = bytearray(96)
    zero[95] = 0x40
    assert g2.classify(bytes(zero), fast=True) == g2.classify(bytes(zero), fast=False) == (None, "zero")
    zero[95] = 0x00                                     # x = 0 without the flag: B' = -u / 5 is looked at like any other right-hand side
    assert g2.classify(bytes(zero), fast=True) == g2.classify(bytes(zero), fast=False)
    for _ in range(16):
        P = g2.random_twist_point(rng)
        assert g2.cofactor_mul(P, fast=True) == g2.cofactor_mul(P, fast=False)
    for ((dom, msg, extra), want), c in zip(vectors, VECTOR_COUNTERS):
        S, got_c = g2.reference("composite", dom, msg, extra, compat=False, fast=True)
        assert ecc.ser_point(E2, S) == want and got_c == c


# ------------------------------------------------------------------------------------------ 3. the library's host code on the vectors
def test_library_host_loop_returns_the_reference_vectors(vectors):
    """hash_to_g2_one_bls12_377, composite mode, compat = 0, with the library's own generator table: the ten points and their counters.
    No device is touched."""
    from celo_bls_snark_rs_amd import ffi
    got_c = []
    for (dom, msg, extra), want in vectors:
        xy, c = ffi.hash_to_g2_one(dom, msg, extra, mode=2, compat=0)
        got_c.append(c)
        assert ecc.ser_point(E2, g2.points_of(xy)[0]) == want
    assert got_c == VECTOR_COUNTERS


def test_library_host_loop_all_modes_and_refused_arguments():
    from celo_bls_snark_rs_amd import ffi
    rng = np.random.default_rng(0x0E)
    msg, extra = g2.rand_bytes(rng, 33), g2.rand_bytes(rng, 3)
    for mode in g2.MODES:
        m = comp.composite_crh(msg) if mode == "tail" else msg
        for compat in (0, 1):
            S, c = g2.reference(mode, SIG, m, extra, compat=bool(compat))
            xy, got_c = ffi.hash_to_g2_one(SIG, m, extra, mode=g2.MODE_INDEX[mode], compat=compat)
            assert got_c == c and g2.points_of(xy)[0] == S, (mode, compat)
    for kw in (dict(mode=4), dict(mode=-1), dict(compat=2), dict(compat=-1)):
        with pytest.raises(RuntimeError):
            ffi.hash_to_g2_one(SIG, msg, extra, **kw)
    with pytest.raises(RuntimeError):
        ffi.hash_to_g2_one(SIG, bytes(hr.PEDERSEN_MAX_BYTES), b"", mode=2)      # counter || message: one byte beyond the generator table
    xy = np.zeros(24, dtype=np.uint64)
    assert ffi.lib().hash_to_g2_one_bls12_377(SIG, msg, C.c_size_t(len(msg)), None, C.c_size_t(0), C.c_int(0), C.c_int(0), _p(xy), None) == 2


def test_batched_entries_refuse_without_a_device():
    """the batched entries are GPU code: without a device they return an error, they do not fall back to the host loop"""
    import torch
    from celo_bls_snark_rs_amd import ffi
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    for call in (lambda: ffi.hash_to_g2_direct(SIG, [b"m"]), lambda: ffi.hash_to_g2_direct(SIG, [bytes(48)], cip22_tail=True),
                 lambda: ffi.hash_to_g2_composite(SIG, [b"m"]), lambda: ffi.hash_to_g2_composite(SIG, [b"m"], cip22=True, compat=1)):
        with pytest.raises(RuntimeError):
            call()


def test_compat_negates_exactly_where_the_two_sign_bits_differ():
    """The remap changes the y-sign flag only, so the same counter wins and the result is the negated point exactly when bit 1 != bit 7 in
    byte 95 of the winning candidate.  Both kinds must occur at least 4 times among the inputs."""
    from celo_bls_snark_rs_amd import ffi
    rng = np.random.default_rng(0xF1A6)
    kinds = {True: 0, False: 0}
    for i in range(16):
        msg, extra = g2.rand_bytes(rng, 5 + i), g2.rand_bytes(rng, i % 3)
        S, c, _, cand = g2.reference_full("direct", POP, msg, extra, compat=False)
        differ = g2.sign_bits_differ(cand)
        kinds[differ] += 1
        assert g2.reference("direct", POP, msg, extra, compat=True) == (E2.neg(S) if differ else S, c)
        plain, remap = ffi.hash_to_g2_one(POP, msg, extra, mode=0, compat=0), ffi.hash_to_g2_one(POP, msg, extra, mode=0, compat=1)
        assert plain[1] == remap[1] == c
        assert g2.points_of(plain[0])[0] == S and g2.points_of(remap[0])[0] == (E2.neg(S) if differ else S), i
    assert min(kinds.values()) >= 4, kinds


# ------------------------------------------------------------------------------------------- host build under bounds tracking
def _ht_hash(ht, mode, compat, dom, msg, extra, table=None):
    out = np.zeros(24, dtype=np.uint64)
    c = ht.ht_hash_to_g2(TAI[mode], C.c_int(int(compat)), dom, msg, C.c_size_t(len(msg)), extra, C.c_size_t(len(extra)), _p(table) if table is not None else None,
                         C.c_size_t(TABLE_CHUNKS if table is not None else 0), _p(out))
    return c, g2.points_of(out)[0]


@pytest.fixture(scope="module")
def length_set():
    """the (message, extra) pairs of the length tests - counter || extra || message of every length 1 ... 130 and the inner lengths of the tail
    grid - with their references for both streamed modes, compat alternating, started on the pool"""
    grid = g2.total_length_grid(np.random.default_rng(0x62))
    assert sorted({1 + len(m) + len(e) for m, e in grid[:130]}) == list(range(1, 131))
    refs = {(mode, compat): g2.Batch(mode, SIG, [m for m, _ in grid], [e for _, e in grid], compat=compat) for mode in ("direct", "tail") for compat in (False, True)}
    return grid, refs


@pytest.mark.parametrize("mode", ["direct", "tail"])
def test_streamed_modes_under_bounds_tracking(ht, length_set, mode):
    grid, refs = length_set
    for compat in (False, True):
        wxy, watt = refs[mode, compat].rows()
        want = g2.points_of(wxy)
        for i, (m, e) in enumerate(grid):
            if (i & 1) == int(compat):
                assert _ht_hash(ht, mode, compat, SIG, m, e) == (int(watt[i]), want[i]), (mode, compat, len(m), len(e))


def test_composite_modes_under_bounds_tracking(ht, small_table):
    """TAI_COMPOSITE (a Pedersen CRH per attempt) and the CIP22 form (one CRH by the same host code, then the tail) on the short table"""
    rng = np.random.default_rng(0xC2)
    ran = 0
    for i, (msg, extra) in enumerate(hr.composite_length_grid(rng)):
        if 1 + len(extra) + len(msg) > TABLE_BYTES:
            continue
        compat = bool(i & 1)
        assert _ht_hash(ht, "composite", compat, SIG, msg, extra, small_table) == g2.reference("composite", SIG, msg, extra, compat)[::-1], (len(msg), len(extra))
        inner = np.zeros(48, dtype=np.uint8)
        assert ht.ht_pedersen_crh(_p(small_table), C.c_size_t(TABLE_CHUNKS), msg, C.c_size_t(len(msg)), _p(inner)) == 0
        assert _ht_hash(ht, "tail", compat, SIG, inner.tobytes(), extra) == g2.reference("composite_cip22", SIG, msg, extra, compat)[::-1], (len(msg), len(extra))
        ran += 1
    assert ran >= 36
    assert ht.ht_hash_to_g2(2, 0, SIG, bytes(104), C.c_size_t(104), b"", C.c_size_t(0), _p(small_table), C.c_size_t(TABLE_CHUNKS), _p(np.zeros(24, dtype=np.uint64))) == -2


def test_the_length_set_meets_every_rejection_class(length_set):
    """what the bounds-tracking runs above went through: at counter 0 the set's candidates include at least 8 of each way a candidate is
    turned down, at least 8 that carry the infinity flag beside x != 0 (ignored), and winners that carry it"""
    grid, refs = length_set
    seen = {"ok": 0, "c0": 0, "c1": 0, "nonsquare": 0, "zero": 0}
    flagged = flagged_ok = 0
    for mode in ("direct", "tail"):
        for m, e in grid:
            cand = g2.candidate_bytes(mode, SIG, b"\0" + e + m)
            why = g2.classify(cand, False, fast=True)[1]
            seen[why] += 1
            flagged += g2.infinity_flag_ignored(cand)
            flagged_ok += g2.infinity_flag_ignored(cand) and why == "ok"
    assert min(seen["c0"], seen["c1"], seen["nonsquare"]) >= 8 and flagged >= 8 and flagged_ok >= 8, (seen, flagged, flagged_ok)
    assert max(int(refs[mode, False].rows()[1].max()) for mode in ("direct", "tail")) >= 4        # several counters were needed somewhere


# ---- tai_finish_g2: the cofactor multiple, and the identity branch the GPU's `redo` path rests on
def _finish(ht, P):
    out = np.zeros(24, dtype=np.uint64)
    ok = ht.ht_tai_finish_g2(_p(g2.rows_of([P])), _p(out))
    assert ok in (0, 1)
    return g2.points_of(out)[0] if ok else None


def test_tai_finish_g2_ordinary_points(ht):
    rng = np.random.default_rng(0xF3)
    for i in range(16):
        P = g2.random_twist_point(rng)
        want = g2.cofactor_mul(P, fast=i >= 4)               # four against the pure-Python ladder, the rest through the pinned fast form
        assert want is not None and _finish(ht, P) == want
    assert E2.in_subgroup(want)
    # points of the r-torsion are ordinary inputs: the multiple is [H2 mod r]P
    for k in (1, 2, 0x1234567):
        P = E2.mul(ecc.G2_377, k)
        assert _finish(ht, P) == E2.mul(P, g2.h2() % R)


def test_tai_finish_g2_returns_identity_on_the_cofactor_subgroup(ht):
    """[r]P of random twist points has order dividing H2: the multiple is the identity, the function returns 0 (what k_hash_finish_g2 flags for
    the serial loop).  No findable hash input reaches this, so it is tested here.  No bound and no assert may trip."""
    rng = np.random.default_rng(0xF4)
    G = ecc.G2_377
    for _ in range(8):
        T = E2.mul(g2.random_twist_point(rng), R)
        assert T is not None and E2.on_curve(T) and E2.mul(T, g2.h2()) is None
        assert _finish(ht, T) is None
        # the sum with a subgroup point is an ordinary input again: the multiple loses the torsion part
        assert _finish(ht, E2.add(G, T)) == E2.mul(G, g2.h2() % R)


# ---- the schedule and its setter
def test_round_widths_at_both_budgets():
    for n, w in ((1, 16), (8192, 16), (8193, 8), (16384, 8), (16385, 4), (32768, 4), (32769, 2), (65536, 2), (65537, 1)):
        assert g2.round_widths([0] * n) == g2.round_widths([0] * n, 17) == [(w, n, 0)]
    for n, w in ((1, 16), (16, 16), (17, 8), (32, 8), (33, 4), (64, 4), (65, 2), (128, 2), (129, 1), (300, 1)):
        assert g2.round_widths([0] * n, 8) == [(w, n, 0)]
    # 129 messages at budget 8, counters 0 x 100, 1 x 20, 2 x 5, 9 x 4: 1 wide on 129; 29 left from base 1: 29 * 8 = 232 <= 256 < 29 * 16, so 8
    # wide; 4 left from base 9 (not a multiple of 16): 16 wide
    assert g2.round_widths([0] * 100 + [1] * 20 + [2] * 5 + [9] * 4, 8) == [(1, 129, 0), (8, 29, 1), (16, 4, 9)]
    # 200 open: 1 wide; 120 left: 2 wide from base 1; 40 left from base 3: 4 wide; 20 left from base 7: 8 wide; 3 left from base 15: 16 wide
    att = [0] * 80 + [1] * 50 + [2] * 30 + [3] * 10 + [6] * 10 + [7] * 10 + [14] * 7 + [15] * 2 + [30]
    assert g2.round_widths(att, 8) == [(1, 200, 0), (2, 120, 1), (4, 40, 3), (8, 20, 7), (16, 3, 15)]
    assert g2.round_widths([], 8) == []


def test_budget_setter_refuses_values_outside_4_to_17():
    from celo_bls_snark_rs_amd import ffi
    for bad in (-1, 0, 3, 18, 64):
        assert ffi.hash_g2_set_lane_budget_log(bad) == 2
    for good in (4, 8, 17):
        assert ffi.hash_g2_set_lane_budget_log(good) == 0
