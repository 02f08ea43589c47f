"""GPU (-m gpu): batched hash-to-G2 through the C ABI (include/celo_bls_amd.h: hash_to_g2_*_bls12_377) against the restatement of
tests/hash_g2_ref.py, which tests/test_hash_g2_host.py pins on the reference's ten G2 vectors (crates/bls-crypto/src/hash_to_curve/
mod.rs:490-513).  Every comparison is of WHOLE outputs - all 24 limbs of every row and every attempt counter - with no sampling and no
tolerance: byte and integer work is bit-exact.  The references are evaluated on the worker processes of tests/ntt_workers.py, all started
when the first test asks for one.

The module follows the code's own shapes (csrc/unit_hash.hip): the four modes, both flag logics, lengths across the Blake2s block, the
generator table's limit, and rounds 1, 2, 4, 8 and 16 counters wide.  Widths below 16 need more than 8192 open messages at the default
lane budget (2^17), each costing the reference a 502-bit multiple over Fq2; so they are reached with the budget set to 2^8
(celo_amd_hash_g2_set_lane_budget_log), where 17 ... 129 messages do.  The width reaches the kernel as an argument either way.

NOT covered here: widths below 16 at the default budget; the identity multiple and counter exhaustion (attempts = 255: no findable input;
the identity branch is tested on the host build, tests/test_hash_g2_host.py); the flagged zero point."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch  # noqa: F401  before the library: both must share one HIP runtime
from oracle.py import ecc
from oracle import cpu_oracle as co
from tests.test_oracle_golden import reference_hash_test_inputs
import hash_ref as hr
import hash_g2_ref as g2

pytestmark = pytest.mark.gpu
SIG, POP = b"ULforxof", b"ULforpop"
N_MASTER = 300
PREFIXES = (1, 15, 16, 17, 32, 33, 64, 65, 128, 129, 300)
SLICE = (37, 37 + 100)
MAX_BYTES = hr.PEDERSEN_MAX_BYTES
VECTOR_COUNTERS = [1, 0, 8, 2, 1, 0, 2, 1, 7, 4]


def _varied(seed, n, max_len, max_extra):
    rng = np.random.default_rng(seed)
    return [g2.rand_bytes(rng, int(rng.integers(0, max_len + 1))) for _ in range(n)], [g2.rand_bytes(rng, int(rng.integers(0, max_extra + 1))) for _ in range(n)]


class Refs:
    """every input of the module and its reference, started on the pool at once: the maximum-length hash first (tens of seconds in one
    worker: it runs beside the rest), then the small sets"""
    def __init__(self):
        g = np.random.default_rng(0x62D)
        self.max_msg, self.max_extra = g2.rand_bytes(g, MAX_BYTES - 1 - 9), g2.rand_bytes(g, 9)
        self.max_composite = g2.Batch("composite", SIG, [self.max_msg], [self.max_extra])
        self.vec_inputs = reference_hash_test_inputs(10)

        self.grid = g2.total_length_grid(np.random.default_rng(0x62))
        self.grid_ref = {(mode, dom, compat): g2.Batch(mode, dom, [m for m, _ in self.grid], [e for _, e in self.grid], compat=compat)
                         for mode, dom, compat in (("direct", SIG, False), ("tail", POP, True))}
        self.grid_noextra_ref = g2.Batch("tail", SIG, [m for m, _ in self.grid], None, compat=False)
        self.comp_grid = hr.composite_length_grid(np.random.default_rng(0xC0))
        self.comp64 = _varied(0x5EED0204, 64, 40, 5)
        self.comp_msgs = ([m for m, _ in self.comp_grid] + self.comp64[0], [e for _, e in self.comp_grid] + self.comp64[1])
        self.comp_ref = {mode: g2.Batch(mode, SIG, *self.comp_msgs) for mode in ("composite", "composite_cip22")}

        self.master = _varied(0x5EED0201, N_MASTER, 130, 40)
        self.direct = {compat: g2.Batch("direct", SIG, *self.master, compat=compat) for compat in (False, True)}
        self.indep = {mode: _varied(0x5EED0210 + i, 40, 48, 4) for i, mode in enumerate(g2.MODES)}
        for m in self.indep["tail"][0]:
            assert len(m) <= 48
        self.indep_ref = {mode: g2.Batch(mode, POP, *self.indep[mode], compat=(i & 1) == 1) for i, mode in enumerate(g2.MODES)}
        self.g1 = _varied(0x5EED0220, 50, 60, 6)
        self.g1_ref = hr.Batch("direct", SIG, *self.g1)


_REFS = None


@pytest.fixture(scope="module")
def refs():
    global _REFS
    if _REFS is None:
        _REFS = Refs()
    return _REFS


def _call(gpu, mode, dom, msgs, extras, compat=0):
    if mode == "direct":
        return gpu.hash_to_g2_direct(dom, msgs, extras, compat=compat)
    if mode == "tail":
        return gpu.hash_to_g2_direct(dom, msgs, extras, cip22_tail=True, compat=compat)
    return gpu.hash_to_g2_composite(dom, msgs, extras, cip22=(mode == "composite_cip22"), compat=compat)


def _same(got, want, lo=0, hi=None):
    """every row and every counter, as integers"""
    (xy, att), (wxy, watt) = got, want
    assert xy.shape[1] == 24
    assert np.array_equal(att, watt[lo:hi]), "counters differ at %s" % np.flatnonzero(att != watt[lo:hi])[:8]
    assert np.array_equal(xy, wxy[lo:hi]), "points differ at rows %s" % np.flatnonzero((xy != wxy[lo:hi]).any(axis=1))[:8]


# ---- the reference's own vectors
def test_the_ten_reference_vectors_through_the_composite_entry(gpu, refs, golden):
    """hash_to_curve/mod.rs:490-513 (test_hash_to_curve_g2): composite hasher, compat = 0.  Points and counters, and the library's own G2
    encoder returns the golden bytes.  The reference draws a domain per vector and a call takes one domain, so each vector is a call; the
    ten messages then go through ONE call under the first domain, against the helper."""
    want = [bytes.fromhex(h) for h in golden["hash_to_curve"]["g2_noncompat"]["points"]]
    assert len(want) == 10
    rows, counters = [], []
    for dom, msg, extra in refs.vec_inputs:                         # every vector has a domain of its own: one call each ...
        xy, att = gpu.hash_to_g2_composite(dom, [msg], [extra], compat=0)
        rows.append(xy[0])
        counters.append(int(att[0]))
    assert counters == VECTOR_COUNTERS
    out, st = gpu.encode_points("g2", np.stack(rows), None, compressed=True)
    assert (st == 0).all() and [out[i].tobytes() for i in range(10)] == want
    assert [ecc.ser_point(ecc.E2_377, P) for P in g2.points_of(np.stack(rows))] == want
    # ... and ten messages in ONE call under one domain, against the helper
    dom = refs.vec_inputs[0][0]
    msgs, extras = [m for _, m, _ in refs.vec_inputs], [e for _, _, e in refs.vec_inputs]
    _same(gpu.hash_to_g2_composite(dom, msgs, extras, compat=0), g2.Batch("composite", dom, msgs, extras).rows())


# ---- lengths
def test_direct_and_tail_over_every_length(gpu, refs):
    """counter || extra || message of every total length 1 ... 130 (across the 64-byte Blake2s block, 64 and 128 ending on one exactly), then
    the inner lengths 0, 1, 15, 62 ... 65, 127, 128, 200; direct with compat = 0 under one domain, the tail with compat = 1 under the other,
    and the tail without the extras pointer"""
    msgs, extras = [m for m, _ in refs.grid], [e for _, e in refs.grid]
    _same(_call(gpu, "direct", SIG, msgs, extras, 0), refs.grid_ref["direct", SIG, False].rows())
    _same(_call(gpu, "tail", POP, msgs, extras, 1), refs.grid_ref["tail", POP, True].rows())
    _same(_call(gpu, "tail", SIG, msgs, None, 0), refs.grid_noextra_ref.rows())
    assert int(refs.grid_ref["direct", SIG, False].rows()[1].max()) >= 4


@pytest.mark.parametrize("mode", ["composite", "composite_cip22"])
def test_composite_lengths_and_a_batch_of_64(gpu, refs, mode):
    """message lengths {0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 100} x extra lengths {0, 1, 7, 32}, then 64 varied messages, in one call"""
    _same(_call(gpu, mode, SIG, *refs.comp_msgs), refs.comp_ref[mode].rows())


def test_composite_at_the_maximum_length_and_one_byte_beyond(gpu, refs):
    """counter || extra || message of exactly 19 530 bytes fills the generator table: accepted, equal to the helper.  One byte more: the
    reference panics, the library returns 2 - and goes on working."""
    assert 1 + len(refs.max_extra) + len(refs.max_msg) == MAX_BYTES
    _same(gpu.hash_to_g2_composite(SIG, [refs.max_msg], [refs.max_extra]), refs.max_composite.rows())
    for msgs, extras in (([refs.max_msg + b"\0"], [refs.max_extra]), ([b"short", refs.max_msg], [b"", refs.max_extra + b"\0"])):
        with pytest.raises(RuntimeError, match="code 2"):
            gpu.hash_to_g2_composite(SIG, msgs, extras)
    _same(gpu.hash_to_g2_composite(SIG, [refs.max_msg], [refs.max_extra]), refs.max_composite.rows())


# ---- every width
def _direct_range(gpu, refs, lo, hi, budget_log, compat=False):
    msgs, extras = refs.master
    want = refs.direct[compat].rows()
    _same(gpu.hash_to_g2_direct(SIG, msgs[lo:hi], extras[lo:hi], compat=int(compat)), want, lo, hi)
    rounds = g2.round_widths(want[1][lo:hi], budget_log)
    assert gpu.hash_last_rounds() == len(rounds), (gpu.hash_last_rounds(), rounds)
    return rounds


def test_every_width_with_the_lane_budget_at_2_to_the_8(gpu, refs):
    """Prefixes of one 300-message set on both sides of 16, 32, 64 and 128 messages, where the first round narrows from 16 to 8, 4, 2 and 1
    counters per message, and a slice that does not start at message 0.  Every row, every counter, and the number of rounds the schedule
    predicts from the REFERENCE counters.  The schedules together must hold every width on live messages, widths 2 ... 16 also as later
    rounds (index list), and a round whose first counter is no multiple of its width."""
    assert gpu.hash_g2_set_lane_budget_log(8) == 0
    try:
        schedules = [_direct_range(gpu, refs, 0, n, 8) for n in PREFIXES] + [_direct_range(gpu, refs, *SLICE, 8)]
    finally:
        assert gpu.hash_g2_set_lane_budget_log(17) == 0
    first = {n: s[0][0] for n, s in zip(PREFIXES, schedules)}
    assert first == {1: 16, 15: 16, 16: 16, 17: 8, 32: 8, 33: 4, 64: 4, 65: 2, 128: 2, 129: 1, 300: 1}
    assert all(count >= 1 for s in schedules for _, count, _ in s)
    later = {w for s in schedules for w, _, _ in s[1:]}
    assert {s[0][0] for s in schedules} == {1, 2, 4, 8, 16} and later >= {2, 4, 8, 16}, later
    assert any(base % w for s in schedules for w, _, base in s[1:])
    _direct_range(gpu, refs, 0, 40, 17)                            # the default is back: 40 messages run 16 wide again


@pytest.mark.parametrize("compat", [False, True])
def test_default_budget_one_message_and_300(gpu, refs, compat):
    for n in (1, N_MASTER):
        assert _direct_range(gpu, refs, 0, n, 17, compat)[0][0] == 16
    plain, remap = refs.direct[False].rows(), refs.direct[True].rows()
    assert np.array_equal(plain[1], remap[1])                      # the remap changes the sign flag only ...
    differ = (plain[0] != remap[0]).any(axis=1)
    assert 100 <= int(differ.sum()) <= 200 and np.array_equal(plain[0][:, :12], remap[0][:, :12])     # ... so about half the points are negated


# ---- batch independence
@pytest.mark.parametrize("mode", g2.MODES)
def test_batch_independence(gpu, refs, mode):
    """The same 40 messages as one call, reversed in calls of 8, and at scattered positions among 200 unrelated messages: identical rows.  On
    top of the comparison with the helper (first assertion), not instead of it."""
    msgs, extras = refs.indep[mode]
    compat = g2.MODES.index(mode) & 1
    one = _call(gpu, mode, POP, msgs, extras, compat)
    _same(one, refs.indep_ref[mode].rows())
    rm, re_ = msgs[::-1], extras[::-1]
    for a in range(0, 40, 8):
        xy, att = _call(gpu, mode, POP, rm[a:a + 8], re_[a:a + 8], compat)
        assert np.array_equal(xy, one[0][::-1][a:a + 8]) and np.array_equal(att, one[1][::-1][a:a + 8]), a
    rng = np.random.default_rng(0x5CA7)
    pos = np.sort(rng.choice(200, size=40, replace=False))
    big_m, big_e = _varied(0x5EED0230, 200, 48, 4)
    for p, m, e in zip(pos, msgs, extras):
        big_m[p], big_e[p] = m, e
    xy, att = _call(gpu, mode, POP, big_m, big_e, compat)
    assert np.array_equal(xy[pos], one[0]) and np.array_equal(att[pos], one[1])


# ---- arguments
def _u8(b):
    return np.frombuffer(b or b"\0", dtype=np.uint8)


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_empty_batch_and_refused_arguments_leave_the_library_usable(gpu, refs):
    """Through ctypes, since ffi.py cannot express these.  Each refusal returns 2; the valid call after it equals the reference."""
    xy, att = gpu.hash_to_g2_direct(SIG, [])
    assert xy.shape == (0, 24) and att.shape == (0,)
    lib = gpu.lib()
    msgs, extras = refs.master[0][:5], refs.master[1][:5]
    want = refs.direct[False].rows()
    moff = np.concatenate([[0], np.cumsum([len(m) for m in msgs])]).astype(np.uint64)
    eoff = np.concatenate([[0], np.cumsum([len(e) for e in extras])]).astype(np.uint64)
    mdat, edat, dom = _u8(b"".join(msgs)), _u8(b"".join(extras)), _u8(SIG)
    assert moff[5] > 0 and eoff[5] > 0
    entries = [("direct", lambda c, *a: lib.hash_to_g2_direct_bls12_377(*a[:6], C.c_int(c), *a[6:])),
               ("tail", lambda c, *a: lib.hash_to_g2_cip22_tail_bls12_377(*a[:6], C.c_int(c), *a[6:])),
               ("composite", lambda c, *a: lib.hash_to_g2_composite_bls12_377(*a[:6], C.c_int(0), C.c_int(c), *a[6:])),
               ("composite_cip22", lambda c, *a: lib.hash_to_g2_composite_bls12_377(*a[:6], C.c_int(1), C.c_int(c), *a[6:]))]

    def valid():
        _same(gpu.hash_to_g2_direct(SIG, msgs, extras), want, 0, 5)

    big = np.zeros(MAX_BYTES + 1, dtype=np.uint8)
    big_off = np.array([0, MAX_BYTES], dtype=np.uint64)               # counter || message: one byte beyond the table
    for mode, fn in entries:
        xy, att = np.zeros((5, 24), dtype=np.uint64), np.zeros(5, dtype=np.uint8)
        ok = (_vp(dom), _vp(mdat), _vp(moff), _vp(edat), _vp(eoff), C.c_size_t(5), _vp(xy), _vp(att))
        down = moff.copy()
        down[2], down[3] = moff[3] + 1, moff[2]
        for what, args in (("domain NULL", (None,) + ok[1:]), ("offsets decreasing", ok[:2] + (_vp(down),) + ok[3:]),
                           ("message bytes NULL", ok[:1] + (None,) + ok[2:]), ("extra bytes NULL", ok[:3] + (None,) + ok[4:]),
                           ("offsets NULL", ok[:2] + (None,) + ok[3:]), ("outputs NULL", ok[:6] + (None, None))):
            assert fn(0, *args) == 2, (mode, what)
            valid()
        for bad in (2, -1):
            assert fn(bad, *ok) == 2, (mode, "compat", bad)
        valid()
        assert fn(0, None, None, None, None, None, C.c_size_t(0), None, None) == 0, mode                  # nothing to do
        if mode.startswith("composite"):
            big_len = big_off if mode == "composite" else np.array([0, MAX_BYTES + 1], dtype=np.uint64)
            assert fn(0, _vp(dom), _vp(big), _vp(big_len), None, None, C.c_size_t(1), _vp(xy), _vp(att)) == 2, (mode, "over-long string")
            valid()
        # all-empty messages with a NULL data pointer and no extras
        zero = np.zeros(6, dtype=np.uint64)
        w = g2.reference(mode, SIG, b"", b"")
        xy[:], att[:] = 0, 0
        assert fn(0, _vp(dom), None, _vp(zero), None, None, C.c_size_t(5), _vp(xy), _vp(att)) == 0, mode
        assert (xy == g2.rows_of([w[0]])[0]).all() and (att == w[1]).all(), mode
    assert lib.celo_amd_hash_g2_last_split(None) == 2
    valid()


# ---- G1 and G2 share the scratch, the stream and the mutex
def test_g1_and_g2_calls_alternate_on_the_shared_scratch(gpu, refs):
    """a G1 call, a larger G2 call, the same G1 call again: each equals its reference and the two G1 results are identical"""
    a = gpu.hash_to_g1_direct(SIG, *refs.g1)
    _same_g1(a, refs.g1_ref.rows())
    _same(gpu.hash_to_g2_direct(SIG, *refs.master), refs.direct[False].rows())
    b = gpu.hash_to_g1_direct(SIG, *refs.g1)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    _same(gpu.hash_to_g2_direct(SIG, refs.master[0][:3], refs.master[1][:3]), refs.direct[False].rows(), 0, 3)


def _same_g1(got, want):
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])


def test_two_threads_one_group_each(gpu, refs):
    """two callers at once (the library serialises them on its hash mutex), four calls each: every result equals the reference"""
    errors = []

    def run_g1():
        try:
            for _ in range(4):
                _same_g1(gpu.hash_to_g1_direct(SIG, *refs.g1), refs.g1_ref.rows())
        except BaseException as e:                                           # reported by the main thread
            errors.append(("g1", repr(e)))

    def run_g2():
        try:
            for _ in range(4):
                _same(gpu.hash_to_g2_direct(SIG, *refs.master, compat=1), refs.direct[True].rows())
        except BaseException as e:
            errors.append(("g2", repr(e)))

    threads = [threading.Thread(target=run_g1), threading.Thread(target=run_g2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert errors == []


@pytest.mark.parametrize("compat", [0, 1])
def test_composite_cip22_is_the_crh_followed_by_the_tail(gpu, compat):
    """three messages: hash_to_g2_composite(cip22) == composite_crh -> hash_to_g2_cip22_tail, rows and attempts byte for byte"""
    msgs, extras = [b"", b"a", b"hash step " * 20], [b"x", b"", b"extra data"]
    for ex in (extras, None):
        xy, att = gpu.hash_to_g2_composite(SIG, msgs, ex, cip22=True, compat=compat)
        txy, tatt = gpu.hash_to_g2_direct(SIG, gpu.composite_crh(msgs), ex, cip22_tail=True, compat=compat)
        assert (att != 255).all() and np.array_equal(att, tatt) and np.array_equal(xy, txy)
