"""GPU (-m gpu): batched hash-to-G1 over the direct hasher through the C ABI (include/celo_bls_amd.h:
hash_to_g1_direct_bls12_377) vs the oracle's restatement (oracle/py/hashing.py: hash_to_g1_direct) - SURVEY.md section 8f
row f1.

What it replaces: TryAndIncrement<DirectHasher, G1>::hash_with_attempt (crates/bls-crypto/src/hash_to_curve/
try_and_increment.rs:87-139, hashers/direct.rs:23-80), one call per message in Signature::batch_verify
(bls/signature.rs:111-114).  The reference holds vectors for Blake2s / the XOF (hashers/direct.rs:88-172, pinned in
tests/test_oracle_golden.py and tests/test_seam_a.py) and for the composite hash-to-curve, none for a direct-hasher point:
the oracle is the checker here.  Byte and integer work: bit-exact, including the attempt counter.

Beyond the first three tests the module follows the code's own shapes (csrc/unit_hash.hip): rounds 1, 2, 4, 8 and 16 counters wide, chosen
from the number of messages still open, so batches on both sides of 8192, 16 384, 32 768 and 65 536 messages, the benchmark's own 2^16
inputs, the CIP22 tail and both composite modes over lengths and at scale, the bulk Pedersen CRH over the whole generator table, call
sequences over the shared grow-only scratch, refused arguments and concurrent callers.  Every comparison is of WHOLE outputs with the
Python oracle (tests/hash_ref.py evaluates it on worker processes, all batches started when the first test asks for one); no sampling, no
tolerance.  Not covered: counter exhaustion (attempts = 255) - no findable input reaches it and there is no hook to force it; the
identity branch of the cofactor multiple is tested on the host build (tests/test_hash_host.py)."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch  # before the library: both must share one HIP runtime
from oracle.py import ecc, hashing as hs
from oracle import cpu_oracle as co
import hash_ref as hr

pytestmark = pytest.mark.gpu
SIG, POP = b"ULforxof", b"ULforpop"


def _want(dom, msgs, extras):
    pts, att = [], []
    for m, e in zip(msgs, extras):
        P, c = hs.hash_to_g1(dom, m, e, composite=False)
        pts.append(P)
        att.append(c)
    return co.pack_g1_377(pts)[0], att


def test_message_lengths_around_the_block_size(gpu):
    """counter || extra || message lengths 1 ... 200 cross the 64-byte Blake2s block boundary at every residue (incl. the
    exact multiples, where the final block is full), with and without extra data"""
    rng = np.random.default_rng(5)
    msgs = [bytes(rng.integers(0, 256, size=l, dtype=np.uint8)) for l in list(range(0, 70)) + [126, 127, 128, 129, 191, 192, 200]]
    extras = [bytes(rng.integers(0, 256, size=(i * 7) % 40, dtype=np.uint8)) for i in range(len(msgs))]
    for dom in (SIG, POP):
        xy, att = gpu.hash_to_g1_direct(dom, msgs, extras)
        wxy, watt = _want(dom, msgs, extras)
        assert att.tolist() == watt and np.array_equal(xy, wxy)
    xy, att = gpu.hash_to_g1_direct(SIG, msgs)                         # extra_off == NULL
    wxy, watt = _want(SIG, msgs, [b""] * len(msgs))
    assert att.tolist() == watt and np.array_equal(xy, wxy)
    assert max(watt) >= 2                                             # several counters were needed somewhere


def test_points_are_in_the_subgroup_and_distinct(gpu):
    msgs = [b"epoch %d" % i for i in range(300)]
    xy, att = gpu.hash_to_g1_direct(SIG, msgs, [b"\x01\x02"] * 300)
    assert (att < 255).all()
    vals = co.from_mont(xy.reshape(-1, 6), ecc.Q377)
    pts = [(vals[2 * i], vals[2 * i + 1]) for i in range(300)]
    assert len(set(pts)) == 300
    for P in pts[:16]:
        assert ecc.E1_377.on_curve(P) and ecc.E1_377.in_subgroup(P)
    wxy, watt = _want(SIG, msgs[:24], [b"\x01\x02"] * 24)
    assert np.array_equal(xy[:24], wxy) and att[:24].tolist() == watt


def test_empty_batch(gpu):
    xy, att = gpu.hash_to_g1_direct(SIG, [])
    assert xy.shape == (0, 12) and att.shape == (0,)


# ======================================================================================================================================
# Whole batches against the oracle.  The inputs are seeded and built here; the reference rows come from tests/hash_ref.py.
N_MASTER = 65537 + 1024
PREFIXES = (1, 2, 63, 64, 65, 4097, 8192, 8193, 16384, 16385, 32768, 32769, 65536, 65537, N_MASTER)
SLICE = (12345, 12345 + 20000)                                  # one call that does not start at message 0 (first round 4 wide)
BENCH_HISTOGRAM = [27508, 16020, 9157, 5394, 3074, 1838, 1064, 627, 358, 228, 103, 67, 46, 23, 11, 9, 4, 2, 2, 0, 1]
MAX_BYTES = hr.PEDERSEN_MAX_BYTES                               # 19 530 = 52 080 chunks of 3 bits exactly
N_CHUNKS = MAX_BYTES * 8 // 3


def _varied(seed, n, max_len, max_extra):
    """n messages of 0 ... max_len bytes with extras of 0 ... max_extra bytes"""
    rng = np.random.default_rng(seed)
    ml, el = rng.integers(0, max_len + 1, size=n), rng.integers(0, max_extra + 1, size=n)
    md, ed = rng.integers(0, 256, size=int(ml.sum()), dtype=np.uint8).tobytes(), rng.integers(0, 256, size=int(el.sum()), dtype=np.uint8).tobytes()
    mo, eo = np.concatenate([[0], np.cumsum(ml)]), np.concatenate([[0], np.cumsum(el)])
    return [md[mo[i]:mo[i + 1]] for i in range(n)], [ed[eo[i]:eo[i + 1]] for i in range(n)]


def _fixed(seed, n, length):
    a = np.random.default_rng(seed).integers(0, 256, size=(n, length), dtype=np.uint8)
    return [a[i].tobytes() for i in range(n)]


def bench_inputs():
    """bench.py's wire leg, restated: default_rng(0x5EED0007), 2^16 messages of 32 bytes, extra 01 02 for each"""
    n = 1 << 16
    hm = np.random.default_rng(0x5EED0007).integers(0, 256, size=(n, 32), dtype=np.uint8)
    return [hm[i].tobytes() for i in range(n)], [b"\x01\x02"] * n


def table_messages():
    """Four messages of the maximum length, bit by bit: chunk k of message s has low two bits (k + s) mod 4 (the table multiple it
    selects) and the sign bit set on even chunks in messages 0 and 2, on odd chunks in 1 and 3.  Each reads all 52 080 chunk positions;
    across the four every one of the 52 080 x 4 table entries is read exactly once."""
    out = []
    k = np.arange(N_CHUNKS)
    for s in range(4):
        v = (k + s) & 3
        bits = np.stack([v & 1, v >> 1, ((k & 1) == (s & 1)).astype(np.int64)], axis=1).reshape(-1).astype(np.uint8)
        out.append(np.packbits(bits, bitorder="little").tobytes())
    return out


class Refs:
    """Every input of the module and its reference, all started on the pool at once: the maximum-length hashes first (half a minute each in
    one worker, so they run beside the rest instead of after it), then the small sets, then the three sets of 2^16 messages."""
    def __init__(self):
        g = np.random.default_rng(0x6A1D)
        self.table_msgs = table_messages()
        self.table_short = [hr.rand_bytes(g, l) for l in (0, 1, 5, 40, 200, 3, 1000, 17)]
        self.max_msg, self.max_extra = hr.rand_bytes(g, MAX_BYTES - 1 - 9), hr.rand_bytes(g, 9)
        self.table = hr.CrhBatch(self.table_msgs, per=1)
        self.max_composite = hr.Batch("composite", SIG, [self.max_msg], [self.max_extra])

        self.tail_grid = hr.tail_length_grid(np.random.default_rng(0x7A11))
        self.tail_grid_ref = {(dom, ex): hr.Batch("tail", dom, [m for m, _ in self.tail_grid], [e if ex else b"" for _, e in self.tail_grid])
                              for dom in (SIG, POP) for ex in (True, False)}
        self.comp_grid = hr.composite_length_grid(np.random.default_rng(0xC0))
        self.comp_grid_ref = {mode: hr.Batch(mode, SIG, [m for m, _ in self.comp_grid], [e for _, e in self.comp_grid]) for mode in ("composite", "composite_cip22")}
        self.comp300 = (_fixed(0x5EED0004, 300, 32), _varied(0x5EED0005, 300, 0, 5)[1])
        self.comp300_ref = hr.Batch("composite", SIG, *self.comp300)
        self.crh_lengths = [hr.rand_bytes(g, l) for l in list(range(71)) + [95, 96, 97, 200, 333, 400]]
        self.crh_lengths_ref = hr.CrhBatch(self.crh_lengths)
        self.indep = {mode: (_fixed(0x5EED0010 + i, 64, 48 if mode == "tail" else 32), _varied(0x5EED0020 + i, 64, 0, 4)[1]) for i, mode in enumerate(hr.MODES)}
        self.indep_ref = {mode: hr.Batch(mode, POP, *self.indep[mode]) for mode in hr.MODES}
        self.tail_big = (_fixed(0x5EED0002, 8193, 48), _varied(0x5EED0003, 8193, 0, 12)[1])
        self.tail_big_ref = hr.Batch("tail", SIG, *self.tail_big)
        self.cip22_big = (_varied(0x5EED0006, 8193, 40, 0)[0], _varied(0x5EED0008, 8193, 0, 6)[1])
        self.cip22_big_ref = hr.Batch("composite_cip22", SIG, *self.cip22_big)

        self.master = _varied(0x5EED0001, N_MASTER, 130, 40)
        self.direct = hr.Batch("direct", SIG, *self.master)
        self.bench = bench_inputs()
        self.bench_ref = hr.Batch("direct", SIG, *self.bench)
        self.crh_many = _varied(0x5EED0009, (1 << 16) + 1, 12, 0)[0]
        self.crh_many_ref = hr.CrhBatch(self.crh_many)


_REFS = None


@pytest.fixture(scope="module")
def refs():
    global _REFS
    if _REFS is None:
        _REFS = Refs()
    return _REFS


def _call(gpu, mode, dom, msgs, extras):
    if mode == "direct":
        return gpu.hash_to_g1_direct(dom, msgs, extras)
    if mode == "tail":
        return gpu.hash_to_g1_direct(dom, msgs, extras, cip22_tail=True)
    return gpu.hash_to_g1_composite(dom, msgs, extras, cip22=(mode == "composite_cip22"))


def _same(got, want, lo=0, hi=None):
    """every row and every counter, as integers"""
    (xy, att), (wxy, watt) = got, want
    assert np.array_equal(att, watt[lo:hi]), "counters differ at %s" % np.flatnonzero(att != watt[lo:hi])[:8]
    assert np.array_equal(xy, wxy[lo:hi]), "points differ at rows %s" % np.flatnonzero((xy != wxy[lo:hi]).any(axis=1))[:8]


def _direct_range(gpu, refs, lo, hi):
    """messages lo ... hi of the master set in one call: whole output, and the number of rounds the schedule predicts from the
    REFERENCE counters"""
    msgs, extras = refs.master
    want = refs.direct.rows()
    _same(gpu.hash_to_g1_direct(SIG, msgs[lo:hi], extras[lo:hi]), want, lo, hi)
    rounds = hr.round_widths(want[1][lo:hi])
    assert gpu.hash_last_rounds() == len(rounds), (gpu.hash_last_rounds(), rounds)
    return rounds


@pytest.mark.parametrize("n", PREFIXES)
def test_direct_prefixes_on_both_sides_of_every_width_boundary(gpu, refs, n):
    """The first n messages of one seeded set (lengths 0 ... 130, extras 0 ... 40: lanes of one wave need different numbers of Blake2s
    blocks).  The sizes sit on both sides of 8192, 16 384, 32 768 and 65 536, where the first round narrows from 16 to 8, 4, 2 and 1
    counters per message; the larger ones widen from round to round as messages drop out.  Every row, every counter."""
    rounds = _direct_range(gpu, refs, 0, n)
    first = {1: 16, 8192: 16, 8193: 8, 16384: 8, 16385: 4, 32768: 4, 32769: 2, 65536: 2, 65537: 1}.get(n)
    assert first is None or rounds[0][0] == first


def test_direct_slice_that_does_not_start_at_message_zero(gpu, refs):
    assert _direct_range(gpu, refs, *SLICE)[0][0] == 4


def test_every_round_width_ran_on_live_messages(gpu, refs):
    """The calls above ran the schedule this test derives from the reference counters (each asserted the library's round count against
    it).  If the lane budget or the widening rule changes, this fails: re-derive PREFIXES from the new rule instead of losing coverage.
    Required: each width 1, 2, 4, 8, 16 as a first round (no index list) on open messages; 2, 4, 8, 16 also as a later round (index
    list, after narrower rounds); and later rounds whose first counter is not a multiple of their width."""
    att = refs.direct.rows()[1]
    first, later, odd_base = set(), set(), set()
    for lo, hi in [(0, n) for n in PREFIXES] + [SLICE]:
        rounds = hr.round_widths(att[lo:hi])
        assert all(count >= 1 for _, count, _ in rounds)
        first.add(rounds[0][0])
        later |= {w for w, _, _ in rounds[1:]}
        odd_base |= {(w, base) for w, _, base in rounds[1:] if base % w}
    assert first == {1, 2, 4, 8, 16} and later >= {2, 4, 8, 16}, (first, later)
    assert len(odd_base) >= 3, odd_base


def test_the_benchmark_inputs_whole(gpu, refs):
    """bench.py's wire leg publishes hashes per second for exactly these inputs without comparing them with anything: here the whole
    output is.  The histogram of counters is a fact about the inputs derived on the CPU; it guards the test data (2, 4 and 16 wide
    rounds follow from it)."""
    want = refs.bench_ref.rows()
    assert np.bincount(want[1], minlength=21).tolist() == BENCH_HISTOGRAM
    assert float(want[1].mean()) + 1 == 2.384765625
    _same(gpu.hash_to_g1_direct(SIG, *refs.bench), want)
    assert [w for w, _, _ in hr.round_widths(want[1])] == [2, 4, 16] and gpu.hash_last_rounds() == 3


# ---- the streamed modes: lengths, then scale
def test_cip22_tail_lengths(gpu, refs):
    """inner of 48 bytes with extras of every length 0 ... 80, then inner lengths 0 ... 200; both domains; with the extras and without
    the extras pointer"""
    inners, extras = [m for m, _ in refs.tail_grid], [e for _, e in refs.tail_grid]
    for dom in (SIG, POP):
        _same(gpu.hash_to_g1_direct(dom, inners, extras, cip22_tail=True), refs.tail_grid_ref[dom, True].rows())
        _same(gpu.hash_to_g1_direct(dom, inners, None, cip22_tail=True), refs.tail_grid_ref[dom, False].rows())


def test_cip22_tail_batch_of_8193(gpu, refs):
    want = refs.tail_big_ref.rows()
    _same(gpu.hash_to_g1_direct(SIG, *refs.tail_big, cip22_tail=True), want)
    assert hr.round_widths(want[1])[0][0] == 8 and gpu.hash_last_rounds() == len(hr.round_widths(want[1]))


@pytest.mark.parametrize("mode", ["composite", "composite_cip22"])
def test_composite_lengths(gpu, refs, mode):
    """message lengths {0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 100} x extra lengths {0, 1, 7, 32}"""
    _same(_call(gpu, mode, SIG, [m for m, _ in refs.comp_grid], [e for _, e in refs.comp_grid]), refs.comp_grid_ref[mode].rows())


def test_composite_batch_of_300(gpu, refs):
    assert len(set(refs.comp300[0])) == 300
    _same(gpu.hash_to_g1_composite(SIG, *refs.comp300), refs.comp300_ref.rows())


def test_composite_at_the_maximum_length_and_one_byte_beyond(gpu, refs):
    """counter || extra || message of exactly 19 530 bytes fills the generator table: accepted, equal to the oracle.  One byte more: the
    reference panics, the library refuses the call - and goes on working."""
    assert 1 + len(refs.max_extra) + len(refs.max_msg) == MAX_BYTES
    _same(gpu.hash_to_g1_composite(SIG, [refs.max_msg], [refs.max_extra]), refs.max_composite.rows())
    with pytest.raises(RuntimeError):
        gpu.hash_to_g1_composite(SIG, [refs.max_msg + b"\0"], [refs.max_extra])
    with pytest.raises(RuntimeError):
        gpu.hash_to_g1_composite(SIG, [b"short", refs.max_msg], [b"", refs.max_extra + b"\0"])
    _same(gpu.hash_to_g1_composite(SIG, [refs.max_msg], [refs.max_extra]), refs.max_composite.rows())


def test_composite_cip22_batch_of_8193(gpu, refs):
    want = refs.cip22_big_ref.rows()
    _same(gpu.hash_to_g1_composite(SIG, *refs.cip22_big, cip22=True), want)
    assert hr.round_widths(want[1])[0][0] == 8


@pytest.mark.parametrize("mode", hr.MODES)
def test_batch_independence(gpu, refs, mode):
    """The same 64 messages as one call, as 64 calls of one, and at scattered positions among 5000 unrelated messages: identical rows.
    A consistency check ON TOP OF the comparison with the oracle (first assertion), not instead of it."""
    msgs, extras = refs.indep[mode]
    one = _call(gpu, mode, POP, msgs, extras)
    _same(one, refs.indep_ref[mode].rows())
    for i in range(64):
        xy, att = _call(gpu, mode, POP, msgs[i:i + 1], extras[i:i + 1])
        assert np.array_equal(xy[0], one[0][i]) and att[0] == one[1][i], i
    rng = np.random.default_rng(0x5CA7)
    pos = np.sort(rng.choice(5000, size=64, replace=False))
    big_m, big_e = _fixed(0x5EED0030, 5000, len(msgs[0])), _varied(0x5EED0031, 5000, 0, 4)[1]
    for p, m, e in zip(pos, msgs, extras):
        big_m[p], big_e[p] = m, e
    xy, att = _call(gpu, mode, POP, big_m, big_e)
    assert np.array_equal(xy[pos], one[0]) and np.array_equal(att[pos], one[1])


# ---- the bulk Pedersen CRH: lengths against the oracle, the whole generator table, more messages than one launch's 65 536 lanes
def test_pedersen_lengths_against_the_oracle(gpu, refs):
    """lengths 0 ... 70 and 95, 96, 97, 200, 333, 400 (tests/test_seam_a.py compares such lengths with the host build of the same header;
    here the checker is independent)"""
    assert gpu.composite_crh(refs.crh_lengths) == refs.crh_lengths_ref.hashes()


def test_pedersen_reads_every_entry_of_the_generator_table(gpu, refs):
    """52 080 chunks x 4 multiples (11.7 MB), built on the host: across four messages of the maximum length every entry is read exactly
    once, both signs at every position.  Submitted in one call between short messages, so lanes of one wave run very different loop
    lengths."""
    for s, m in enumerate(refs.table_msgs):
        assert len(m) == MAX_BYTES
    sel = np.zeros((N_CHUNKS, 4), dtype=np.int64)
    for m in refs.table_msgs:                                                 # the construction itself: one read per entry
        b = np.unpackbits(np.frombuffer(m, dtype=np.uint8), bitorder="little").reshape(N_CHUNKS, 3)
        sel[np.arange(N_CHUNKS), b[:, 0] + 2 * b[:, 1]] += 1
    assert (sel == 1).all()
    msgs = []
    for short, big in zip(refs.table_short[:4], refs.table_msgs):
        msgs += [short, big]
    msgs += refs.table_short[4:]
    got = gpu.composite_crh(msgs)
    assert [got[1], got[3], got[5], got[7]] == refs.table.hashes()
    assert [got[0], got[2], got[4], got[6]] + got[8:] == [hr.comp.composite_crh(m) for m in refs.table_short]


def test_pedersen_batch_of_65537(gpu, refs):
    """one message per lane across the 65 536 boundary of the launch; whole output against the (memoised) oracle, not a sample"""
    assert gpu.composite_crh(refs.crh_many) == refs.crh_many_ref.hashes()


# ---- call sequences, arguments, threads
def test_scratch_is_shared_and_grows_across_calls(gpu, refs):
    """The device scratch is grow-only and shared by the hash and the Pedersen entries: small, large, small again, Pedersen, composite,
    direct - each equal to the reference rows of the tests above."""
    msgs, extras = refs.master
    want = refs.direct.rows()
    for lo, hi in ((0, 3), (0, N_MASTER), (0, 3)):
        _same(gpu.hash_to_g1_direct(SIG, msgs[lo:hi], extras[lo:hi]), want, lo, hi)
    assert gpu.composite_crh(refs.crh_lengths) == refs.crh_lengths_ref.hashes()
    _same(gpu.hash_to_g1_composite(SIG, *refs.comp300), refs.comp300_ref.rows())
    _same(gpu.hash_to_g1_direct(SIG, msgs[5:9], extras[5:9]), want, 5, 9)
    _same(gpu.hash_to_g1_composite(SIG, *refs.cip22_big, cip22=True), refs.cip22_big_ref.rows())
    _same(gpu.hash_to_g1_direct(SIG, msgs[:70], extras[:70]), want, 0, 70)


def _u8(b):
    return np.frombuffer(b or b"\0", dtype=np.uint8)


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_refused_arguments_leave_the_library_usable(gpu, refs):
    """Through ctypes, since ffi.py cannot express these.  A refusal returns an error code; the valid call after it succeeds and equals
    the reference."""
    lib = gpu.lib()
    msgs, extras = refs.master[0][:5], refs.master[1][:5]
    want = refs.direct.rows()
    moff = np.concatenate([[0], np.cumsum([len(m) for m in msgs])]).astype(np.uint64)
    eoff = np.concatenate([[0], np.cumsum([len(e) for e in extras])]).astype(np.uint64)
    mdat, edat, dom = _u8(b"".join(msgs)), _u8(b"".join(extras)), _u8(SIG)
    assert moff[5] > 0 and eoff[5] > 0
    entries = [("direct", lambda *a: lib.hash_to_g1_direct_bls12_377(*a)), ("tail", lambda *a: lib.hash_to_g1_cip22_tail_bls12_377(*a)),
               ("composite", lambda *a: lib.hash_to_g1_composite_bls12_377(*a[:6], C.c_int(0), *a[6:])),
               ("composite_cip22", lambda *a: lib.hash_to_g1_composite_bls12_377(*a[:6], C.c_int(1), *a[6:]))]

    def valid():
        _same(gpu.hash_to_g1_direct(SIG, msgs, extras), want, 0, 5)

    for mode, fn in entries:
        xy, att = np.zeros((5, 12), dtype=np.uint64), np.zeros(5, dtype=np.uint8)
        ok = (_vp(dom), _vp(mdat), _vp(moff), _vp(edat), _vp(eoff), C.c_size_t(5), _vp(xy), _vp(att))
        down = moff.copy()
        down[2], down[3] = moff[3] + 1, moff[2]
        for what, args in (("domain NULL", (None,) + ok[1:]), ("offsets decreasing", ok[:2] + (_vp(down),) + ok[3:]),
                           ("message bytes NULL", ok[:1] + (None,) + ok[2:]), ("extra bytes NULL", ok[:3] + (None,) + ok[4:]),
                           ("offsets NULL", ok[:2] + (None,) + ok[3:]), ("outputs NULL", ok[:6] + (None, None))):
            assert fn(*args) != 0, (mode, what)
            valid()
        assert fn(None, None, None, None, None, C.c_size_t(0), None, None) == 0, mode                     # nothing to do
        # all-empty messages with a NULL data pointer; an extras pointer with every extra empty; neither pointer
        zero = np.zeros(6, dtype=np.uint64)
        w = hr.reference(mode, SIG, b"", b"")
        wrow = co.pack_g1_377([w[0]])[0][0]
        for args in ((_vp(dom), None, _vp(zero), _vp(edat), _vp(zero)), (_vp(dom), None, _vp(zero), None, _vp(zero)), (_vp(dom), None, _vp(zero), None, None)):
            xy[:], att[:] = 0, 0
            assert fn(*args, C.c_size_t(5), _vp(xy), _vp(att)) == 0, mode
            assert (xy == wrow).all() and (att == w[1]).all(), mode
    out = np.zeros((5, 48), dtype=np.uint8)
    for what, args in (("offsets NULL", (_vp(mdat), None)), ("offsets decreasing", (_vp(mdat), _vp(down))), ("bytes NULL", (None, _vp(moff)))):
        assert lib.composite_crh_bls12_377(*args, C.c_size_t(5), _vp(out)) != 0, what
        assert gpu.composite_crh(msgs) == [hr.comp.composite_crh(m) for m in msgs]
    assert lib.composite_crh_bls12_377(_vp(mdat), _vp(moff), C.c_size_t(5), None) != 0
    assert lib.composite_crh_bls12_377(None, None, C.c_size_t(0), None) == 0
    assert lib.composite_crh_bls12_377(None, _vp(zero), C.c_size_t(5), _vp(out)) == 0 and out.tobytes() == hr.comp.composite_crh(b"") * 5
    assert lib.celo_amd_hash_last_rounds(None) != 0
    valid()


def test_four_threads_one_mode_each(gpu, refs):
    """four callers at once (the library serialises them on its hash mutex), three calls each: every result equals the reference"""
    jobs = {"direct": ((refs.master[0][:3000], refs.master[1][:3000]), tuple(a[:3000] for a in refs.direct.rows())),
            "tail": (refs.tail_big, refs.tail_big_ref.rows()), "composite": (refs.comp300, refs.comp300_ref.rows()),
            "composite_cip22": (refs.cip22_big, refs.cip22_big_ref.rows())}
    errors = []

    def run(mode):
        try:
            (msgs, extras), want = jobs[mode]
            for _ in range(3):
                _same(_call(gpu, mode, SIG, msgs, extras), want)
        except BaseException as e:                                           # reported by the main thread
            errors.append((mode, repr(e)))

    threads = [threading.Thread(target=run, args=(mode,)) for mode in hr.MODES]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert errors == []
