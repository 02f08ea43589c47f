"""GPU: masked segmented point sums aggregate_by_bitmap_* / _dev (csrc/unit_seals.hip) for BLS12-377 G1 and G2 on the cases of
tests/aggregate_cases.py.  Expected sums: oracle/py/ecc.py, computed once per (key list, bitmap); every comparison is on whole outputs - rows
limb for limb, identity flags and counts."""
import threading
import numpy as np
import pytest
import torch  # before the library: both must share one HIP runtime
import aggregate_cases as ac

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(autouse=True)
def _default_hooks(gpu):
    try:
        yield
    finally:
        gpu.set_aggregate_lanes(0)
        gpu.set_aggregate_complement(-1)


def _same(got, want, labels):
    assert len(got[1]) == len(labels) == len(want[1])
    bad = [labels[i] for i in range(len(labels)) if got[1][i] != want[1][i] or got[2][i] != want[2][i] or not np.array_equal(got[0][i], want[0][i])]
    assert not bad, bad[:5]


def _shared(gpu, name, pts, bitmaps):
    xy, inf = ac.pack_keys(name, pts)
    return gpu.aggregate_by_bitmap(name, xy, inf, [0, len(pts)], np.stack(bitmaps).reshape(len(bitmaps), len(pts)))


def _per_seal(gpu, name, sets):
    """sets: [(points, bitmap)], each seal with rows of its own"""
    xy, inf = ac.pack_keys(name, tuple(P for ps, _ in sets for P in ps))
    off = np.cumsum([0] + [len(ps) for ps, _ in sets]).astype(np.uint32)
    bits = np.concatenate([np.asarray(b, dtype=np.uint8) for _, b in sets] + [np.zeros(0, dtype=np.uint8)])
    return gpu.aggregate_by_bitmap(name, xy, inf, off, bits)


def _expected_sets(name, sets):
    rows, flags = ac.group(name).pack([ac.oracle_sum(name, ps, b) for ps, b in sets])
    return rows, flags, np.array([int(np.count_nonzero(b)) for _, b in sets], dtype=np.uint32)


@pytest.mark.parametrize("n", ac.SET_SIZES)
@pytest.mark.parametrize("name", ac.GROUPS)
def test_set_sizes_and_patterns(gpu, name, n):
    """every pattern over one set of n keys: as one shared-set call (lane width and side by rule) and as per-seal sets of n rows each"""
    pts = ac.keys(name, n)
    pats = ac.patterns(n)
    labels = ["n=%d %s" % (n, label) for label, _ in pats]
    want = ac.expected(name, pts, [b for _, b in pats])
    _same(_shared(gpu, name, pts, [b for _, b in pats]), want, labels)
    assert gpu.seals_last()["path"] == -1 and gpu.seals_last()["lanes"] in ac.LANES
    _same(_per_seal(gpu, name, [(pts, b) for _, b in pats]), want, labels)


@pytest.mark.parametrize("lanes", ac.LANES)
@pytest.mark.parametrize("name", ac.GROUPS)
def test_every_lane_width_and_complement(gpu, name, lanes):
    """n = 100 and 65 under each lane width, the complement by rule, never and always: identical rows, the oracle's"""
    gpu.set_aggregate_lanes(lanes)
    for n in (100, 65):
        pts = ac.keys(name, n)
        pats = ac.patterns(n)
        want = ac.expected(name, pts, [b for _, b in pats])
        for complement in (-1, 0, 1):
            gpu.set_aggregate_complement(complement)
            _same(_shared(gpu, name, pts, [b for _, b in pats]), want, ["n=%d L=%d c=%d %s" % (n, lanes, complement, label) for label, _ in pats])
            assert gpu.seals_last()["lanes"] == lanes


@pytest.mark.parametrize("lanes", ac.LANES)
@pytest.mark.parametrize("name", ac.GROUPS)
def test_special_key_lists(gpu, name, lanes):
    """duplicates, P and -P, P, P, -2P, flagged rows, sums that are the identity: ragged per-seal sets in one call, and each list as a shared
    set with the complement never and always"""
    gpu.set_aggregate_lanes(lanes)
    cases = ac.special_key_lists(name)
    sets = [(ps, b) for _, ps, b, _ in cases]
    want = _expected_sets(name, sets)
    assert want[1].tolist() == [1 if ident else 0 for _, _, _, ident in cases]
    _same(_per_seal(gpu, name, sets), want, [label for label, _, _, _ in cases])
    for complement in (0, 1):
        gpu.set_aggregate_complement(complement)
        for i, (label, ps, b, _) in enumerate(cases):
            _same(_shared(gpu, name, ps, [b]), tuple(w[i:i + 1] for w in want), ["%s shared c=%d" % (label, complement)])


def _seeded_bitmaps(m, n, seed):
    rng = np.random.default_rng(seed)
    bits = (rng.random((m, n)) < 0.7).astype(np.uint8)
    bits[bits != 0] = rng.integers(1, 256, size=int(np.count_nonzero(bits)), dtype=np.uint8)
    return bits


@pytest.mark.parametrize("m", ac.SEAL_COUNTS)
@pytest.mark.parametrize("name", ac.GROUPS)
def test_seal_counts_shared_and_ragged(gpu, name, m):
    """m seals over one shared set of 9 keys, and m ragged per-seal sets of 0 .. 12 rows with an empty set in the middle"""
    pts = ac.keys(name, 9)
    bits = _seeded_bitmaps(m, 9, 50 + m)
    _same(_shared(gpu, name, pts, list(bits)), ac.expected(name, pts, list(bits)), ["seal %d" % i for i in range(m)])
    pool = ac.keys(name, 100)
    rng = np.random.default_rng(60 + m)
    sizes = rng.integers(0, 13, size=m).tolist()
    sizes[m // 2] = 0
    sets = []
    for i, k in enumerate(sizes):
        lo = int(rng.integers(0, 100 - 12))
        sets.append((pool[lo:lo + k], _seeded_bitmaps(1, k, 1000 * m + i)[0]))
    _same(_per_seal(gpu, name, sets), _expected_sets(name, sets), ["set %d of %d rows" % (i, k) for i, k in enumerate(sizes)])


@pytest.mark.parametrize("name", ac.GROUPS)
def test_dev_form_matches_the_host_form(gpu, name):
    g = ac.group(name)
    m, n = 65, 100
    pts = ac.keys(name, n)
    xy, inf = ac.pack_keys(name, pts)
    inf[17] = 1                                     # a flagged row: adds nothing, still counts
    bits = _seeded_bitmaps(m, n, 77)
    host = gpu.aggregate_by_bitmap(name, xy, inf, [0, n], bits)
    flagged = tuple(None if j == 17 else P for j, P in enumerate(pts))
    first =g.pack([ac.oracle_sum(name, flagged, b) for b in bits[:3]])
    assert np.array_equal(host[0][:3], first[0]) and host[2].tolist() == [int(np.count_nonzero(b)) for b in bits]
    d_xy = torch.from_numpy(xy.view(np.int64).copy()).cuda()
    d_inf = torch.from_numpy(inf.copy()).cuda()
    d_bits = torch.from_numpy(bits.copy()).cuda()
    for with_count in (True, False):
        d_out = torch.full((m * g.aw,), SENTINEL, dtype=torch.int64, device="cuda")
        d_oinf = torch.full((m,), 9, dtype=torch.uint8, device="cuda")
        d_cnt = torch.full((m,), 9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rc = gpu.aggregate_by_bitmap_dev(name, d_xy.data_ptr(), d_inf.data_ptr(), [0, n], d_bits.data_ptr(), m, d_out.data_ptr(), d_oinf.data_ptr(),
                                         d_cnt.data_ptr() if with_count else 0)
        torch.cuda.synchronize()
        assert rc == 0
        cnt = d_cnt.cpu().numpy().view(np.uint32)
        assert np.array_equal(d_out.cpu().numpy().view(np.uint64).reshape(m, g.aw), host[0]) and np.array_equal(d_oinf.cpu().numpy(), host[1])
        assert np.array_equal(cnt, host[2]) if with_count else (cnt == 9).all()
    # a refused device call writes nothing
    d_out = torch.full((m * g.aw,), SENTINEL, dtype=torch.int64, device="cuda")
    d_oinf = torch.full((m,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert gpu.aggregate_by_bitmap_dev(name, d_xy.data_ptr(), 0, [0, n, n], d_bits.data_ptr(), m, d_out.data_ptr(), d_oinf.data_ptr()) == 2
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy().view(np.uint64) == SENTINEL).all() and (d_oinf.cpu().numpy() == 9).all()


@pytest.mark.parametrize("name", ac.GROUPS)
def test_one_bitmap_changes_one_row(gpu, name):
    m, n = 65, 100
    pts = ac.keys(name, n)
    bits = _seeded_bitmaps(m, n, 78)
    before = _shared(gpu, name, pts, list(bits))
    for seal in (0, 40, 64):
        changed = bits.copy()
        changed[seal, (7 * seal) % n] = 0 if changed[seal, (7 * seal) % n] else 1
        after = _shared(gpu, name, pts, list(changed))
        others = [i for i in range(m) if i != seal]
        assert np.array_equal(after[0][others], before[0][others]) and np.array_equal(after[1][others], before[1][others])
        assert np.array_equal(after[2][others], before[2][others])
        want = ac.expected(name, pts, [changed[seal]])
        assert np.array_equal(after[0][seal], want[0][0]) and not np.array_equal(after[0][seal], before[0][seal]) and after[2][seal] == want[2][0]


def test_two_threads_calling_concurrently(gpu):
    """two host threads, both groups, shared and per-seal forms at once: every result is the oracle's"""
    work_items = {}
    for name in ac.GROUPS:                          # the references first, outside the threads
        pts = ac.keys(name, 65)
        pats = ac.patterns(65)
        work_items[name] = (pts, pats, ac.expected(name, pts, [b for _, b in pats]))
    errors = []

    def work(order):
        try:
            gpu.use_device(0)
            for name in order:
                pts, pats, want = work_items[name]
                labels = [label for label, _ in pats]
                _same(_shared(gpu, name, pts, [b for _, b in pats]), want, labels)
                _same(_per_seal(gpu, name, [(pts, b) for _, b in pats]), want, labels)
        except BaseException as e:      # noqa: BLE001  (reported by the main thread)
            errors.append(repr(e))
    threads = [threading.Thread(target=work, args=(o,)) for o in (ac.GROUPS, ac.GROUPS[::-1])]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_last_call_record_and_the_lane_rule(gpu):
    """the width the rule picks: from the most rows a seal adds AFTER the side choice, and the number of seals"""
    name = "bls12_377_g1"
    pts = ac.keys(name, 100)
    all_but_one = dict(ac.patterns(100))["all but one"]
    _shared(gpu, name, pts, [all_but_one])                          # the complement: one row to add
    rec = gpu.seals_last()
    assert rec["lanes"] == 1 and rec["ms"]["sums"] > 0 and rec["ms"]["wall"] >= rec["ms"]["sums"]
    gpu.set_aggregate_complement(0)
    _shared(gpu, name, pts, [all_but_one])                          # 99 rows: 32 lanes of 4
    assert gpu.seals_last()["lanes"] == 32


@pytest.mark.parametrize("m", [1, 65])
@pytest.mark.parametrize("name", ac.GROUPS)
def test_host_and_device_forms_with_and_without_flags(gpu, name, m):
    """m = 1 and one seal past a 64-lane workgroup over 9 keys without an identity: flags of zero and no flags at all, host and device
    forms - four times the same rows, flags and counts"""
    g = ac.group(name)
    n = 9
    xy, inf = ac.pack_keys(name, ac.keys(name, n))
    assert not inf.any()
    bits = _seeded_bitmaps(m, n, 300 + m)
    want = gpu.aggregate_by_bitmap(name, xy, inf, [0, n], bits)
    none = gpu.aggregate_by_bitmap(name, xy, None, [0, n], bits)
    assert all(np.array_equal(a, b) for a, b in zip(none, want))
    d_xy = torch.from_numpy(xy.view(np.int64).copy()).cuda()
    d_inf = torch.from_numpy(inf.copy()).cuda()
    d_bits = torch.from_numpy(bits.copy()).cuda()
    for flags in (d_inf.data_ptr(), 0):
        d_out = torch.full((m * g.aw,), SENTINEL, dtype=torch.int64, device="cuda")
        d_oinf = torch.full((m,), 9, dtype=torch.uint8, device="cuda")
        d_cnt = torch.full((m,), 9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert gpu.aggregate_by_bitmap_dev(name, d_xy.data_ptr(), flags, [0, n], d_bits.data_ptr(), m, d_out.data_ptr(), d_oinf.data_ptr(), d_cnt.data_ptr()) == 0
        torch.cuda.synchronize()
        got = (d_out.cpu().numpy().view(np.uint64).reshape(m, g.aw), d_oinf.cpu().numpy(), d_cnt.cpu().numpy().view(np.uint32))
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
