"""CPU (-m "not gpu"): the masked segmented point sums of csrc/aggregate.h through the host twin of host_test.cpp under bounds tracking - the
lane loop, the fold rounds and the complement that k_seal_count / k_masked_sum of unit_seals.hip run - limb for limb against oracle/py/ecc.py:
both groups, every lane width, the complement off, on and by rule, on the bitmap patterns and key lists of tests/aggregate_cases.py."""
import ctypes as C
import numpy as np
import pytest
import aggregate_cases as ac
from helpers import build_hosttest


@pytest.fixture(scope="module")
def ht():
    lib = C.CDLL(build_hosttest())
    lib.ht_aggregate_by_bitmap.restype = None
    lib.ht_aggregate_pick_lanes.restype = C.c_uint32
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_sums(ht, name, xy, inf, offsets, bits, m, lanes, complement):
    g = ac.group(name)
    off = np.ascontiguousarray(offsets, dtype=np.uint32)
    xy = np.ascontiguousarray(xy, dtype=np.uint64).reshape(-1, g.aw)
    if xy.shape[0] == 0:
        xy = np.zeros((1, g.aw), dtype=np.uint64)
    b = np.ascontiguousarray(bits, dtype=np.uint8).reshape(-1)
    if b.size == 0:
        b = np.zeros(1, dtype=np.uint8)
    out = np.full((m, g.aw), 0xA5, dtype=np.uint64)
    oinf = np.full(m, 9, dtype=np.uint8)
    cnt = np.full(m, 0xA5A5A5A5, dtype=np.uint32)
    ht.ht_aggregate_by_bitmap(C.c_int(g.gid), _p(xy), _p(inf), _p(off), C.c_size_t(off.shape[0] - 1), _p(b), C.c_size_t(m), C.c_int(lanes), C.c_int(complement),
                              _p(out), _p(oinf), _p(cnt))
    return out, oinf, cnt


def _same(got, want, labels):
    bad = [labels[i] for i in range(len(labels)) if got[1][i] != want[1][i] or got[2][i] != want[2][i] or not np.array_equal(got[0][i], want[0][i])]
    assert not bad, bad[:5]


@pytest.mark.parametrize("complement", [0, 1, -1])
@pytest.mark.parametrize("lanes", ac.LANES)
@pytest.mark.parametrize("name", ac.GROUPS)
def test_shared_set_patterns_match_the_oracle(ht, name, lanes, complement):
    """one shared set, one seal per pattern; set sizes below, at and past a lane width"""
    for n in (0, 1, 2, 7, 9, 65):
        pts = ac.keys(name, n)
        pats = ac.patterns(n)
        xy, inf = ac.pack_keys(name, pts)
        bits = np.stack([b for _, b in pats])
        got = host_sums(ht, name, xy, None, [0, n], bits, len(pats), lanes, complement)
        _same(got, ac.expected(name, pts, [b for _, b in pats]), ["n=%d %s" % (n, label) for label, _ in pats])


@pytest.mark.parametrize("lanes", ac.LANES)
@pytest.mark.parametrize("name", ac.GROUPS)
def test_special_key_lists(ht, name, lanes):
    """duplicates, a key and its negative, P, P, -2P, flagged rows: as per-seal sets (ragged, one call) and each as a shared set under the
    complement"""
    cases = ac.special_key_lists(name)
    pts = tuple(P for _, ps, _, _ in cases for P in ps)
    xy, inf = ac.pack_keys(name, pts)
    off = np.cumsum([0] + [len(ps) for _, ps, _, _ in cases]).astype(np.uint32)
    bits = np.concatenate([b for _, _, b, _ in cases])
    rows, flags = ac.group(name).pack([ac.oracle_sum(name, ps, b) for _, ps, b, _ in cases])
    want = (rows, flags, np.array([np.count_nonzero(b) for _, _, b, _ in cases], dtype=np.uint32))
    assert flags.tolist() == [1 if ident else 0 for _, _, _, ident in cases]
    labels = [label for label, _, _, _ in cases]
    _same(host_sums(ht, name, xy, inf, off, bits, len(cases), lanes, -1), want, labels)
    for i, (label, ps, b, _) in enumerate(cases):
        for complement in (0, 1):
            got = host_sums(ht, name, xy, inf, [off[i], off[i + 1]], b[None, :], 1, lanes, complement)
            _same(got, tuple(w[i:i + 1] for w in want), [label + " shared, complement %d" % complement])


@pytest.mark.parametrize("name", ac.GROUPS)
def test_ragged_sets_with_an_empty_one_and_the_lane_rule(ht, name):
    """per-seal sets of 5, 0, 66 and 1 rows, lanes by rule; and the rule itself at its borders"""
    sizes = [5, 0, 66, 1]
    pts = ac.keys(name, sum(sizes))
    xy, inf = ac.pack_keys(name, pts)
    off = np.cumsum([0] + sizes).astype(np.uint32)
    rng = np.random.default_rng(3)
    bits = (rng.random(sum(sizes)) < 0.7).astype(np.uint8)
    segs = [(pts[off[i]:off[i + 1]], bits[off[i]:off[i + 1]]) for i in range(len(sizes))]
    rows, flags = ac.group(name).pack([ac.oracle_sum(name, ps, b) for ps, b in segs])
    want = (rows, flags, np.array([np.count_nonzero(b) for _, b in segs], dtype=np.uint32))
    _same(host_sums(ht, name, xy, None, off, bits, len(sizes), 0, -1), want, ["set of %d" % s for s in sizes])
    pick = lambda a, m: ht.ht_aggregate_pick_lanes(C.c_uint32(a), C.c_size_t(m))
    assert [pick(a, 1) for a in (0, 1, 4, 5, 8, 9, 128, 129, 256, 257, 1 << 20)] == [1, 1, 1, 2, 2, 4, 32, 64, 64, 64, 64]
    assert [pick(1 << 20, m) for m in (1, 1024, 1025, 2048, 1 << 15, (1 << 16) - 1, 1 << 16, 1 << 24)] == [64, 64, 32, 32, 2, 1, 1, 1]
