"""CPU (-m "not gpu"): batched variable-base scalar multiplication (csrc/var_base.h) through the host twins of host_test.cpp under bounds
tracking - the per-lane table, the plain ladder, the subgroup (GLV) ladder and the shared-scalar form that the kernels of unit_varbase.hip
run, over the same lane-interleaved workspace - on the cases of tests/scalar_mul_cases.py: plain against the oracle, GLV against plain,
shared scalar against per-row.  Whole outputs, limb for limb, flags included."""
import ctypes as C
import numpy as np
import pytest
from oracle import cpu_oracle as co
import scalar_mul_cases as sc
from helpers import build_hosttest


@pytest.fixture(scope="module")
def ht():
    lib = C.CDLL(build_hosttest())
    lib.ht_var_base_table.restype = None
    lib.ht_var_base_mul.restype = None
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_mul(ht, name, xy, inf, scalars, c, glv=False):
    g = sc.group(name)
    xy = np.ascontiguousarray(xy, dtype=np.uint64).reshape(-1, g.aw)
    s = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, g.sw)
    n = xy.shape[0]
    out = np.full((n, g.aw), 0xA5, dtype=np.uint64)
    oinf = np.full(n, 9, dtype=np.uint8)
    ht.ht_var_base_mul(C.c_int(g.gid), C.c_int(1 if glv else 0), _p(xy), _p(inf), _p(s), C.c_size_t(s.shape[0]), C.c_size_t(n), C.c_int(c), _p(out), _p(oinf))
    return out, oinf


def _same(got, want, labels=None):
    bad = [i for i in range(len(want[1])) if got[1][i] != want[1][i] or not np.array_equal(got[0][i], want[0][i])]
    assert not bad, [(i, labels[i] if labels else None) for i in bad[:5]]


@pytest.mark.parametrize("c", [2, 4, 5, 8])
@pytest.mark.parametrize("name", sc.GROUPS)
def test_table_of_one_point(ht, name, c):
    """[e + 1]P for e < 2^(c-1): a subgroup point, every low-order point (identity entries at the multiples of its order), the identity"""
    g = sc.group(name)
    H = 1 << (c - 1)
    for P, order in [(sc.subgroup_points(name)[1], None)] + [(P, o) for _, P, o in sc.low_order_points(name)] + [(None, 1)]:
        xy, inf = g.pack([P])
        out = np.full((H, g.aw), 0xA5, dtype=np.uint64)
        oinf = np.full(H, 9, dtype=np.uint8)
        ht.ht_var_base_table(C.c_int(g.gid), _p(xy), C.c_int(int(inf[0])), C.c_int(c), _p(out), _p(oinf))
        want = g.pack([g.E.mul(P, e + 1) for e in range(H)])
        _same((out, oinf), want)
        if order:
            assert oinf.tolist() == [1 if (e + 1) % order == 0 else 0 for e in range(H)]


@pytest.mark.parametrize("c", sc.WINDOWS)
@pytest.mark.parametrize("name", sc.GROUPS)
def test_plain_ladder_matches_the_oracle(ht, name, c):
    b = sc.case_batch(name)
    _same(host_mul(ht, name, b.xy, b.inf, b.sc, c), sc.expected(name), b.labels)


@pytest.mark.parametrize("c", sc.WINDOWS)
def test_glv_ladder_matches_the_plain_ladder(ht, c):
    name = "bls12_377_g1"
    b = sc.case_batch(name)
    keep = [i for i in range(b.n) if not b.plain_only[i]]
    s = b.take(keep)
    plain = host_mul(ht, name, s.xy, s.inf, s.sc, c)
    _same(plain, (sc.expected(name)[0][keep], sc.expected(name)[1][keep]), s.labels)
    _same(host_mul(ht, name, s.xy, s.inf, s.sc, c, glv=True), plain, s.labels)


@pytest.mark.parametrize("name", sc.GROUPS)
def test_shared_scalar_matches_per_row(ht, name):
    g = sc.group(name)
    b = sc.case_batch(name)
    for k in (g.r - 1, dict(sc.scalar_list(name))["uniform 3"], 0):
        one = co.ints_to_limbs([k], g.sw)
        per_row = host_mul(ht, name, b.xy, b.inf, np.repeat(one, b.n, axis=0), 4)
        _same(host_mul(ht, name, b.xy, b.inf, one, 4), per_row, b.labels)
        _same(per_row, sc.oracle_rows(name, b.xy, b.inf, one), b.labels)
    if name == "bls12_377_g1":
        keep = [i for i in range(b.n) if not b.plain_only[i]]
        s = b.take(keep)
        one = co.ints_to_limbs([g.r - 2], g.sw)
        _same(host_mul(ht, name, s.xy, s.inf, one, 5, glv=True), sc.oracle_rows(name, s.xy, s.inf, one), s.labels)
