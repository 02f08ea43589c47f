"""GPU: batched variable-base scalar multiplication scalar_mul_batch_* / _dev (csrc/unit_varbase.hip) for the four groups and the subgroup
(GLV) entry of BLS12-377 G1, on the cases of tests/scalar_mul_cases.py.  Expected rows: the CPU oracle (orc_mul_* + orc_normalize_*), computed
once per group; every comparison is on whole outputs, limb for limb, flags included."""
import ctypes as C
import threading
import numpy as np
import pytest
import torch  # before the library: both must share one HIP runtime
from oracle import cpu_oracle as co
import scalar_mul_cases as sc

pytestmark = pytest.mark.gpu
ENTRIES = [(name, False) for name in sc.GROUPS] + [("bls12_377_g1", True)]
IDS = [name + ("_subgroup" if sub else "") for name, sub in ENTRIES]
SEED, BIG = 4242, 257
SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(autouse=True)
def _default_hooks(gpu):
    yield
    gpu.set_scalar_mul_window(0)
    gpu.set_scalar_mul_chunk_rows(0)


def _same(got, want, labels=None):
    bad = [i for i in range(len(want[1])) if got[1][i] != want[1][i] or not np.array_equal(got[0][i], want[0][i])]
    assert not bad, [(i, labels[i] if labels else None) for i in bad[:5]]


def _cases(name, subgroup):
    """(batch, expected rows) of the case list; the subgroup entry takes the rows of subgroup points only"""
    b, (rows, inf) = sc.case_batch(name), sc.expected(name)
    if not subgroup:
        return b, (rows, inf)
    keep = [i for i in range(b.n) if not b.plain_only[i]]
    return b.take(keep), (rows[keep], inf[keep])


def _big(name):
    return sc.seeded_batch(name, BIG, SEED), sc.seeded_expected(name, BIG, SEED)


def _dev_call(gpu, name, subgroup, b, n_sc=None, sc_rows=None):
    g = sc.group(name)
    scal = b.sc if sc_rows is None else sc_rows
    d_xy = torch.from_numpy(b.xy.view(np.int64).copy()).cuda()
    d_inf = torch.from_numpy(b.inf.copy()).cuda()
    d_sc = torch.from_numpy(np.ascontiguousarray(scal).view(np.int64).copy()).cuda()
    d_out = torch.full((b.n * g.aw,), SENTINEL, dtype=torch.int64, device="cuda")
    d_oinf = torch.full((b.n,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = gpu.scalar_mul_batch_dev(name, d_xy.data_ptr(), d_inf.data_ptr(), d_sc.data_ptr(), scal.shape[0] if n_sc is None else n_sc, b.n, d_out.data_ptr(),
                                  d_oinf.data_ptr(), subgroup=subgroup)
    torch.cuda.synchronize()
    return rc, d_out.cpu().numpy().view(np.uint64).reshape(b.n, g.aw), d_oinf.cpu().numpy()


@pytest.mark.parametrize("name,subgroup", ENTRIES, ids=IDS)
def test_case_list_matches_the_oracle(gpu, name, subgroup):
    b, want = _cases(name, subgroup)
    _same(gpu.scalar_mul_batch(name, b.xy, b.inf, b.sc, subgroup=subgroup), want, b.labels)


@pytest.mark.parametrize("n", [1, 63, 64, 65, BIG])
@pytest.mark.parametrize("name,subgroup", ENTRIES, ids=IDS)
def test_batch_sizes_around_the_workgroup(gpu, name, subgroup, n):
    """n = 1, the workgroup size - 1, exact, + 1, and 257: prefixes of one seeded batch, so a row's result cannot depend on what follows it"""
    assert gpu.SCALAR_MUL_BLOCK == 64
    b, (rows, inf) = _big(name)
    s = b.take(range(n))
    _same(gpu.scalar_mul_batch(name, s.xy, s.inf, s.sc, subgroup=subgroup), (rows[:n], inf[:n]))
    if n == 1:                                                      # inf = NULL: no flags
        s2 = b.take([1])
        assert not s2.inf[0]
        _same(gpu.scalar_mul_batch(name, s2.xy, None, s2.sc, subgroup=subgroup), (rows[1:2], inf[1:2]))


@pytest.mark.parametrize("n", [63, 64, 65, 129])
@pytest.mark.parametrize("name,subgroup", ENTRIES, ids=IDS)
def test_chunk_border(gpu, name, subgroup, n):
    """chunks of 64 rows: below, at and just past one chunk, and two chunks and a row"""
    b, (rows, inf) = _big(name)
    gpu.set_scalar_mul_chunk_rows(64)
    lo = BIG - n                                                    # a suffix: the rows sit at other positions than in the size test
    s = b.take(range(lo, BIG))
    _same(gpu.scalar_mul_batch(name, s.xy, s.inf, s.sc, subgroup=subgroup), (rows[lo:], inf[lo:]))


@pytest.mark.parametrize("c", sc.WINDOWS)
@pytest.mark.parametrize("name,subgroup", ENTRIES, ids=IDS)
def test_every_window_width(gpu, name, subgroup, c):
    """the first 65 rows of the case list (the edge scalars, the window cases of every width, uniform values) under each accepted width"""
    b, (rows, inf) = _cases(name, subgroup)
    s = b.take(range(65))
    assert not any(s.plain_only)
    gpu.set_scalar_mul_window(c)
    _same(gpu.scalar_mul_batch(name, s.xy, s.inf, s.sc, subgroup=subgroup), (rows[:65], inf[:65]), s.labels)
    if not subgroup:                                               # the low-order points, whose tables hold identities, under this width
        t = b.take([i for i in range(b.n) if b.plain_only[i]])
        keep = [i for i in range(b.n) if b.plain_only[i]]
        _same(gpu.scalar_mul_batch(name, t.xy, t.inf, t.sc), (rows[keep], inf[keep]), t.labels)


@pytest.mark.parametrize("name,subgroup", ENTRIES, ids=IDS)
def test_dev_form_and_shared_scalar(gpu, name, subgroup):
    g = sc.group(name)
    b, want = _cases(name, subgroup)
    rc, out, oinf = _dev_call(gpu, name, subgroup, b)
    assert rc == 0
    _same((out, oinf), want, b.labels)
    # one scalar for every row == n copies of it (host and device forms), == the oracle
    for k in (g.r - 1, b.ks[40]):
        one = co.ints_to_limbs([k], g.sw)
        copies = np.repeat(one, b.n, axis=0)
        shared = gpu.scalar_mul_batch(name, b.xy, b.inf, one, subgroup=subgroup)
        _same(shared, gpu.scalar_mul_batch(name, b.xy, b.inf, copies, subgroup=subgroup), b.labels)
        _same(shared, sc.oracle_rows(name, b.xy, b.inf, one), b.labels)
        rc, out, oinf = _dev_call(gpu, name, subgroup, b, sc_rows=one)
        assert rc == 0
        _same((out, oinf), shared, b.labels)


@pytest.mark.parametrize("name,subgroup", ENTRIES, ids=IDS)
def test_rows_are_independent_of_neighbours_and_position(gpu, name, subgroup):
    b, (rows, inf) = _cases(name, subgroup)
    rng = np.random.default_rng(5)
    perm = rng.permutation(b.n).tolist()
    s = b.take(perm)
    _same(gpu.scalar_mul_batch(name, s.xy, s.inf, s.sc, subgroup=subgroup), (rows[perm], inf[perm]), s.labels)
    gpu.set_scalar_mul_chunk_rows(64)
    rev = list(range(b.n))[::-1]
    s = b.take(rev)
    _same(gpu.scalar_mul_batch(name, s.xy, s.inf, s.sc, subgroup=subgroup), (rows[rev], inf[rev]), s.labels)


@pytest.mark.parametrize("name,subgroup", ENTRIES, ids=IDS)
def test_refused_arguments_leave_the_outputs_untouched(gpu, name, subgroup):
    g = sc.group(name)
    b = sc.seeded_batch(name, 65, SEED + 1)
    fn = getattr(gpu.lib(), "scalar_mul_batch_" + name + ("_subgroup" if subgroup else ""))
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    at_r = co.ints_to_limbs([g.r], g.sw)
    first, last = b.sc.copy(), b.sc.copy()
    first[0], last[-1] = at_r[0], at_r[0]
    all_ones = np.full((1, g.sw), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    refused = [("xy NULL", None, b.sc, b.n, True, True), ("scalars NULL", b.xy, None, b.n, True, True), ("out NULL", b.xy, b.sc, b.n, False, True),
               ("flags NULL", b.xy, b.sc, b.n, True, False), ("two scalars for 65 rows", b.xy, b.sc, 2, True, True), ("no scalar", b.xy, b.sc, 0, True, True),
               ("first scalar = r", b.xy, first, b.n, True, True), ("last scalar = r", b.xy, last, b.n, True, True), ("shared scalar = r", b.xy, at_r, 1, True, True),
               ("shared scalar all ones", b.xy, all_ones, 1, True, True)]
    for label, xy, scal, n_sc, with_out, with_inf in refused:
        out = np.full((b.n, g.aw), SENTINEL, dtype=np.uint64)
        oinf = np.full(b.n, 9, dtype=np.uint8)
        rc = fn(p(xy), p(b.inf), p(scal), C.c_size_t(n_sc), C.c_size_t(b.n), p(out) if with_out else None, p(oinf) if with_inf else None)
        assert rc == 2, label
        assert (out == SENTINEL).all() and (oinf == 9).all(), label
    # n = 0: nothing to do, whatever the pointers
    assert fn(None, None, None, C.c_size_t(0), C.c_size_t(0), None, None) == 0
    # the device form: a scalar >= r among the device's scalars
    bad = b.take(range(b.n))
    bad.sc = last
    rc, out, oinf = _dev_call(gpu, name, subgroup, bad)
    assert rc == 2 and (out == SENTINEL).all() and (oinf == 9).all()
    rc, out, oinf = _dev_call(gpu, name, subgroup, b, n_sc=3)
    assert rc == 2 and (out == SENTINEL).all() and (oinf == 9).all()
    # and the call after a refusal is a normal one
    _same(gpu.scalar_mul_batch(name, b.xy, b.inf, b.sc, subgroup=subgroup), sc.seeded_expected(name, 65, SEED + 1))


def test_group_without_subgroup_path_is_refused_by_the_wrapper(gpu):
    b = sc.seeded_batch("bls12_377_g2", 1, 1)
    with pytest.raises(ValueError):
        gpu.scalar_mul_batch("bls12_377_g2", b.xy, b.inf, b.sc, subgroup=True)


def test_two_threads_calling_concurrently(gpu):
    """two host threads, four calls each, different groups and entries at once: every result is the oracle's"""
    jobs = [[("bls12_377_g1", True), ("bw6_761_g1", False), ("bls12_377_g1", False), ("bls12_377_g2", False)],
            [("bls12_377_g2", False), ("bls12_377_g1", True), ("bw6_761_g2", False), ("bls12_377_g1", False)]]
    for name in sc.GROUPS:
        sc.expected(name)                                           # the references first, outside the threads
    errors = []

    def work(mine):
        try:
            gpu.use_device(0)
            for name, subgroup in mine:
                b, want = _cases(name, subgroup)
                _same(gpu.scalar_mul_batch(name, b.xy, b.inf, b.sc, subgroup=subgroup), want, b.labels)
        except BaseException as e:      # noqa: BLE001  (reported by the main thread)
            errors.append(repr(e))
    threads = [threading.Thread(target=work, args=(j,)) for j in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_timings_of_the_last_call(gpu):
    b, _ = _big("bls12_377_g1")
    gpu.scalar_mul_batch("bls12_377_g1", b.xy, b.inf, b.sc)
    ms = gpu.scalar_mul_last_ms()
    assert ms["table"] > 0 and ms["ladder"] > 0 and ms["normalize"] > 0 and ms["wall"] >= ms["table"] + ms["ladder"] + ms["normalize"]


@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("name,subgroup", ENTRIES, ids=IDS)
def test_host_and_device_forms_agree_with_and_without_flags(gpu, name, subgroup, n):
    """rows without an identity among them: the host form with flags of zero and with none, the device form with flags of zero and with a
    null pointer - four times the same bytes"""
    g = sc.group(name)
    b, want = _big(name)
    keep = [i for i in range(BIG) if not b.inf[i]][:n]
    s, want = b.take(keep), (want[0][keep], want[1][keep])
    assert not s.inf.any()
    _same(gpu.scalar_mul_batch(name, s.xy, s.inf, s.sc, subgroup=subgroup), want)
    _same(gpu.scalar_mul_batch(name, s.xy, None, s.sc, subgroup=subgroup), want)
    rc, out, oinf = _dev_call(gpu, name, subgroup, s)
    assert rc == 0
    _same((out, oinf), want)
    d_xy = torch.from_numpy(s.xy.view(np.int64).copy()).cuda()
    d_sc = torch.from_numpy(s.sc.view(np.int64).copy()).cuda()
    d_out = torch.full((n * g.aw,), SENTINEL, dtype=torch.int64, device="cuda")
    d_oinf = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert gpu.scalar_mul_batch_dev(name, d_xy.data_ptr(), 0, d_sc.data_ptr(), n, n, d_out.data_ptr(), d_oinf.data_ptr(), subgroup=subgroup) == 0
    torch.cuda.synchronize()
    _same((d_out.cpu().numpy().view(np.uint64).reshape(n, g.aw), d_oinf.cpu().numpy()), want)


@pytest.mark.parametrize("name,subgroup", ENTRIES, ids=IDS)
def test_device_range_check_over_two_blocks(gpu, name, subgroup):
    """257 device scalars: the check runs 256 lanes per block, so row 256 sits alone in the second.  All r - 1 passes; r in row 256 and
    all-ones in row 0 are refused with nothing written; the call after a refusal is a normal one."""
    g = sc.group(name)
    b, _ = _big(name)
    top = np.repeat(co.ints_to_limbs([g.r - 1], g.sw), BIG, axis=0)
    rc, out, oinf = _dev_call(gpu, name, subgroup, b, sc_rows=top)
    assert rc == 0
    _same((out, oinf), gpu.scalar_mul_batch(name, b.xy, b.inf, top, subgroup=subgroup))
    last, first = top.copy(), top.copy()
    last[256] = co.ints_to_limbs([g.r], g.sw)[0]
    first[0] = 0xFFFFFFFFFFFFFFFF
    for bad in (last, first):
        rc, out, oinf = _dev_call(gpu, name, subgroup, b, sc_rows=bad)
        assert rc == 2 and (out == SENTINEL).all() and (oinf == 9).all()
    rc, out, oinf = _dev_call(gpu, name, subgroup, b)
    assert rc == 0
    _same((out, oinf), sc.seeded_expected(name, BIG, SEED))
