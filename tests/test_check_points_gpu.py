"""GPU: the bulk point validator check_points_* (csrc/check.h, csrc/unit_check.hip) on the case list of tests/subgroup_cases.py - whose
expected statuses tests/test_subgroup_cases.py proves with the oracle - and the BW6-761 subgroup test by endomorphism against its twin, the
r P ladder, through the validator and through the BW6-761 decoders (celo_amd_wire761_set_subgroup_test 0 / 1)."""
import ctypes as C
import threading
import numpy as np
import pytest
import torch  # before the library: both must share one HIP runtime
from oracle.py import ecc
import subgroup_cases as sc

pytestmark = pytest.mark.gpu
G761 = ["bw6_761_g1", "bw6_761_g2"]


def mismatches(cs, got, level):
    return [(cs.labels[i], int(got[i]), int(cs.want[level][i])) for i in np.nonzero(got != cs.want[level])[0]]


def check(gpu, cs, level, inf=True):
    st, first = gpu.check_points(cs.name, cs.xy, cs.inf if inf else None, level)
    return st, first


def rotated(cs, n, start=3, step=7):
    """n rows that walk the case list (step and len(list) need not be coprime: every class still occurs for n >= len)"""
    return cs.take([(start + step * i) % cs.n for i in range(n)])


@pytest.fixture
def hook(gpu):
    """the subgroup-test switch, put back to its default when the test ends"""
    try:
        yield gpu.wire761_set_subgroup_test
    finally:
        gpu.wire761_set_subgroup_test(0)


@pytest.mark.parametrize("name", sc.GROUPS)
def test_case_list_at_both_levels(gpu, name):
    cs = sc.cases(name)
    got = {}
    for level in (1, 2):
        got[level], first = check(gpu, cs, level)
        assert np.array_equal(got[level], cs.want[level]), mismatches(cs, got[level], level)
        assert first == cs.first_bad(level)
    # level 1 against level 2: they differ exactly on the curve points outside the subgroup
    differ = got[1] != got[2]
    assert differ.any() and (got[2][differ] == 3).all() and (got[1][differ] == 0).all() and not (got[2][~differ] == 3).any()


@pytest.mark.parametrize("name", sc.GROUPS)
def test_batch_sizes(gpu, name):
    cs = sc.cases(name)
    for n in (1, 63, 64, 65, 257):
        b = rotated(cs, n, start=n)
        for level in (1, 2):
            st, first = check(gpu, b, level)
            assert np.array_equal(st, b.want[level]), (n, level, mismatches(b, st, level))
            assert first == b.first_bad(level), (n, level)
    # no rejected row: first_bad is n
    good = cs.take([0, 1] * 33)
    st, first = check(gpu, good, 2)
    assert not st.any() and first == 66


@pytest.mark.parametrize("name", sc.GROUPS)
def test_every_class_at_the_wave_borders(gpu, name):
    """a 65-row batch of mixed statuses with case c at rows 0, 63 (the last lane of the first wave) and 64 (the first of the second), for every c"""
    cs = sc.cases(name)
    for c in range(cs.n):
        idx = [(c + 1 + 5 * i) % cs.n for i in range(65)]
        for pos in (0, 63, 64):
            idx[pos] = c
        b = cs.take(idx)
        st, first = check(gpu, b, 2)
        assert np.array_equal(st, b.want[2]), (cs.labels[c], mismatches(b, st, 2))
        assert first == b.first_bad(2)
        assert len(set(b.want[2][:64].tolist())) >= 3                     # the statuses are mixed inside the first wave


@pytest.mark.parametrize("name", sc.GROUPS)
def test_null_flags_are_all_zero_flags(gpu, name):
    cs = sc.cases(name)
    b = cs.take(np.nonzero(cs.inf == 0)[0])
    for level in (1, 2):
        with_zero, f0 = check(gpu, b, level)
        without, f1 = check(gpu, b, level, inf=False)
        assert np.array_equal(with_zero, without) and np.array_equal(without, b.want[level]) and f0 == f1


@pytest.mark.parametrize("name", sc.GROUPS)
def test_device_form_on_a_callers_stream(gpu, name):
    cs = sc.cases(name)
    b = rotated(cs, 130)
    want, want_first = check(gpu, b, 2)
    stream = torch.cuda.Stream()
    d_xy = torch.from_numpy(b.xy.view(np.int64).copy()).cuda()
    d_inf = torch.from_numpy(b.inf.copy()).cuda()
    d_st = torch.full((b.n,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    first = gpu.check_points_dev(name, d_xy.data_ptr(), d_inf.data_ptr(), b.n, d_st.data_ptr(), 2, stream.cuda_stream)
    assert first == want_first and np.array_equal(d_st.cpu().numpy(), want) and np.array_equal(want, b.want[2])
    assert np.array_equal(d_xy.cpu().numpy().view(np.uint64), b.xy)       # the caller's rows are only read
    # no flags on the device either, on the null stream
    d_st.fill_(0xEE)
    torch.cuda.synchronize()
    nf = sc.Cases(name, b.labels, b.xy, np.zeros(b.n, dtype=np.uint8), b.want[1], b.want[2])
    first = gpu.check_points_dev(name, d_xy.data_ptr(), 0, b.n, d_st.data_ptr(), 1, 0)
    st_host, first_host = check(gpu, nf, 1, inf=False)
    assert first == first_host and np.array_equal(d_st.cpu().numpy(), st_host)


@pytest.mark.parametrize("name", sc.GROUPS)
def test_one_changed_row_changes_one_status(gpu, name):
    cs = sc.cases(name)
    good = [i for i in range(cs.n) if cs.want[2][i] == 0]
    outside = [i for i in range(cs.n) if cs.want[2][i] == 3]
    idx = [good[i % len(good)] for i in range(65)]
    base, first = check(gpu, cs.take(idx), 2)
    assert not base.any() and first == 65
    idx[37] = outside[0]
    st, first = check(gpu, cs.take(idx), 2)
    assert first == 37 and st[37] == 3 and np.array_equal(np.delete(st, 37), np.delete(base, 37))


def test_refusals(gpu):
    lib = gpu.lib()
    for name in sc.GROUPS:
        cs = sc.cases(name)
        st = np.full(cs.n, 0xEE, dtype=np.uint8)
        fb = C.c_uint64(0xEEEE)
        fn = getattr(lib, "check_points_" + name)
        p_xy, p_inf, p_st = cs.xy.ctypes.data_as(C.c_void_p), cs.inf.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p)
        assert fn(None, p_inf, C.c_size_t(cs.n), C.c_int(2), p_st, C.byref(fb)) == 2
        assert fn(p_xy, p_inf, C.c_size_t(cs.n), C.c_int(2), None, C.byref(fb)) == 2
        assert fn(p_xy, p_inf, C.c_size_t(cs.n), C.c_int(0), p_st, C.byref(fb)) == 2
        assert fn(p_xy, p_inf, C.c_size_t(cs.n), C.c_int(3), p_st, C.byref(fb)) == 2
        assert fn(p_xy, p_inf, C.c_size_t(1 << 31), C.c_int(2), p_st, C.byref(fb)) == 2
        assert (st == 0xEE).all() and fb.value == 0xEEEE
        assert fn(None, None, C.c_size_t(0), C.c_int(1), None, C.byref(fb)) == 0 and fb.value == 0
        assert fn(p_xy, p_inf, C.c_size_t(cs.n), C.c_int(2), p_st, None) == 0 and np.array_equal(st, cs.want[2])   # first_bad may be NULL


def test_two_threads(gpu):
    out, errs = {}, []

    def work(name):
        try:
            gpu.use_device(0)
            cs = sc.cases(name)
            for _ in range(4):
                st, first = check(gpu, cs, 2)
                assert np.array_equal(st, cs.want[2]) and first == cs.first_bad(2)
            out[name] = True
        except BaseException as e:  # noqa: BLE001  (reported by the main thread)
            errs.append((name, repr(e)))
    ts = [threading.Thread(target=work, args=(n,)) for n in ("bw6_761_g2", "bls12_377_g1")]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs and len(out) == 2, errs


@pytest.mark.parametrize("name", G761)
def test_validator_is_the_same_under_either_subgroup_test(gpu, hook, name):
    cs = sc.cases(name)
    b = rotated(cs, 130)
    got = {}
    for form in (0, 1):
        hook(form)
        got[form] = check(gpu, b, 2)
    assert np.array_equal(got[0][0], got[1][0]) and got[0][1] == got[1][1] and np.array_equal(got[0][0], b.want[2])
    # the ladder's kernel zeroes the rows it rejects: it must have been given a copy, with device pointers too
    hook(1)
    d_xy = torch.from_numpy(b.xy.view(np.int64).copy()).cuda()
    d_st = torch.full((b.n,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    first = gpu.check_points_dev(name, d_xy.data_ptr(), 0, b.n, d_st.data_ptr(), 2, 0)
    unflagged = sc.Cases(name, b.labels, b.xy, np.zeros(b.n, dtype=np.uint8), b.want[1], b.want[2])
    hook(0)
    want, want_first = check(gpu, unflagged, 2, inf=False)
    assert first == want_first and np.array_equal(d_st.cpu().numpy(), want) and np.array_equal(d_xy.cpu().numpy().view(np.uint64), b.xy)


@pytest.mark.parametrize("name", G761)
def test_decoders_are_the_same_under_either_subgroup_test(gpu, hook, name):
    """decompress_bw6_761_* and decode_uncompressed_bw6_761_* (checked) on the serialized case list: G +- (0, 2), the order-13 sum and the
    points of order 2 among them.  Statuses and rows are identical with the hook at 0 and at 1, and they are the oracle's."""
    g = sc.group(name)
    on = sc.on_curve_cases(name)
    labels = [label for label, _, _ in on]
    if name == "bw6_761_g2":
        assert {"G + (0, 2)", "G - (0, 2)", "G + order 13"} <= set(labels)
    pts = [P for _, P, _ in on] * 3                                        # past one wave
    members = [m for _, _, m in on] * 3
    want_st = np.array([0 if m else 3 for m in members], dtype=np.uint8)
    want_xy = g.pack(pts)
    want_xy[want_st != 0] = 0
    for compressed in (True, False):
        data = b"".join(ecc.ser_point(g.E, P, compressed=compressed) for P in pts)
        got = {}
        for form in (0, 1):
            hook(form)
            got[form] = gpu.decompress(name, data, check_subgroup=True) if compressed else gpu.decode_uncompressed(name, data, check=True)
        assert np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[0][0], got[1][0]), compressed
        bad = np.nonzero(got[0][1] != want_st)[0]
        assert bad.size == 0, [(labels[i % len(on)], int(got[0][1][i])) for i in bad]
        assert np.array_equal(got[0][0], want_xy)


def test_the_hook_refuses_what_it_does_not_know(gpu, hook):
    lib = gpu.lib()
    hook(1)
    for bad in (2, -1, 7):
        assert lib.celo_amd_wire761_set_subgroup_test(C.c_int(bad)) == 2
        with pytest.raises(ValueError):
            hook(bad)
    # a refused value leaves the setting alone: still the ladder, still the same verdicts
    cs = sc.cases("bw6_761_g2")
    st, _ = check(gpu, cs, 2)
    assert np.array_equal(st, cs.want[2])
