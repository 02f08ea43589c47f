"""CPU (-m "not gpu"): the host twins of the bulk point validator and of the BW6-761 subgroup test by endomorphism, under bounds tracking
(csrc/host_test.cpp ht_w761_subgroup_both, ht_check_rows; the kernels run the same templates).

- w761_in_subgroup_endo == w761_in_subgroup == the oracle's mul(P, r) on every on-curve case of tests/subgroup_cases.py and on 200 seeded
  random curve points per group.
- check_row's statuses at both levels, with either form of the BW6-761 test, against the case list.
- The new symbols are exported and wrapped, and the refusals work without a device.
- The same templates in a stand-alone program built with -fsanitize=address,undefined."""
import ctypes as C
import os
import shutil
import subprocess
import numpy as np
import pytest
import subgroup_cases as sc
from helpers import build_hosttest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["check_points_bls12_377_g1", "check_points_bls12_377_g2", "check_points_bw6_761_g1", "check_points_bw6_761_g2",
               "check_points_bls12_377_g1_dev", "check_points_bls12_377_g2_dev", "check_points_bw6_761_g1_dev", "check_points_bw6_761_g2_dev",
               "celo_amd_wire761_set_subgroup_test", "celo_amd_check_points_last_ms"]
G761 = ["bw6_761_g1", "bw6_761_g2"]


@pytest.fixture(scope="module")
def ht():
    return C.CDLL(build_hosttest())


def both(ht, name, P):
    row = sc.group(name).pack([P])[0]
    return ht.ht_w761_subgroup_both(C.c_int(1 if name.endswith("g2") else 0), row.ctypes.data_as(C.c_void_p))


def check_rows(ht, cs, level, ladder=0, inf=True):
    st = np.full(cs.n, 0xEE, dtype=np.uint8)
    rc = ht.ht_check_rows(C.c_int(sc.group(cs.name).gid), cs.xy.ctypes.data_as(C.c_void_p), cs.inf.ctypes.data_as(C.c_void_p) if inf else None,
                          C.c_size_t(cs.n), C.c_int(level), C.c_int(ladder), st.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return st


@pytest.mark.parametrize("name", G761)
def test_endo_equals_ladder_equals_oracle_on_the_case_list(ht, name):
    for label, P, member in sc.on_curve_cases(name):
        assert both(ht, name, P) == (3 if member else 0), label


@pytest.mark.parametrize("name", G761)
def test_endo_equals_ladder_equals_oracle_on_random_curve_points(ht, name):
    pts = sc.seeded_curve_points(name, 200, 7611 + name.endswith("g2"))
    verdicts = [member for _, member in pts]
    assert len(pts) >= 199 and any(verdicts) and not all(verdicts)
    for i, (P, member) in enumerate(pts):
        assert both(ht, name, P) == (3 if member else 0), i


@pytest.mark.parametrize("name", sc.GROUPS)
def test_row_checker_statuses(ht, name):
    cs = sc.cases(name)
    for level in (1, 2):
        for ladder in ((0, 1) if name in G761 and level == 2 else (0,)):
            got = check_rows(ht, cs, level, ladder)
            assert np.array_equal(got, cs.want[level]), [(cs.labels[i], int(got[i]), int(cs.want[level][i])) for i in np.nonzero(got != cs.want[level])[0]]
    # without flags a flagged case is judged by its coordinates: the level-1 verdict of the same row with the flag cleared
    unflagged = sc.Cases(name, cs.labels, cs.xy, np.zeros(cs.n, dtype=np.uint8), cs.want[1], cs.want[2])
    got = check_rows(ht, unflagged, 1, inf=False)
    keep = cs.inf == 0
    assert np.array_equal(got[keep], cs.want[1][keep]) and set(got[~keep].tolist()) <= {0, 2}
    assert np.array_equal(got, check_rows(ht, unflagged, 1))
    assert ht.ht_check_rows(C.c_int(4), None, None, C.c_size_t(0), C.c_int(1), C.c_int(0), None) == 2
    assert ht.ht_check_rows(C.c_int(0), None, None, C.c_size_t(0), C.c_int(3), C.c_int(0), None) == 2


def test_new_symbols_exported():
    from celo_bls_snark_rs_amd import ffi
    lib = C.CDLL(ffi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in ffi.EXPORTS and hasattr(lib, name), name
    assert callable(ffi.check_points) and callable(ffi.wire761_set_subgroup_test)


def test_refusals_need_no_device():
    """2 with nothing written, before any device use: a NULL required pointer, a level outside {1, 2}, n > 2^31 - 1; the hook refuses
    anything but 0 and 1.  n = 0 is no refusal, and it is answered before the device is looked for."""
    from celo_bls_snark_rs_amd import ffi
    lib = ffi.lib()
    for name in sc.GROUPS:
        g = sc.group(name)
        xy = np.zeros((2, g.words), dtype=np.uint64)
        st = np.full(2, 0xEE, dtype=np.uint8)
        fb = C.c_uint64(0xEEEE)
        p_xy, p_st = xy.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p)
        for fn, tail in ((getattr(lib, "check_points_" + name), ()), (getattr(lib, "check_points_" + name + "_dev"), (None,))):
            assert fn(None, None, C.c_size_t(2), C.c_int(1), p_st, C.byref(fb), *tail) == 2
            assert fn(p_xy, None, C.c_size_t(2), C.c_int(1), None, C.byref(fb), *tail) == 2
            for level in (0, 3, -1):
                assert fn(p_xy, None, C.c_size_t(2), C.c_int(level), p_st, C.byref(fb), *tail) == 2
            assert fn(p_xy, None, C.c_size_t(1 << 31), C.c_int(2), p_st, C.byref(fb), *tail) == 2
            assert (st == 0xEE).all() and fb.value == 0xEEEE
            assert fn(None, None, C.c_size_t(0), C.c_int(7), None, None, *tail) == 2       # a level that does not exist, even for n = 0
            assert fn(None, None, C.c_size_t(0), C.c_int(2), None, C.byref(fb), *tail) == 0 and fb.value == 0
            fb.value = 0xEEEE
    for bad in (2, -1, 100):
        assert lib.celo_amd_wire761_set_subgroup_test(C.c_int(bad)) == 2
    assert lib.celo_amd_wire761_set_subgroup_test(C.c_int(1)) == 0 and lib.celo_amd_wire761_set_subgroup_test(C.c_int(0)) == 0
    with pytest.raises(ValueError):
        ffi.wire761_set_subgroup_test(2)


def test_templates_under_address_and_ub_sanitizers(tmp_path):
    """tests/subgroup_asan_main.cpp: its own main, built with -fsanitize=address,undefined (the runtimes linked into the program), run as a
    subprocess on the BW6-761 case lists: both forms of the subgroup test and check_row at both levels, every buffer a heap array of its exact
    size.  It prints the statuses; they are the case list's.  No sanitizer enters this process."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler to build tests/subgroup_asan_main.cpp")
    exe = str(tmp_path / "subgroup_asan")
    build = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                            "-I" + os.path.join(ROOT, "celo-bls-snark-rs_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "subgroup_asan_main.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    for name in sc.GROUPS:
        cs = sc.cases(name)
        data = tmp_path / (name + ".bin")
        data.write_bytes(cs.xy.tobytes() + cs.inf.tobytes())
        run = subprocess.run([exe, str(sc.group(name).gid), str(cs.n), str(data)], capture_output=True, text=True)
        assert run.returncode == 0 and "subgroup ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
        lines = run.stdout.splitlines()
        assert lines[0] == " ".join(str(int(v)) for v in cs.want[1]) and lines[1] == " ".join(str(int(v)) for v in cs.want[2]), name
