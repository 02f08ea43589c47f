"""CPU (-m "not gpu"): wide BLS12-377 verifying keys and the many-lane input sum without a device - the host twins of
k_g16_inputs_lanes<G16Bls> (ht_g16_input_lanes_377: phase 1 and the fold for a given L, bounds tracked) against the oracle's MSM on whole
rows, the fold's doubling / cancelling / identity branches from the key's known scalars, the window, parse and lane rules against their
restatements (tests/groth16_wide_cases.py), the argument refusals of the five new symbols, and a sanitizer run of the host templates in a
program of its own."""
import ctypes as C
import os
import re
import shutil
import subprocess
import numpy as np
import pytest
from oracle.py import ecc
from oracle import cpu_oracle as co
from tests import groth16_verify377_cases as gc
from tests import groth16_wide_cases as wc
from tests import helpers as H

R = gc.R
TWIN_C = 4                       # window bits of the twin's tables: the fewest entries per base (64 windows of 8)


@pytest.fixture(scope="module")
def ht():
    return C.CDLL(H.build_hosttest())


@pytest.fixture(scope="module")
def key257():
    """one key for every input count up to 257 = 256 + 1: a key of fewer inputs is a prefix of it (wc.sub_key), so the twin builds its tables once"""
    return gc.Key(257, 0x61DE)


def lane_rows(ht, key, xs, L):
    n_in, n = key.n_in, len(xs)
    inputs = co.ints_to_limbs([v for x in xs for v in x], 4).reshape(n, n_in, 4) if n_in else np.zeros((n, 0, 4), dtype=np.uint64)
    out = np.zeros((n, 12), dtype=np.uint64)
    inf = np.zeros(n, dtype=np.uint8)
    st = np.zeros(n, dtype=np.uint8)
    abc = np.ascontiguousarray(key.abc)
    rc = ht.ht_g16_input_lanes_377(co._p(abc), C.c_size_t(n_in + 1), co._p(inputs), C.c_size_t(n), C.c_int(TWIN_C), C.c_int(L), co._p(out), co._p(inf), co._p(st))
    assert rc == 0
    return out, inf, st


def limbs(xs, n_in):
    return co.ints_to_limbs([v for x in xs for v in x], 4).reshape(len(xs), n_in, 4) if n_in else np.zeros((len(xs), 0, 4), dtype=np.uint64)


@pytest.mark.parametrize("L", wc.LANES)
def test_lane_sums_equal_the_oracles_msm(ht, key257, L):
    """whole rows at every input count around the lane count: the edge inputs, random ones, and r, r + 1, 2^256 - 1 at the first input, the
    last and one of another lane - the status set, and the input entered as zero"""
    ht.ht_g16_input_lanes_377(co._p(np.ascontiguousarray(key257.abc)), C.c_size_t(258), co._p(np.zeros((1, 257, 4), dtype=np.uint64)), C.c_size_t(1), C.c_int(TWIN_C),
                              C.c_int(1), co._p(np.zeros(12, dtype=np.uint64)), co._p(np.zeros(1, dtype=np.uint8)), co._p(np.zeros(1, dtype=np.uint8)))
    for n_in in sorted({0, 1, 2, max(L - 1, 0), L, L + 1, 65, 130}):
        key = wc.sub_key(key257, n_in)
        rng = ecc.SplitMix64(1000 * L + n_in)
        xs = [[v] * n_in for v in gc.EDGE_INPUTS] + [[ecc.random_scalar(rng, R) for _ in range(n_in)] for _ in range(2)]
        bad = wc.bad_input_rows(n_in, L, rng) if n_in else []
        n_good = len(xs)
        xs += [x for x, _ in bad]
        out, inf, st = lane_rows(ht, key, xs, L)
        assert st.tolist() == [0] * n_good + [1] * len(bad), (L, n_in)
        zeroed = xs[:n_good] + [[0 if k == j else v for k, v in enumerate(x)] for x, j in bad]
        want, winf = gc.acc_rows(key, limbs(zeroed, n_in))
        assert np.array_equal(out, want) and np.array_equal(inf, winf), (L, n_in)


@pytest.mark.parametrize("L", wc.LANES[1:])
def test_fold_branches(ht, key257, L):
    """equal partials (doubling), opposite ones (cancelling) and identities in the first round, the last round and at lane 0, built from the
    key's scalars: the row is the oracle's - the identity where the whole sum cancels"""
    key = wc.sub_key(key257, max(L, 3) + 1)
    cases = wc.fold_branch_inputs(key, L)
    assert {"double_lane0", "cancel_lane0", "only_lane0", "only_last_lane"} <= set(cases) and (L < 4 or "double_first_round" in cases and "cancel_last_round" in cases)
    names = sorted(cases)
    xs = [cases[k] for k in names]
    out, inf, st = lane_rows(ht, key, xs, L)
    want, winf = gc.acc_rows(key, limbs(xs, key.n_in))
    assert not st.any()
    assert np.array_equal(out, want) and np.array_equal(inf, winf), (L, [k for i, k in enumerate(names) if not np.array_equal(out[i], want[i])])
    # the cases are what they claim: the cancelling ones at lane 0 and in the last round sum to the identity, the doubling ones to twice a partial
    assert inf[names.index("cancel_lane0")] == 1 and key.acc_scalar(cases["cancel_lane0"]) == 0
    assert key.acc_scalar(cases["double_lane0"]) == 2 * key.u[0] % R
    if L >= 4:
        assert inf[names.index("cancel_last_round")] == 1
        assert key.acc_scalar(cases["double_first_round"]) == (key.u[0] + 2 * key.u[2]) % R and key.acc_scalar(cases["cancel_first_round"]) == key.u[0]


def test_twin_refuses_a_width_that_is_no_power_of_two(ht, key257):
    key = wc.sub_key(key257, 2)
    z = np.zeros((1, 2, 4), dtype=np.uint64)
    o, i, s = np.zeros(12, dtype=np.uint64), np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
    for L in (0, 3, 257, 512, -2):
        assert ht.ht_g16_input_lanes_377(co._p(np.ascontiguousarray(key.abc)), C.c_size_t(3), co._p(z), C.c_size_t(1), C.c_int(TWIN_C), C.c_int(L), co._p(o), co._p(i), co._p(s)) == 2


def test_window_rule_at_every_border(ht):
    """ht_g16_window_bits_wide_377 against the restatement at every border +- 1: the last input count of 10 .. 4 bits is
    39 | 70 | 128 | 221 | 381 | 642 | 1024, and 1024 inputs at 4 bits fill the budget exactly"""
    ht.ht_g16_window_bits_wide_377.restype = C.c_int
    for c, last in wc.BORDERS.items():
        for n in (last - 1, last, last + 1):
            got = ht.ht_g16_window_bits_wide_377(C.c_size_t(n))
            want = wc.window_bits_wide(n)
            assert got == (-1 if want is None else want), n
        assert wc.window_bits_wide(last) == c and wc.window_bits_wide(last + 1) == (c - 1 if c > 4 else None)
        assert last * gc.fb_windows(253, c) * (1 << (c - 1)) * gc.ENTRY_BYTES <= gc.TABLE_BUDGET
        assert (last + 1) * gc.fb_windows(253, c) * (1 << (c - 1)) * gc.ENTRY_BYTES > gc.TABLE_BUDGET
    assert 1024 * gc.fb_windows(253, 4) * 8 * gc.ENTRY_BYTES == gc.TABLE_BUDGET
    assert wc.window_bits_wide(509) == 5 and wc.window_bits_wide(1022) == 4
    assert ht.ht_g16_window_bits_377(C.c_size_t(64)) == 9                # the narrow rule as it was


def test_lane_rule(ht):
    """ht_g16_pick_lanes against its restatement over a grid; one proof of 509 inputs gets the widest width the work term admits, 2^16 proofs
    get one lane, and a key of at most 64 inputs gets one lane whatever the batch"""
    ht.ht_g16_pick_lanes.restype = C.c_uint32
    got = lambda n, m: ht.ht_g16_pick_lanes(C.c_size_t(n), C.c_size_t(m))
    for n in (0, 1, 2, 39, 64, 65, 66, 70, 128, 129, 255, 256, 257, 381, 509, 512, 513, 642, 1022, 1024):
        for m in (1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 1024, 4096, (1 << 15) - 1, 1 << 15, (1 << 15) + 1, 1 << 16, (1 << 16) + 1, 1 << 20, 1 << 24):
            L = got(n, m)
            assert L == wc.pick_lanes(n, m), (n, m)
            assert L in wc.LANES
    work509 = 1
    while work509 * wc.INPUTS_PER_LANE < 509:
        work509 *= 2
    assert got(509, 1) == min(256, work509) and got(509, 1) > 1
    assert got(509, 1 << 16) == 1 and got(1024, 1 << 16) == 1
    assert all(got(n, m) == 1 for n in (0, 1, 64) for m in (1, 64, 1 << 16))


# ---- the wide parse
def parse_wide(ht, data, cap=1030):
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    rows = np.zeros((cap, 24), dtype=np.uint64)
    inf = np.zeros(cap, dtype=np.uint8)
    n, bad = C.c_uint64(0), C.c_uint64(1 << 40)
    rc = ht.ht_g16_vk_parse_wide_377(co._p(buf), C.c_size_t(buf.size), C.c_size_t(cap), co._p(rows), co._p(inf), C.byref(n), C.byref(bad))
    return rc, rows[:4 + n.value], inf[:4 + n.value], bad.value


def test_wide_parse(ht, key257):
    """1024 inputs are accepted and 1025 refused with 36 (the rows repeat: the parse does not mind); 30, 31 and 33 as the narrow parse gives
    them; the narrow parse still refuses 65"""
    reps = np.concatenate([key257.abc] * 4)                              # 1032 rows of valid points
    rc, rows, inf, _ = parse_wide(ht, key257.serialize(reps[:1025]))
    assert rc == 0 and not inf.any() and rows.shape[0] == 4 + 1025
    assert np.array_equal(rows[4:, :12], reps[:1025]) and np.array_equal(rows[0, :12], key257.alpha) and np.array_equal(rows[3], key257.delta)
    assert parse_wide(ht, key257.serialize(reps[:1026]))[0] == 36
    key = wc.sub_key(key257, 65)
    data = key.serialize()
    assert parse_wide(ht, data)[0] == 0
    assert parse_wide(ht, data[:-1])[0] == 30 and parse_wide(ht, data + b"\0")[0] == 31
    off = bytearray(data)
    at = 48 + 3 * 96 + 8 + 65 * 48                                       # gamma_abc[65], the last row
    off[at:at + 48] = ecc.ser_point(ecc.E1_377, gc.off_subgroup_point(False, 5))
    rc, _, _, bad = parse_wide(ht, off)
    assert rc == 33 and bad == 4 + 65
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    n, bad = C.c_uint64(0), C.c_uint64(0)
    rows, inf = np.zeros((80, 24), dtype=np.uint64), np.zeros(80, dtype=np.uint8)
    assert ht.ht_g16_vk_parse_377(co._p(buf), C.c_size_t(buf.size), C.c_size_t(80), co._p(rows), co._p(inf), C.byref(n), C.byref(bad)) == 36


def test_argument_refusals_need_no_device():
    """the five new symbols are declared, exported and wrapped, and refuse their arguments before any device use"""
    from celo_bls_snark_rs_amd import ffi
    lib = ffi.lib()
    p = co._p
    z = np.zeros(24, dtype=np.uint64)
    abc = np.zeros((1027, 12), dtype=np.uint64)
    h = C.c_void_p()
    header = open(os.path.join(gc.ROOT, "include", "celo_bls_amd.h")).read()
    for name in ("groth16_vk_load_bls12_377_wide", "groth16_vk_load_bls12_377_wide_serialized", "celo_amd_groth16_set_input_lanes", "celo_amd_groth16_inputs_last",
                 "groth16_hash_helper_verify_bls12_377"):
        assert name in ffi.EXPORTS and hasattr(lib, name) and re.search(r"\b%s\(" % name, header), name
    assert ffi.VK_WIDE_INPUTS == wc.WIDE_MAX == 1024 and ffi.G16_INPUT_LANES == wc.LANES
    wide = lib.groth16_vk_load_bls12_377_wide
    assert wide(None, p(z), p(z), p(z), p(abc), C.c_size_t(1), C.byref(h)) == 2
    assert wide(p(z), p(z), p(z), p(z), None, C.c_size_t(1), C.byref(h)) == 2
    assert wide(p(z), p(z), p(z), p(z), p(abc), C.c_size_t(1), None) == 2
    assert wide(p(z), p(z), p(z), p(z), p(abc), C.c_size_t(0), C.byref(h)) == 2
    assert wide(p(z), p(z), p(z), p(z), p(abc), C.c_size_t(1026), C.byref(h)) == ffi.VK_ERR_INPUTS == 36
    assert lib.groth16_vk_load_bls12_377(p(z), p(z), p(z), p(z), p(abc), C.c_size_t(66), C.byref(h)) == 36          # the narrow loader as it was
    ser = lib.groth16_vk_load_bls12_377_wide_serialized
    assert ser(None, C.c_size_t(500), C.byref(h)) == 2 and ser(p(np.zeros(400, dtype=np.uint8)), C.c_size_t(400), None) == 2
    assert ser(p(np.zeros(343, dtype=np.uint8)), C.c_size_t(343), C.byref(h)) == 30
    hdr = np.zeros(344 + 48, dtype=np.uint8)
    hdr[336], hdr[337] = 1026 & 255, 1026 >> 8
    assert ser(p(hdr), C.c_size_t(hdr.size), C.byref(h)) == 36
    hdr[336], hdr[337] = 66, 0
    assert ser(p(hdr), C.c_size_t(hdr.size), C.byref(h)) == 30          # 66 rows are admitted by the wide loader: the bytes end early
    assert lib.groth16_vk_load_bls12_377_serialized(p(hdr), C.c_size_t(hdr.size), C.byref(h)) == 36
    assert not h.value
    # the setter and the reader
    setter = lib.celo_amd_groth16_set_input_lanes
    for L in (0,) + ffi.G16_INPUT_LANES:
        assert setter(C.c_int(L)) == 0, L
    for L in (3, 512, -1, 5, 255, 257, 1 << 20):
        assert setter(C.c_int(L)) == 2, L
        with pytest.raises(ValueError):
            ffi.groth16_set_input_lanes(L)
    ffi.groth16_set_input_lanes(0)
    lanes, n_in = C.c_int(-1), C.c_int(-1)
    assert lib.celo_amd_groth16_inputs_last(None, C.byref(n_in)) == 2 and lib.celo_amd_groth16_inputs_last(C.byref(lanes), None) == 2
    assert lib.celo_amd_groth16_inputs_last(C.byref(lanes), C.byref(n_in)) == 0 and ffi.groth16_inputs_last() == (lanes.value, n_in.value)
    # the helper verifier
    hv = lib.groth16_hash_helper_verify_bls12_377
    rows, proofs, out = np.zeros((18, 48), dtype=np.uint8), np.zeros(192, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
    fake = C.c_void_p(0x1000)
    args = lambda vk=fake, r=rows, n=1, e=18, order=0, pr=proofs, mode=0, o=out: (vk, p(r), C.c_size_t(n), C.c_size_t(e), C.c_int(order), p(pr), C.c_int(mode), None, p(o))
    assert hv(*args(vk=None)) == 2 and hv(*args(r=None)) == 2 and hv(*args(pr=None)) == 2 and hv(*args(o=None)) == 2
    assert hv(*args(n=0)) == 2 and hv(*args(e=0)) == 2 and hv(*args(n=(1 << 24) + 1)) == 2 and hv(*args(n=1 << 20, e=18)) == 2
    assert hv(*args(order=2)) == 2 and hv(*args(mode=2)) == 2
    assert hv(*args()) == 2                                              # a handle that is not alive: refused, not followed
    assert callable(ffi.hash_helper_verify) and callable(ffi.groth16_inputs_last)


def test_resources_of_the_lanes_kernel():
    """from the build's own resource remarks: k_g16_inputs_lanes<G16Bls> runs without scratch at two waves per SIMD, and asks for no static LDS
    (its fold buffer is dynamic: at most 128 slots of 272 bytes)"""
    txt = open(os.path.join(gc.ROOT, "celo-bls-snark-rs_amd", "build", "unit_groth16_verify377.remarks.txt")).read()
    m = re.search(r"Function Name: \S*k_g16_inputs_lanes\S*G16Bls\S*.*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)", txt, re.S)
    assert m and [int(v) for v in m.groups()] == [0, 2, 0], m and m.groups()
    assert 128 * 272 < 64 << 10


def test_address_and_ub_check_of_the_lane_sum_in_a_program_of_its_own(tmp_path, key257):
    """tests/g16_lanes_asan_main.cpp: its own main, built with -fsanitize=address,undefined (the runtimes linked into the program), run as a
    subprocess - the lane sum and the fold at L = 256 with 130 inputs.  Its row is the oracle's.  No sanitizer enters this process."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler to build tests/g16_lanes_asan_main.cpp")
    key = wc.sub_key(key257, 130)
    rng = ecc.SplitMix64(77)
    x = [ecc.random_scalar(rng, R) for _ in range(130)]
    x[0], x[129], x[64] = R - 1, gc.ALL_ONES, 0
    data = tmp_path / "key_and_inputs.bin"
    data.write_bytes(np.ascontiguousarray(key.abc, dtype=np.uint64).tobytes() + limbs([x], 130).tobytes())
    exe = str(tmp_path / "g16_lanes_asan")
    build = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                            "-I" + os.path.join(gc.ROOT, "celo-bls-snark-rs_amd", "csrc"), "-o", exe, os.path.join(gc.ROOT, "tests", "g16_lanes_asan_main.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe, str(data)], capture_output=True, text=True)
    assert run.returncode == 0 and "g16 lanes ok" in run.stdout and "bad=0" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    want, winf = gc.acc_rows(key, limbs([x], 130))
    assert winf[0] == 0 and run.stdout.splitlines()[0] == " ".join("%016x" % int(v) for v in want[0])
