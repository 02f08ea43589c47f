"""CPU (-m "not gpu"): the HashToBits circuit through its host-only entries (hash_to_bits_r1cs_size_bls12_377, hash_to_bits_r1cs_bls12_377)
and the host twin of the assignment (celo_amd_hash_to_bits_assignment_host), against the Python restatement in tests/hashbits_ref.py.
Everything is integer arithmetic and every comparison is exact.  The matrices and assignments are made once per m and shared, unchanged."""
import ctypes as C
import functools
import os
import random
import shutil
import subprocess
import numpy as np
import pytest
import hashbits_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS = [1, 2, 3, 21]


def ffi():
    from celo_bls_snark_rs_amd import ffi as f
    return f


def rows_for(m, kind, seed=7):
    if kind == "zero":
        return np.zeros((m, 48), dtype=np.uint8)
    if kind == "ones":
        return np.full((m, 48), 0xFF, dtype=np.uint8)
    rng = random.Random(1000 * m + seed)
    return np.frombuffer(bytes(rng.randrange(256) for _ in range(48 * m)), dtype=np.uint8).reshape(m, 48).copy()


@functools.lru_cache(maxsize=None)
def circuit(m):
    sizes, mats = ffi().hash_to_bits_r1cs(m)
    return sizes, mats, hr.System(sizes["n_vars"], mats)


def host_z(rows, bit_order=0):
    return hr.from_mont(ffi().hash_to_bits_assignment(rows, bit_order, host=True))


@pytest.mark.parametrize("m", MS)
def test_size_query_agrees_with_the_arrays_and_the_load_rules(m):
    sizes, mats, _ = circuit(m)
    assert sizes["n_inputs"] == hr.n_inputs(m)
    assert (1 << sizes["log_n"]) >= sizes["n_constraints"] + sizes["n_inputs"] > (1 << (sizes["log_n"] - 1))
    assert sizes["n_vars"] == sizes["n_inputs"] + m * sizes["stride"]
    for k, (rp, col, val) in zip("abc", mats):
        # groth16_r1cs_load's host validation: row_ptr monotone from 0 to nnz, col < n_vars, val < r
        assert rp[0] == 0 and rp[-1] == sizes["nnz_" + k] == col.shape[0] and np.all(np.diff(rp.astype(np.int64)) >= 0)
        assert col.size == 0 or int(col.max()) < sizes["n_vars"]
        assert all(v < hr.R377 for v in hr.limbs_to_ints(hr.unique_rows(val)[0]))


def test_sizes_are_affine_in_m_apart_from_the_pack_rows():
    s = {m: circuit(m)[0] for m in MS}
    per = s[2]["n_constraints"] - (s[2]["n_inputs"] - 1) - (s[1]["n_constraints"] - (s[1]["n_inputs"] - 1))
    for m in MS:
        assert s[m]["n_constraints"] == m * per + s[m]["n_inputs"] - 1
        assert s[m]["n_vars"] == m * s[1]["stride"] + s[m]["n_inputs"] and s[m]["stride"] == s[1]["stride"]
    # the matrices of epoch e are those of epoch 0 with the columns moved by e * stride: nnz without the pack rows is m times that of one epoch
    for k, idx in (("nnz_a", 0), ("nnz_b", 1), ("nnz_c", 2)):
        body = {m: int(circuit(m)[1][idx][0][m * per]) for m in MS}
        assert all(body[m] == m * body[1] for m in MS), k
    assert all(s[m]["nnz_b"] == m * int(circuit(1)[1][1][0][per]) + s[m]["n_inputs"] - 1 for m in MS)
    assert all(s[m]["nnz_c"] == m * s[1]["nnz_c"] for m in MS)


def test_n_inputs_follows_the_formula_at_the_chunk_borders():
    f = ffi()
    assert (384 * 21) % 252 == 0 and (512 * 63) % 252 == 0          # the message chunks / the XOF chunks end exactly on a border
    for m in (1, 2, 3, 17, 18, 20, 21, 22, 62, 63, 64, 143):
        rc, s = f.hash_to_bits_size(m)
        assert rc == 0 and s["n_inputs"] == hr.n_inputs(m) == 1 + -(-384 * m // 252) + -(-512 * m // 252), m
    assert hr.n_inputs(17) - 1 == 61 and hr.n_inputs(18) - 1 == 65    # the batch verifier's limit of 64 inputs falls between
    assert f.hash_to_bits_size(143)[1]["log_n"] == 23


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("kind", ["random", "zero", "ones"])
def test_host_twin_satisfies_every_row_and_states_the_instance(m, kind):
    sizes, _, system = circuit(m)
    rows = rows_for(m, kind)
    for order in (0, 1):
        z = host_z(rows, order)
        assert len(z) == sizes["n_vars"] and z[0] == 1
        assert z[:sizes["n_inputs"]] == hr.instance(rows, order)
        assert set(z[sizes["n_inputs"]:]) <= {0, 1}
        assert system.unsatisfied(z).size == 0


def test_bit_order_one_is_order_zero_on_the_reversed_row():
    rows = rows_for(3, "random", 11)
    # the 384-bit reversal of a row read as one little-endian integer
    rev = np.array([list(int(format(int.from_bytes(bytes(r), "little"), "0384b")[::-1], 2).to_bytes(48, "little")) for r in rows], dtype=np.uint8)
    assert np.array_equal(ffi().hash_to_bits_assignment(rows, 1, host=True), ffi().hash_to_bits_assignment(rev, 0, host=True))
    assert hr.message_bits(rows[0], 1) == hr.message_bits(rows[0], 0)[::-1] == hr.message_bits(rev[0], 0)


@pytest.mark.wall_clock(600)
def test_every_single_variable_perturbation_breaks_a_row():
    sizes, _, system = circuit(1)
    z = host_z(rows_for(1, "random", 3))
    witness = range(sizes["n_inputs"], sizes["n_vars"])
    # every witness variable: 0 <-> 1, and to 2
    assert system.perturbation_misses(z, witness, [lambda v: 1 - v, lambda v: 2]) == []
    # every instance variable (the constant one included): + 1, and to 0
    assert system.perturbation_misses(z, range(sizes["n_inputs"]), [lambda v: v + 1, lambda v: 0]) == []


def test_swapped_statements_are_unsatisfied():
    sizes, _, system = circuit(2)
    n_in, mc = sizes["n_inputs"], -(-384 * 2 // 252)
    z, other = host_z(rows_for(2, "random", 1)), host_z(rows_for(2, "random", 2))
    assert system.unsatisfied(z).size == 0
    with_xof = z[:1 + mc] + other[1 + mc:n_in] + z[n_in:]           # the witness of M with the XOF inputs of M'
    with_msg = z[:1] + other[1:1 + mc] + z[1 + mc:]                 # ... with the message inputs of M'
    assert system.unsatisfied(with_xof).size > 0 and system.unsatisfied(with_msg).size > 0


def test_refusals_need_no_device():
    f = ffi()
    lib = f.lib()
    out = np.zeros(8, dtype=np.uint64)
    rows = rows_for(1, "random")
    z = np.zeros((circuit(1)[0]["n_vars"], 4), dtype=np.uint64)
    assert lib.hash_to_bits_r1cs_size_bls12_377(C.c_size_t(0), f._p(out)) == 2
    assert lib.hash_to_bits_r1cs_size_bls12_377(C.c_size_t(1), None) == 2
    assert lib.hash_to_bits_r1cs_size_bls12_377(C.c_size_t(1 << 20), f._p(out)) == 2          # log_n > 28
    assert lib.hash_to_bits_r1cs_size_bls12_377(C.c_size_t(1 << 40), f._p(out)) == 2
    assert lib.hash_to_bits_r1cs_bls12_377(C.c_size_t(1), *([None] * 9)) == 2
    assert lib.hash_to_bits_r1cs_bls12_377(C.c_size_t(0), *([None] * 9)) == 2
    for fn in (lib.celo_amd_hash_to_bits_assignment_host, lib.hash_to_bits_assignment_bls12_377):
        assert fn(f._p(rows), C.c_size_t(0), C.c_int(0), f._p(z)) == 2
        assert fn(None, C.c_size_t(1), C.c_int(0), f._p(z)) == 2
        assert fn(f._p(rows), C.c_size_t(1), C.c_int(0), None) == 2
        assert fn(f._p(rows), C.c_size_t(1), C.c_int(2), f._p(z)) == 2
        assert fn(f._p(rows), C.c_size_t(1 << 20), C.c_int(0), f._p(z)) == 2
    assert lib.hash_to_bits_public_inputs_bls12_377(f._p(rows), C.c_size_t(1), C.c_size_t(1), C.c_int(2), f._p(z)) == 2
    assert lib.hash_to_bits_public_inputs_bls12_377(f._p(rows), C.c_size_t(0), C.c_size_t(1), C.c_int(0), f._p(z)) == 2
    assert lib.hash_to_bits_public_inputs_bls12_377(None, C.c_size_t(1), C.c_size_t(1), C.c_int(0), f._p(z)) == 2
    h = C.c_void_p()
    assert lib.hash_to_bits_r1cs_load_bls12_377(C.c_size_t(0), C.byref(h)) == 2 and not h
    assert lib.hash_to_bits_r1cs_load_bls12_377(C.c_size_t(1), None) == 2
    k = np.zeros(4, dtype=np.uint64)
    o = np.zeros(36, dtype=np.uint64)
    assert lib.groth16_hash_helper_prove_bls12_377(None, None, f._p(rows), C.c_size_t(1), C.c_int(0), C.c_uint(16), *([f._p(k)] * 6), f._p(o), f._p(o), f._p(o), f._p(o)) == 2
    assert lib.celo_amd_hash_helper_last(None) == 2


def test_address_and_ub_check_of_the_host_code_in_a_program_of_its_own(tmp_path):
    """tests/hashbits_asan_main.cpp: its own main, built with -fsanitize=address,undefined (the runtimes linked into the program), run as a subprocess - the CSR writer into arrays of
    exactly the sizes the query reports, and the host twin, at m = 1 and 3.  No sanitizer enters this process."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler to build tests/hashbits_asan_main.cpp")
    exe = str(tmp_path / "hashbits_asan")
    build = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                            "-I" + os.path.join(ROOT, "celo-bls-snark-rs_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "hashbits_asan_main.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "hashbits ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    sizes = circuit(3)[0]
    assert "m=3 constraints=%d vars=%d inputs=%d" % (sizes["n_constraints"], sizes["n_vars"], sizes["n_inputs"]) in run.stdout
