"""CPU (-m "not gpu"): the R1CS products and the Lagrange basis of csrc/r1cs.h, run through the host twins of host_test.cpp under bounds
tracking (a bound violation aborts the twin) - the validation of groth16_r1cs_load_*, the sums of unit_r1cs.hip's kernels in their short /
chunk / combine order, the blocked Lagrange evaluation - against the Python restatement in tests/groth16_setup_ref.py (witness_rows,
lagrange_at, qap_at).  Every comparison is whole-output and exact."""
import ctypes as C
import random
import numpy as np
import pytest
from oracle import cpu_oracle as co
import groth16_setup_ref as gs
import r1cs_cases as rc
from helpers import build_hosttest

NEW_SYMBOLS = ["groth16_r1cs_load_bw6_761", "groth16_r1cs_load_bls12_377", "groth16_r1cs_info", "groth16_r1cs_free", "groth16_r1cs_rows",
               "groth16_r1cs_rows_dev", "groth16_r1cs_check", "groth16_r1cs_qap_at_tau", "groth16_r1cs_qap_at_tau_dev",
               "groth16_prove_r1cs_with_key", "groth16_setup_r1cs_bw6_761", "groth16_setup_r1cs_bls12_377", "celo_amd_r1cs_last_timings"]
CURVES = ["bw6_761", "bls12_377"]


@pytest.fixture(scope="module")
def ht():
    lib = C.CDLL(build_hosttest())
    for name in ("ht_r1cs_rows", "ht_r1cs_lagrange", "ht_r1cs_cols", "ht_r1cs_params"):
        getattr(lib, name).restype = None
    lib.ht_r1cs_check_rows.restype = C.c_int64
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def cases(curve):
    from celo_bls_snark_rs_amd import ffi
    return [rc.toy(curve), rc.chain(curve, 40), rc.chain(curve, 62), rc.random_r1cs(curve, 3001, 1237, 5, 21, ffi.R1CS_CHUNK, ffi.R1CS_LONG)]


def host_validate(ht, case, mats=None, n_vars=None, n_inputs=None, nnz=None):
    mats = mats if mats is not None else case.csr()
    arr = lambda t, xs: (t * 3)(*[C.cast(_p(x), t) for x in xs])
    rp = arr(C.c_void_p, [m[0] for m in mats])
    col = arr(C.c_void_p, [m[1] for m in mats])
    val = arr(C.c_void_p, [m[2] for m in mats])
    nz = (C.c_uint64 * 3)(*(nnz if nnz is not None else [m[1].shape[0] for m in mats]))
    bad = C.c_uint64(0xdead)
    code = ht.ht_r1cs_validate(C.c_int(rc.CURVE_ID[case.curve]), C.c_size_t(case.m), C.c_size_t(case.n_vars if n_vars is None else n_vars),
                               C.c_size_t(case.n_inputs if n_inputs is None else n_inputs), rp, col, val, nz, C.byref(bad))
    return code, bad.value


def host_rows(ht, case, z, log_n):
    N = rc.N64[case.curve]
    zz = rc.mont(z, case.p)
    out = []
    for row_ptr, col, val in case.csr():
        o = np.zeros((1 << log_n, N), dtype=np.uint64)
        ht.ht_r1cs_rows(C.c_int(rc.CURVE_ID[case.curve]), _p(row_ptr), _p(col), _p(val), C.c_size_t(case.m), _p(zz), _p(o))
        out.append(o)
    out[0][case.m:case.m + case.n_inputs] = zz[:case.n_inputs]
    return out


def host_lagrange(ht, curve, log_n, omega, tau):
    p, N = gs.FIELDS[curve], rc.N64[curve]
    out = np.zeros((1 << log_n, N), dtype=np.uint64)
    zt = np.zeros(N, dtype=np.uint64)
    ht.ht_r1cs_lagrange(C.c_int(rc.CURVE_ID[curve]), C.c_uint(log_n), _p(rc.mont([omega], p)), _p(rc.mont([tau], p)), _p(out), _p(zt))
    return out, zt


def test_new_symbols_declared_and_exported():
    from celo_bls_snark_rs_amd import ffi
    lib = C.CDLL(ffi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in ffi.EXPORTS and hasattr(lib, name), name


def test_new_calls_refuse_without_a_device():
    import torch
    from celo_bls_snark_rs_amd import ffi
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    case = rc.toy("bw6_761")
    with pytest.raises(RuntimeError):
        ffi.R1CS.load("bw6_761", case.m, case.n_vars, case.n_inputs, case.csr())
    fake = ffi.R1CS.__new__(ffi.R1CS)
    fake.curve, fake.m, fake.n_vars, fake.n_inputs, fake.N, fake.h = "bw6_761", case.m, case.n_vars, case.n_inputs, 6, C.c_void_p()
    z6 = np.zeros(6, dtype=np.uint64)
    with pytest.raises(RuntimeError):
        fake.rows(np.zeros((case.n_vars, 6), dtype=np.uint64), 3)
    with pytest.raises(RuntimeError):
        fake.check(np.zeros((case.n_vars, 6), dtype=np.uint64))
    with pytest.raises(RuntimeError):
        fake.qap_at_tau(3, z6, z6)
    with pytest.raises(RuntimeError):
        ffi.groth16_setup_r1cs(fake, 3, z6, z6, np.zeros(24, dtype=np.uint64), np.zeros(24, dtype=np.uint64), np.zeros(24, dtype=np.uint64))
    key = ffi.ProvingKey("bw6_761", None, None, None, None, None, None)
    with pytest.raises(RuntimeError):
        key.prove_r1cs(fake, np.zeros((case.n_vars, 6), dtype=np.uint64), 3,
                       {k: z6 for k in ("omega", "omega_inv", "coset", "coset_inv", "size_inv", "vanishing_inv")})


def test_ffi_constants_match_the_header(ht):
    from celo_bls_snark_rs_amd import ffi
    out = (C.c_uint32 * 3)()
    ht.ht_r1cs_params(out)
    assert (out[0], out[1]) == (ffi.R1CS_LONG, ffi.R1CS_CHUNK)
    assert out[1] % 64 == 0 and out[0] < out[1]


@pytest.mark.parametrize("curve", CURVES)
def test_validate_accepts_the_cases_and_names_what_it_rejects(ht, curve):
    p = gs.FIELDS[curve]
    N = rc.N64[curve]
    for case in cases(curve):
        assert host_validate(ht, case) == (0, 0xdead), case.name
    case = cases(curve)[3]
    fresh = lambda: [tuple(a.copy() for a in m) for m in case.csr()]
    # a row whose end lies before its start (matrix b, row 77)
    mats = fresh()
    mats[1][0][78] = mats[1][0][77] - 1
    assert host_validate(ht, case, mats) == (34, (1 << 60) | 77)
    # row_ptr[m] != nnz (matrix c): one entry fewer than the offsets say
    mats = fresh()
    assert host_validate(ht, case, mats, nnz=[m[1].shape[0] - (k == 2) for k, m in enumerate(mats)]) == (34, (2 << 60) | case.m)
    # row_ptr[0] != 0 (matrix a)
    mats = fresh()
    mats[0][0][0] = 1
    assert host_validate(ht, case, mats) == (34, 0)
    # col == n_vars (matrix a, entry 1000)
    mats = fresh()
    mats[0][1][1000] = case.n_vars
    assert host_validate(ht, case, mats) == (34, 1000)
    # val == p, as raw limbs (matrix c, entry 5); p - 1 is accepted
    mats = fresh()
    mats[2][2][5] = co.ints_to_limbs([p], N)[0]
    assert host_validate(ht, case, mats) == (34, (2 << 60) | 5)
    mats[2][2][5] = co.ints_to_limbs([p - 1], N)[0]
    assert host_validate(ht, case, mats)[0] == 0
    # the shapes the setup also refuses with 2
    assert host_validate(ht, case, n_inputs=0)[0] == 2
    assert host_validate(ht, case, n_inputs=case.n_vars + 1)[0] == 2


@pytest.mark.parametrize("curve", CURVES)
def test_host_rows_match_witness_rows(ht, curve):
    """the case list includes a row of more than 3 chunks (chunk-and-combine), one of exactly the threshold and one just above it"""
    from celo_bls_snark_rs_amd import ffi
    for case in cases(curve):
        if case.name.startswith("random"):
            lens = np.diff(case.mats[0].row_ptr.astype(np.int64))
            assert lens.max() >= 3 * ffi.R1CS_CHUNK and lens.min() == 0
            assert ffi.R1CS_LONG in np.diff(case.mats[1].row_ptr.astype(np.int64)) and ffi.R1CS_LONG + 1 in np.diff(case.mats[2].row_ptr.astype(np.int64))
        z = rc.random_assignment(case, 3)
        for log_n in {case.log_n(), case.log_n() + 2}:             # m + n_inputs both close to and well below the domain size
            want = gs.witness_rows(*case.mats, z, case.n_inputs, log_n, case.p)
            got = host_rows(ht, case, z, log_n)
            for g, w in zip(got, want):
                assert np.array_equal(g, co.to_mont(w, case.p)), (case.name, log_n)


@pytest.mark.parametrize("curve", CURVES)
def test_host_lagrange_matches_lagrange_at(ht, curve):
    p = gs.FIELDS[curve]
    rng = random.Random(17)
    for log_n in (0, 2, 3, 6, 12):                                  # domains smaller than, equal to and larger than a lane's block
        omega = gs.root_of_unity(curve, log_n)
        tau = rng.randrange(2, p)
        got, zt = host_lagrange(ht, curve, log_n, omega, tau)
        assert np.array_equal(got, co.to_mont(gs.lagrange_at(tau, log_n, omega, p), p)), log_n
        assert np.array_equal(zt, co.to_mont([(pow(tau, 1 << log_n, p) - 1) % p], p)[0])
    # tau a domain point: the indicator vector, Z(tau) = 0, no division by zero
    log_n = 6
    omega = gs.root_of_unity(curve, log_n)
    for k in (3, 0, 63):
        got, zt = host_lagrange(ht, curve, log_n, omega, pow(omega, k, p))
        assert np.array_equal(got, co.to_mont([1 if j == k else 0 for j in range(1 << log_n)], p)), k
        assert not zt.any()


@pytest.mark.parametrize("curve", CURVES)
def test_host_cols_match_qap_at(ht, curve):
    """the transposes (column 0 and the hub columns are lists of many chunks) times L(tau), plus the input-consistency terms"""
    rng = random.Random(23)
    for case in cases(curve):
        p, N = case.p, rc.N64[curve]
        log_n = case.log_n()
        omega = gs.root_of_unity(curve, log_n)
        tau = rng.randrange(2, p)
        wa, wb, wc, wzt = gs.qap_at(*case.mats, case.n_vars, case.n_inputs, tau, log_n, omega, p)
        L, zt = host_lagrange(ht, curve, log_n, omega, tau)
        assert np.array_equal(zt, co.to_mont([wzt], p)[0])
        for k, ((row_ptr, col, val), want) in enumerate(zip(case.csr(), (wa, wb, wc))):
            out = np.zeros((case.n_vars, N), dtype=np.uint64)
            ht.ht_r1cs_cols(C.c_int(rc.CURVE_ID[curve]), _p(row_ptr), _p(col), _p(val), C.c_size_t(case.m), C.c_size_t(case.n_vars), _p(L),
                            C.c_size_t(case.n_inputs if k == 0 else 0), _p(out))
            assert np.array_equal(out, co.to_mont(want, p)), (case.name, k)


@pytest.mark.parametrize("curve", CURVES)
def test_host_check_finds_the_first_unsatisfied_constraint(ht, curve):
    case = rc.chain(curve, 40)
    p, N = case.p, rc.N64[curve]
    z = gs.squaring_witness(40, 3, p)
    run = lambda zz: ht.ht_r1cs_check_rows(C.c_int(rc.CURVE_ID[curve]), *[_p(o) for o in host_rows(ht, case, zz, case.log_n())], C.c_size_t(case.m))
    assert run(z) == -1
    bad = list(z)
    bad[2 + 20] = (bad[2 + 20] + 1) % p              # x_20: constraint 19 (its output) fails first, then 20
    assert run(bad) == 19
    bad[2 + 7] = (bad[2 + 7] + 1) % p
    assert run(bad) == 6
