"""GPU: R1CS matrices on the device (groth16_r1cs_*, csrc/unit_r1cs.hip) and the two chained entry points they make possible
(groth16_prove_r1cs_with_key, groth16_setup_r1cs_*), against the Python restatement in tests/groth16_setup_ref.py.  Integer arithmetic:
every comparison is exact (np.array_equal on limbs) and covers the whole output."""
import ctypes as C
import random
import threading
import numpy as np
import pytest
import torch  # before the library: both must share one HIP runtime
from oracle.py import groth16_prover as gp
from oracle import cpu_oracle as co
import groth16_setup_ref as gs
import r1cs_cases as rc

pytestmark = pytest.mark.gpu
CURVES = ["bw6_761", "bls12_377"]


def load(gpu, case):
    return gpu.R1CS.load(case.curve, case.m, case.n_vars, case.n_inputs, case.csr())


def domain_consts(curve, log_n):
    p = gs.FIELDS[curve]
    k = gp.domain_constants(log_n, gs.root_of_unity(curve, log_n), gs.coset_generator(p), p)
    return {name: co.to_mont([v], p)[0] for name, v in k.items()}


def check_products(gpu, case, log_n, seed):
    """rows and qap_at_tau of one case against witness_rows / qap_at, whole outputs"""
    p = case.p
    rng = random.Random(seed)
    r = load(gpu, case)
    try:
        info = r.info()
        assert (info["n_constraints"], info["n_vars"], info["n_inputs"]) == (case.m, case.n_vars, case.n_inputs)
        assert [info["nnz_a"], info["nnz_b"], info["nnz_c"]] == [M.col.shape[0] for M in case.mats] and info["device_bytes"] > 0
        z = rc.random_assignment(case, seed)
        got = r.rows(rc.mont(z, p), log_n)
        want = gs.witness_rows(*case.mats, z, case.n_inputs, log_n, p)
        for k in range(3):
            assert np.array_equal(got[k], co.to_mont(want[k], p)), (case.name, "rows", k)
        del got, want
        omega, tau = gs.root_of_unity(case.curve, log_n), rng.randrange(2, p)
        a, b, c, zt = r.qap_at_tau(log_n, rc.mont([omega], p)[0], rc.mont([tau], p)[0])
        wa, wb, wc, wzt = gs.qap_at(*case.mats, case.n_vars, case.n_inputs, tau, log_n, omega, p)
        assert np.array_equal(zt, co.to_mont([wzt], p)[0])
        for k, (g, w) in enumerate(((a, wa), (b, wb), (c, wc))):
            assert np.array_equal(g, co.to_mont(w, p)), (case.name, "qap", k)
    finally:
        r.release()


@pytest.mark.parametrize("curve", CURVES)
def test_small_cases_match_the_restatement(gpu, curve):
    for case in (rc.toy(curve), rc.chain(curve, 40), rc.chain(curve, 62)):
        check_products(gpu, case, case.log_n(), 5)
        check_products(gpu, case, case.log_n() + 3, 6)                  # m + n_inputs well below the domain size
    case = rc.chain(curve, 62)
    r = load(gpu, case)
    try:
        with pytest.raises(RuntimeError, match="code 2"):               # a domain smaller than m + n_inputs
            r.rows(rc.mont(rc.random_assignment(case, 1), case.p), 5)
    finally:
        r.release()


@pytest.mark.parametrize("curve", CURVES)
def test_qap_at_a_domain_point_is_the_indicator(gpu, curve):
    """tau = omega^3: L_j = [j == 3] and Z(tau) = 0, so a_i(tau) = A[3][i] (+ nothing: 3 < m), no division by zero"""
    case = rc.chain(curve, 40)
    p, log_n = case.p, case.log_n()
    omega = gs.root_of_unity(curve, log_n)
    r = load(gpu, case)
    try:
        a, b, c, zt = r.qap_at_tau(log_n, rc.mont([omega], p)[0], rc.mont([pow(omega, 3, p)], p)[0])
    finally:
        r.release()
    assert not zt.any()
    for got, M in zip((a, b, c), case.mats):
        want = [0] * case.n_vars
        for v, k in M.row(3).items():
            want[v] = (want[v] + k) % p
        assert np.array_equal(got, co.to_mont(want, p))


@pytest.mark.wall_clock(1500)
@pytest.mark.parametrize("curve,log_n", [("bw6_761", 12), ("bls12_377", 12), ("bw6_761", 16), ("bls12_377", 16), ("bw6_761", 20), ("bls12_377", 20)])
def test_random_r1cs_whole_outputs(gpu, curve, log_n):
    """skewed lists both ways (a row of 3 chunks + 37 terms; column 0 in over half of all constraints and two hub columns in a tenth), m and
    n_vars not multiples of 64, m + n_inputs a few rows below the domain size"""
    n = 1 << log_n
    case = rc.random_r1cs(curve, n - 7 - 13, (n * 3) // 5 + 3, 7, 100 + log_n, gpu.R1CS_CHUNK, gpu.R1CS_LONG)
    assert case.m % 64 and case.n_vars % 64 and case.m + case.n_inputs < n
    check_products(gpu, case, log_n, log_n)


@pytest.mark.parametrize("curve", CURVES)
def test_check_names_the_first_unsatisfied_constraint(gpu, curve):
    m = 5000
    case = rc.chain(curve, m)
    p = case.p
    z = gs.squaring_witness(m, 3, p)
    r = load(gpu, case)
    try:
        assert r.check(rc.mont(z, p)) == -1
        bad = list(z)
        bad[2 + 4100] = (bad[2 + 4100] + 1) % p               # x_4100: its defining constraint 4099 fails, and 4100
        assert r.check(rc.mont(bad, p)) == 4099
        bad[2 + 17] = (bad[2 + 17] + 1) % p                   # two separate failures: the smallest index
        assert r.check(rc.mont(bad, p)) == 16
    finally:
        r.release()


@pytest.mark.parametrize("curve", CURVES)
def test_load_rejections(gpu, curve):
    case = rc.random_r1cs(curve, 3001, 1237, 5, 21, gpu.R1CS_CHUNK, gpu.R1CS_LONG)
    p, N = case.p, rc.N64[curve]
    fresh = lambda: [tuple(a.copy() for a in m) for m in case.csr()]

    def rejected(mats, code, first_bad, **kw):
        with pytest.raises(gpu.R1CSLoadError) as e:
            gpu.R1CS.load(curve, case.m, kw.get("n_vars", case.n_vars), kw.get("n_inputs", case.n_inputs), mats)
        assert (e.value.code, e.value.first_bad) == (code, first_bad)

    mats = fresh()
    mats[1][0][78] = mats[1][0][77] - 1
    rejected(mats, 34, (1 << 60) | 77)
    mats = fresh()
    mats[2] = (mats[2][0], mats[2][1][:-1].copy(), mats[2][2][:-1].copy())         # row_ptr[m] != nnz
    rejected(mats, 34, (2 << 60) | case.m)
    mats = fresh()
    mats[0][1][1000] = case.n_vars
    rejected(mats, 34, 1000)
    mats = fresh()
    mats[2][2][5] = co.ints_to_limbs([p], N)[0]
    rejected(mats, 34, (2 << 60) | 5)
    rejected(fresh(), 2, None, n_inputs=0)
    rejected(fresh(), 2, None, n_inputs=case.n_vars + 1)
    # *out_r1cs stays NULL after a rejection (the raw call: R1CS.__init__ would hide it), and a following valid load works
    mats = fresh()
    mats[0][1][1000] = case.n_vars
    keep, args = gpu._csr_args(mats, N)
    h, bad = C.c_void_p(0x1234), C.c_uint64(0)
    code = getattr(gpu.lib(), "groth16_r1cs_load_" + curve)(C.c_size_t(case.m), C.c_size_t(case.n_vars), C.c_size_t(case.n_inputs), *args, C.byref(h), C.byref(bad))
    assert (code, h.value, bad.value) == (34, None, 1000)
    check_products(gpu, case, 12, 9)


def test_key_and_circuit_of_different_curves(gpu):
    """a BW6-761 key with a BLS12-377 circuit, and groth16_setup_r1cs_bw6_761 on a BLS12-377 circuit: code 2 before anything is read"""
    p = gs.FIELDS["bw6_761"]
    case = rc.toy("bw6_761")
    r, other = load(gpu, case), load(gpu, rc.toy("bls12_377"))
    try:
        out, _, _ = setup_from_matrices(gpu, r, case, 3, 4, want_vk=False, want_rows=False, want_key=True)
        key = out["key"]
        try:
            buf = np.zeros(64, dtype=np.uint64)
            ptr = buf.ctypes.data_as(C.c_void_p)
            assert gpu.lib().groth16_prove_r1cs_with_key(key.h, other.h, ptr, C.c_uint(3), *([ptr] * 6), *([ptr] * 3)) == 2
            assert gpu.lib().groth16_setup_r1cs_bw6_761(other.h, C.c_uint(3), *([ptr] * 5), C.c_int(0), ptr, None, None) == 2
            # ... and the same key with its own circuit proves
            z = gs.toy_witness(3, p)
            assert affine("bw6_761", key.prove_r1cs(r, rc.mont(z, p), 3, domain_consts("bw6_761", 3))) == piecewise_proof(gpu, key, case, z, 3)
        finally:
            key.release()
    finally:
        r.release()
        other.release()


def affine(curve, out):
    kinds = ("761", "761", "761") if curve == "bw6_761" else ("g1_377", "g2_377", "g1_377")
    return tuple(co.jac_to_affine(o, k) for o, k in zip(out, kinds))


def piecewise_proof(gpu, key, case, z, log_n):
    """witness_rows in Python -> witness_map(canonical) -> key.prove"""
    p, curve = case.p, case.curve
    wa, wb, wc = (co.to_mont(v, p) for v in gs.witness_rows(*case.mats, z, case.n_inputs, log_n, p))
    fn = gpu.witness_map if curve == "bw6_761" else gpu.witness_map_fr377
    h = fn(wa, wb, wc, log_n, domain_consts(curve, log_n), canonical=True)
    return affine(curve, key.prove(co.ints_to_limbs(z[1:], rc.N64[curve]), case.n_vars - case.n_inputs, h))


def verifies(gpu, curve, vk, proof, public):
    x1, i1, x2, i2 = gs.pairing_inputs(curve, vk, proof, public)
    return (gpu.pairing_product_is_one_bw6 if curve == "bw6_761" else gpu.pairing_product_is_one)(x1, i1, x2, i2)


def setup_from_matrices(gpu, r, case, log_n, seed, **kw):
    p, curve = case.p, case.curve
    rng = random.Random(seed)
    G1, G2 = gs.generators(curve)
    tau, toxic = rng.randrange(2, p), [rng.randrange(1, p) for _ in range(4)]
    out = gpu.groth16_setup_r1cs(r, log_n, rc.mont([gs.root_of_unity(curve, log_n)], p)[0], rc.mont([tau], p)[0], rc.mont(toxic, p),
                                 gs.pack(curve, 1, [G1])[0][0], gs.pack(curve, 2, [G2])[0][0], **kw)
    return out, tau, toxic


def witness_of(case, size, x0):
    return gs.toy_witness(x0, case.p) if size == "toy" else gs.squaring_witness(case.m, x0, case.p)


SIZES = {"toy": None, "chain_2_16": 1 << 16, "chain_2_20": (1 << 20) - 2}


def case_of(curve, size):
    return rc.toy(curve) if size == "toy" else rc.chain(curve, SIZES[size])


@pytest.mark.wall_clock(1500)
@pytest.mark.parametrize("curve,size", [("bw6_761", "toy"), ("bls12_377", "toy"), ("bw6_761", "chain_2_16"), ("bls12_377", "chain_2_16"),
                                        ("bw6_761", "chain_2_20")])
def test_round_trip_from_matrices(gpu, curve, size):
    """nothing computed in Python but the witness and vk_x: groth16_setup_r1cs (want_key) -> prove_r1cs -> the pairing check accepts, rejects a
    wrong public input and rejects the proof of an unsatisfied witness (which check() names); up to chain_2_16 the chained proof also equals
    the piecewise one (witness_rows in Python -> witness_map -> key.prove) as affine points"""
    case = case_of(curve, size)
    p, log_n = case.p, case.log_n()
    if size == "chain_2_20":
        assert case.m + case.n_inputs == 1 << 20
    z = witness_of(case, size, 7)
    r = load(gpu, case)
    try:
        out, _, _ = setup_from_matrices(gpu, r, case, log_n, 11, want_rows=False, want_key=True)
        key = out["key"]
        try:
            consts = domain_consts(curve, log_n)
            proof = affine(curve, key.prove_r1cs(r, rc.mont(z, p), log_n, consts))
            assert verifies(gpu, curve, out["vk"], proof, z[:case.n_inputs])
            assert not verifies(gpu, curve, out["vk"], proof, [1, (z[1] + 1) % p])
            bad = list(z)
            bad[3] = (bad[3] + 1) % p
            assert r.check(rc.mont(z, p)) == -1 and r.check(rc.mont(bad, p)) >= 0
            assert not verifies(gpu, curve, out["vk"], affine(curve, key.prove_r1cs(r, rc.mont(bad, p), log_n, consts)), z[:case.n_inputs])
            if size != "chain_2_20":
                assert piecewise_proof(gpu, key, case, z, log_n) == proof
            assert gpu.r1cs_timings()["prove_r1cs_wall"] > 0
        finally:
            key.release()
    finally:
        r.release()


@pytest.mark.parametrize("curve", CURVES)
def test_setup_from_matrices_equals_setup_from_qap_at(gpu, curve):
    """chain(40): the vk and rows of groth16_setup_r1cs equal those of groth16_setup fed with qap_at's output, bit for bit"""
    case = rc.chain(curve, 40)
    p, log_n = case.p, case.log_n()
    r = load(gpu, case)
    try:
        got, tau, toxic = setup_from_matrices(gpu, r, case, log_n, 3)
    finally:
        r.release()
    a, b, c, zt = gs.qap_at(*case.mats, case.n_vars, case.n_inputs, tau, log_n, gs.root_of_unity(curve, log_n), p)
    G1, G2 = gs.generators(curve)
    m = lambda v: co.to_mont(v, p)
    want = gpu.groth16_setup(curve, m(a), m(b), m(c), case.n_inputs, m([zt])[0], m([tau])[0], (1 << log_n) - 1, m(toxic),
                             gs.pack(curve, 1, [G1])[0][0], gs.pack(curve, 2, [G2])[0][0])
    for part in ("vk", "rows"):
        assert sorted(got[part]) == sorted(want[part])
        for name in want[part]:
            assert np.array_equal(got[part][name], want[part][name]), name


@pytest.mark.wall_clock(1500)
def test_two_to_22_rows_and_the_identity_of_the_two_products(gpu):
    """BW6-761, random_r1cs at log_n = 22 (about 4 terms per row).  rows() against witness_rows on the whole output (the count asserted)
    and, on whole outputs, the identity that ties the two products:
        sum_i w_i a_i(tau) == sum_j L_j (A w)_j + sum_(i < n_inputs) w_i L_(m + i)      (likewise b, c without the last sum)
    for a random vector w, the left side from qap_at_tau, (A w) from rows, L recomputed in Python."""
    curve, log_n = "bw6_761", 22
    n = 1 << log_n
    case = rc.random_r1cs(curve, n - 7 - 29, (n * 3) // 5 + 3, 7, 2222, gpu.R1CS_CHUNK, gpu.R1CS_LONG)
    p = case.p
    rng = random.Random(22)
    w = rc.random_assignment(case, 77)
    r = load(gpu, case)
    try:
        rows = r.rows(rc.mont(w, p), log_n)
        omega, tau = gs.root_of_unity(curve, log_n), rng.randrange(2, p)
        qa, qb, qc, zt = r.qap_at_tau(log_n, rc.mont([omega], p)[0], rc.mont([tau], p)[0])
        t = gpu.r1cs_timings()
    finally:
        r.release()
    assert t["rows"] > 0 and t["lagrange"] > 0 and t["columns"] > 0
    # rows, whole output (about a minute of Python at this size: inside the wall-clock mark, so nothing is sampled)
    assert sum(int(np.count_nonzero(np.diff(M.row_ptr.astype(np.int64)) > gpu.R1CS_LONG)) for M in case.mats) >= 2
    want = gs.witness_rows(*case.mats, w, case.n_inputs, log_n, p)
    compared = 0
    for k in range(3):
        assert len(want[k]) == n and rows[k].shape[0] == n
        assert np.array_equal(rows[k], co.to_mont(want[k], p)), k
        compared += n
    assert compared == 3 * n
    print("rows compared against witness_rows: all %d rows of each of the three outputs" % n)
    del want
    # the tail of the rows: the input-consistency rows, then zeros
    assert np.array_equal(rows[0][case.m:case.m + case.n_inputs], co.to_mont(w[:case.n_inputs], p))
    assert not rows[0][case.m + case.n_inputs:].any() and not rows[1][case.m:].any() and not rows[2][case.m:].any()
    # the identity, whole outputs
    assert np.array_equal(zt, co.to_mont([(pow(tau, n, p) - 1) % p], p)[0])
    L = gs.lagrange_at(tau, log_n, omega, p)
    extra = sum(w[i] * L[case.m + i] for i in range(case.n_inputs)) % p
    for k, (q, rw) in enumerate(((qa, rows[0]), (qb, rows[1]), (qc, rows[2]))):
        lhs = sum(x * y for x, y in zip(w, co.from_mont(q, p))) % p
        rhs = sum(x * y for x, y in zip(L[:case.m], co.from_mont(rw[:case.m], p))) % p
        assert lhs == (rhs + (extra if k == 0 else 0)) % p, k


@pytest.mark.parametrize("curve", CURVES)
def test_two_threads_share_a_key_and_a_circuit(gpu, curve):
    case = rc.chain(curve, 1 << 12)
    p, log_n = case.p, case.log_n()
    zs = [rc.mont(gs.squaring_witness(case.m, x0, p), p) for x0 in (3, 5)]
    r = load(gpu, case)
    try:
        out, _, _ = setup_from_matrices(gpu, r, case, log_n, 8, want_vk=False, want_rows=False, want_key=True)
        key = out["key"]
        try:
            consts = domain_consts(curve, log_n)
            single = [affine(curve, key.prove_r1cs(r, z, log_n, consts)) for z in zs]
            got, errs = [None, None], []

            def work(i):
                try:
                    gpu.use_device(0)
                    for _ in range(3):
                        got[i] = affine(curve, key.prove_r1cs(r, zs[i], log_n, consts))
                except Exception as e:      # noqa: BLE001  (reported by the assertion below)
                    errs.append(e)

            ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
            for t in ts:
                t.start()
            for t in ts:
                t.join()
            assert not errs, errs
            assert got == single
        finally:
            key.release()
    finally:
        r.release()


@pytest.mark.parametrize("curve", CURVES)
def test_host_and_device_forms_of_rows_and_qap_at_tau(gpu, curve):
    """the smallest case and a chain of 65 constraints (one row past a 64-lane wave): groth16_r1cs_rows / _qap_at_tau and their _dev forms
    return the same bytes, every byte of the device buffers written"""
    for case in (rc.toy(curve), rc.chain(curve, 65)):
        p, log_n, N = case.p, case.log_n(), 6 if curve == "bw6_761" else 4
        n = 1 << log_n
        z = rc.mont(rc.random_assignment(case, 9), p)
        omega, tau = rc.mont([gs.root_of_unity(curve, log_n)], p)[0], rc.mont([random.Random(10).randrange(2, p)], p)[0]
        r = load(gpu, case)
        try:
            rows = r.rows(z, log_n)
            a, b, c, zt = r.qap_at_tau(log_n, omega, tau)
            d_z = torch.from_numpy(np.ascontiguousarray(z, dtype=np.uint64).view(np.int64).copy()).cuda()
            d_rows = [torch.full((n * N,), 0x5A5A5A5A, dtype=torch.int64, device="cuda") for _ in range(3)]
            d_qap = [torch.full((case.n_vars * N,), 0x5A5A5A5A, dtype=torch.int64, device="cuda") for _ in range(3)]
            torch.cuda.synchronize()
            r.rows_dev(d_z.data_ptr(), log_n, *[t.data_ptr() for t in d_rows])
            zt_dev = r.qap_at_tau_dev(log_n, omega, tau, *[t.data_ptr() for t in d_qap])
            torch.cuda.synchronize()
        finally:
            r.release()
        for k in range(3):
            assert np.array_equal(d_rows[k].cpu().numpy().view(np.uint64).reshape(n, N), rows[k]), (case.name, "rows", k)
            assert np.array_equal(d_qap[k].cpu().numpy().view(np.uint64).reshape(case.n_vars, N), (a, b, c)[k]), (case.name, "qap", k)
        assert np.array_equal(zt_dev, zt)
