"""CPU (-m "not gpu"): batched fixed-base scalar multiplication and the Groth16 setup's scalar preparation (csrc/fixed_base.h), run through
the host twins of host_test.cpp under bounds tracking - the table build, digit recoding, table lookup and accumulation of the kernels of
unit_setup.hip - against oracle/py/ecc and the Python restatement of ark-groth16 0.1's setup (tests/groth16_setup_ref.py), and a whole
Groth16 chain on the CPU: R1CS -> QAP at tau -> key rows by the host twins -> the oracle's prover -> the pairing check."""
import ctypes as C
import random
import numpy as np
import pytest
from oracle.py import ecc
from oracle.py import groth16_prover as gp
from oracle import cpu_oracle as co
import groth16_setup_ref as gs
from helpers import build_hosttest

NEW_SYMBOLS = ["fixed_base_mul_bls12_377_g1", "fixed_base_mul_bls12_377_g2", "fixed_base_mul_bw6_761_g1", "fixed_base_mul_bw6_761_g2",
               "fixed_base_mul_bls12_377_g1_dev", "fixed_base_mul_bls12_377_g2_dev", "fixed_base_mul_bw6_761_g1_dev", "fixed_base_mul_bw6_761_g2_dev",
               "normalize_bw6_761_g1", "normalize_bw6_761_g2", "groth16_setup_bw6_761", "groth16_setup_bls12_377",
               "celo_amd_fixed_base_set_window", "celo_amd_setup_last_timings"]
GROUPS = gs.GROUPS


@pytest.fixture(scope="module")
def ht():
    lib = C.CDLL(build_hosttest())
    lib.ht_fixed_base_mul.restype = None
    lib.ht_setup_scalars.restype = None
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_fbm(ht, group, gen, scalars, c):
    gid, curve, g, sw, aw = GROUPS[group]
    gen_rows, _ = gs.pack(curve, g, [gen])
    sc = co.ints_to_limbs(scalars, sw)
    out = np.zeros((len(scalars), aw), dtype=np.uint64)
    inf = np.zeros(len(scalars), dtype=np.uint8)
    ht.ht_fixed_base_mul(C.c_int(gid), _p(np.ascontiguousarray(gen_rows[0])), _p(sc), C.c_size_t(len(scalars)), C.c_int(c), _p(out), _p(inf))
    return out, inf


edge_scalars = gs.edge_scalars


def test_new_symbols_declared_and_exported():
    from celo_bls_snark_rs_amd import ffi
    lib = C.CDLL(ffi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in ffi.EXPORTS and hasattr(lib, name), name


@pytest.mark.parametrize("group", sorted(GROUPS))
@pytest.mark.parametrize("c", [5, 8, 10])
def test_host_fixed_base_mul_matches_oracle(ht, group, c):
    _, curve, g, _, _ = GROUPS[group]
    r, E1, E2, _, _, _ = gs.CURVES[curve]
    E = E1 if g == 1 else E2
    G = gs.generators(curve)[g - 1]
    rng = random.Random(hash((group, c)) & 0xffff)
    sc = edge_scalars(r, r.bit_length(), c, rng)
    for gen in (G, E.mul(G, 0xC0FFEE)):                       # the standard generator and another element of the subgroup
        out, inf = host_fbm(ht, group, gen, sc, c)
        want = [E.mul(gen, k) for k in sc]
        rows, winf = gs.pack(curve, g, want)
        assert inf.tolist() == winf.tolist() == [1 if k == 0 else 0 for k in sc]
        assert np.array_equal(out, rows), group


def test_lagrange_evaluation_interpolates():
    """sum_i L_i(tau) f(omega^i) = f(tau) for a polynomial of degree < n"""
    for curve in ("bw6_761", "bls12_377"):
        p = gs.FIELDS[curve]
        log_n = 5
        n, w = 1 << log_n, gs.root_of_unity(curve, log_n)
        rng = random.Random(7)
        f = [rng.randrange(p) for _ in range(n)]
        ev = lambda x: sum(c * pow(x, i, p) for i, c in enumerate(f)) % p
        tau = rng.randrange(p)
        L = gs.lagrange_at(tau, log_n, w, p)
        assert sum(l * ev(pow(w, i, p)) for i, l in enumerate(L)) % p == ev(tau)


def _setup_inputs(curve, circuit, seed):
    A, B, Cm, n_vars, n_in = circuit
    p = gs.FIELDS[curve]
    rng = random.Random(seed)
    log_n = gs.domain_log(len(A), n_in)
    tau = rng.randrange(2, p)
    a, b, c, zt = gs.qap_at(A, B, Cm, n_vars, n_in, tau, log_n, gs.root_of_unity(curve, log_n), p)
    toxic = [rng.randrange(1, p) for _ in range(4)]
    return {"a": a, "b": b, "c": c, "zt": zt, "tau": tau, "log_n": log_n, "n_h": (1 << log_n) - 1, "toxic": toxic, "n_vars": n_vars, "n_in": n_in}


def host_setup_scalars(ht, curve, s):
    p = gs.FIELDS[curve]
    N = 6 if curve == "bw6_761" else 4
    n_vars, n_in, n_h = s["n_vars"], s["n_in"], s["n_h"]
    q = [np.ascontiguousarray(co.to_mont(v, p)) for v in (s["a"], s["b"], s["c"])]
    zt, tau = co.to_mont([s["zt"]], p), co.to_mont([s["tau"]], p)
    tox = np.ascontiguousarray(co.to_mont(s["toxic"], p))
    n1, n2 = 3 + n_in + 2 * n_vars + n_h + (n_vars - n_in), 3 + n_vars
    g1 = np.zeros((n1, N), dtype=np.uint64)
    g2 = np.zeros((n2, N), dtype=np.uint64)
    ht.ht_setup_scalars(C.c_int(0 if curve == "bw6_761" else 1), _p(q[0]), _p(q[1]), _p(q[2]), C.c_size_t(n_vars), C.c_size_t(n_in), _p(zt), _p(tau),
                        C.c_size_t(n_h), _p(tox), _p(g1), _p(g2))
    return co.limbs_to_ints(g1, N), co.limbs_to_ints(g2, N)


@pytest.mark.parametrize("curve", ["bw6_761", "bls12_377"])
def test_host_setup_scalars_match_the_restatement(ht, curve):
    """the twin of k_setup_fr / k_setup_h (blocked powers of tau) against generate_parameters restated; n_h spans several blocks"""
    s = _setup_inputs(curve, gs.squaring_chain(90), 11)
    got1, got2 = host_setup_scalars(ht, curve, s)
    ref = gs.setup_scalars(s["a"], s["b"], s["c"], s["n_in"], s["zt"], s["tau"], s["n_h"], *s["toxic"], gs.FIELDS[curve])
    want1, want2 = gs.scalar_lists(ref, s["n_vars"], s["n_in"])
    assert got1 == want1 and got2 == want2


def test_cpu_groth16_round_trip_toy_circuit(ht):
    """x^3 + x + 5 = out over BW6-761: key rows by the host twins, the proof by oracle/py/groth16_prover, the pairing check by the oracle:
    e(A, B) = e(alpha, beta) e(vk_x, gamma) e(C, delta) holds for the right public input and fails for a wrong one"""
    curve = "bw6_761"
    p = gs.FIELDS[curve]
    circ = gs.toy_circuit()
    A, B, Cm, n_vars, n_in = circ
    s = _setup_inputs(curve, circ, 5)
    g1s, g2s = host_setup_scalars(ht, curve, s)
    G1, G2 = gs.generators(curve)
    r1, i1 = host_fbm(ht, "bw6_761_g1", G1, g1s, 8)
    r2, i2 = host_fbm(ht, "bw6_761_g2", G2, g2s, 8)
    key = gs.split_rows(curve, gs.ark_zero_fix(curve, r1, i1), gs.ark_zero_fix(curve, r2, i2), n_vars, n_in, s["n_h"])
    z = gs.toy_witness(3, p)
    log_n = s["log_n"]
    wa, wb, wc = gs.witness_rows(A, B, Cm, z, n_in, log_n, p)
    h = gp.witness_map(wa, wb, wc, log_n, gs.root_of_unity(curve, log_n), gs.coset_generator(p))
    k, v = key["rows"], key["vk"]
    proof = gp.prove_no_zk(k["a_query"], k["b_g2_query"], k["h_query"], k["l_query"], v["alpha_g1"], v["beta_g2"], z[1:], n_vars - n_in, h, threads=2)
    assert co.pairing_product_761(*gs.pairing_inputs(curve, v, proof, z[:n_in]))[1]
    assert not co.pairing_product_761(*gs.pairing_inputs(curve, v, proof, [1, (z[1] + 1) % p]))[1]
