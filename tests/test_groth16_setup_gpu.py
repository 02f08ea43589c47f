"""GPU: Groth16 parameter generation (groth16_setup_bw6_761 / _bls12_377, csrc/unit_setup.hip) and the whole chain it makes testable for the
first time: R1CS -> QAP at tau (tests/groth16_setup_ref.py) -> setup on the device -> witness map -> proof with the setup's key -> the
Groth16 pairing check on the device, e(A, B) = e(alpha, beta) e(vk_x, gamma) e(C, delta)."""
import random
import numpy as np
import pytest
import torch  # before the library: both must share one HIP runtime
from oracle.py import groth16_prover as gp
from oracle import cpu_oracle as co
import groth16_setup_ref as gs

pytestmark = pytest.mark.gpu
CURVES = ["bw6_761", "bls12_377"]


def setup_inputs(curve, circuit, seed):
    A, B, Cm, n_vars, n_in = circuit
    p = gs.FIELDS[curve]
    rng = random.Random(seed)
    log_n = gs.domain_log(len(A), n_in)
    tau = rng.randrange(2, p)
    a, b, c, zt = gs.qap_at(A, B, Cm, n_vars, n_in, tau, log_n, gs.root_of_unity(curve, log_n), p)
    return {"a": a, "b": b, "c": c, "zt": zt, "tau": tau, "log_n": log_n, "n_h": (1 << log_n) - 1, "toxic": [rng.randrange(1, p) for _ in range(4)],
            "n_vars": n_vars, "n_in": n_in}


def run_setup(gpu, curve, s, **kw):
    p = gs.FIELDS[curve]
    G1, G2 = gs.generators(curve)
    m = lambda v: co.to_mont(v, p)
    return gpu.groth16_setup(curve, m(s["a"]), m(s["b"]), m(s["c"]), s["n_in"], m([s["zt"]])[0], m([s["tau"]])[0], s["n_h"], m(s["toxic"]),
                             gs.pack(curve, 1, [G1])[0][0], gs.pack(curve, 2, [G2])[0][0], **kw)


def witness_map(gpu, curve, circuit, z, log_n):
    A, B, Cm, _, n_in = circuit
    p = gs.FIELDS[curve]
    wa, wb, wc = (co.to_mont(v, p) for v in gs.witness_rows(A, B, Cm, z, n_in, log_n, p))
    k = gp.domain_constants(log_n, gs.root_of_unity(curve, log_n), gs.coset_generator(p), p)
    consts = {name: co.to_mont([v], p)[0] for name, v in k.items()}
    fn = gpu.witness_map if curve == "bw6_761" else gpu.witness_map_fr377
    return fn(wa, wb, wc, log_n, consts, canonical=True)


def prove(gpu, key, curve, circuit, z, log_n):
    _, _, _, n_vars, n_in = circuit
    h = witness_map(gpu, curve, circuit, z, log_n)
    sw = 6 if curve == "bw6_761" else 4
    out = key.prove(co.ints_to_limbs(z[1:], sw), n_vars - n_in, h)
    kinds = ("761", "761", "761") if curve == "bw6_761" else ("g1_377", "g2_377", "g1_377")
    return tuple(co.jac_to_affine(o, k) for o, k in zip(out, kinds))


def verifies(gpu, curve, vk, proof, public):
    x1, i1, x2, i2 = gs.pairing_inputs(curve, vk, proof, public)
    return (gpu.pairing_product_is_one_bw6 if curve == "bw6_761" else gpu.pairing_product_is_one)(x1, i1, x2, i2)


@pytest.mark.parametrize("curve", CURVES)
def test_setup_rows_are_their_scalars_times_the_generator(gpu, curve):
    circ = gs.squaring_chain(40)
    s = setup_inputs(curve, circ, 3)
    p = gs.FIELDS[curve]
    out = run_setup(gpu, curve, s)
    ref = gs.setup_scalars(s["a"], s["b"], s["c"], s["n_in"], s["zt"], s["tau"], s["n_h"], *s["toxic"], p)
    _, E1, E2, _, _, _ = gs.CURVES[curve]
    G1, G2 = gs.generators(curve)
    for part in ("vk", "rows"):
        for name, rows in out[part].items():
            g2 = name.endswith("g2") or name == "b_g2_query"
            k = ref[name] if isinstance(ref[name], list) else [ref[name]]
            want = [(E2 if g2 else E1).mul(G2 if g2 else G1, x) for x in k]
            wrows, winf = gs.pack(curve, 2 if g2 else 1, want)
            assert np.array_equal(np.asarray(rows).reshape(wrows.shape), gs.ark_zero_fix(curve, wrows, winf)), name


@pytest.mark.wall_clock(1500)
@pytest.mark.parametrize("size", ["toy", "chain_2_16"])
@pytest.mark.parametrize("curve", CURVES)
def test_round_trip_setup_prove_verify(gpu, curve, size):
    p = gs.FIELDS[curve]
    if size == "toy":
        circ, z = gs.toy_circuit(), gs.toy_witness(3, p)
    else:
        circ, z = gs.squaring_chain(1 << 16), gs.squaring_witness(1 << 16, 7, p)
    s = setup_inputs(curve, circ, 11)
    out = run_setup(gpu, curve, s, want_key=True)
    key = out["key"]
    try:
        proof = prove(gpu, key, curve, circ, z, s["log_n"])
        assert verifies(gpu, curve, out["vk"], proof, z[:2])
        assert not verifies(gpu, curve, out["vk"], proof, [1, (z[1] + 1) % p])          # a wrong public input
        bad = list(z)
        bad[3] = (bad[3] + 1) % p                                                        # an unsatisfied witness
        assert not verifies(gpu, curve, out["vk"], prove(gpu, key, curve, circ, bad, s["log_n"]), z[:2])
        # the key built from out_rows by groth16_load_key_* proves the same; for BW6-761 also the serialized rows
        r, v = out["rows"], out["vk"]
        limb_key = gpu.ProvingKey(curve, r["a_query"], r["b_g2_query"], r["h_query"], r["l_query"], v["alpha_g1"], v["beta_g2"])
        assert prove(gpu, limb_key, curve, circ, z, s["log_n"]) == proof
        limb_key.release()
        if curve == "bw6_761" and size == "toy":
            import bw6_serial as bs
            pts = {name: gs.to_points(curve, 2 if name in bs.G2_FIELDS else 1, rows) for part in ("vk", "rows") for name, rows in out[part].items()}
            kd = {name: (pts[name] if name in ("gamma_abc_g1", "a_query", "b_g1_query", "b_g2_query", "h_query", "l_query") else pts[name][0])
                  for name in bs.SECTIONS}
            ser_key = gpu.ProvingKey.from_serialized(bs.ser_key(kd, 0))
            assert prove(gpu, ser_key, curve, circ, z, s["log_n"]) == proof
            ser_key.release()
    finally:
        key.release()


@pytest.mark.parametrize("curve", CURVES)
def test_setup_rejects_bad_arguments(gpu, curve):
    s = setup_inputs(curve, gs.toy_circuit(), 2)
    for change in ({"n_in": 0}, {"n_in": 7}, {"toxic": s["toxic"][:2] + [0] + s["toxic"][3:]}, {"toxic": s["toxic"][:3] + [0]}):
        with pytest.raises(gpu.SetupError) as e:
            run_setup(gpu, curve, dict(s, **change))
        assert e.value.code == 2
    with pytest.raises(gpu.SetupError) as e:
        run_setup(gpu, curve, s, want_vk=False, want_rows=False, want_key=False)
    assert e.value.code == 2


@pytest.mark.wall_clock(1500)
def test_bw6_761_setup_two_to_20_variables(gpu):
    """n_vars = 2^20 (random QAP values: the rows do not depend on a circuit), n_h = 2^20 - 1: every row checked by one random linear
    combination per group, sum_i w_i row_i = (sum_i w_i k_i) G"""
    curve, p = "bw6_761", gs.FIELDS["bw6_761"]
    n, n_in = 1 << 20, 2
    rng = random.Random(2020)
    s = {"a": [rng.randrange(p) for _ in range(n)], "b": [rng.randrange(p) for _ in range(n)], "c": [rng.randrange(p) for _ in range(n)],
         "zt": rng.randrange(p), "tau": rng.randrange(p), "n_h": n - 1, "toxic": [rng.randrange(1, p) for _ in range(4)], "n_vars": n, "n_in": n_in}
    out = run_setup(gpu, curve, s)
    alpha, beta, gamma, delta = s["toxic"]
    gi, di = pow(gamma, -1, p), pow(delta, -1, p)
    lc = [(beta * x + alpha * y + z) % p for x, y, z in zip(s["a"], s["b"], s["c"])]
    h, cur = [], s["zt"] * di % p
    for _ in range(n - 1):
        h.append(cur)
        cur = cur * s["tau"] % p
    g1_scalars = [alpha, beta, delta] + [v * gi % p for v in lc[:n_in]] + s["a"] + s["b"] + h + [v * di % p for v in lc[n_in:]]
    g2_scalars = [beta, gamma, delta] + s["b"]
    v, r = out["vk"], out["rows"]
    g1_rows = np.concatenate([v["alpha_g1"][None], r["beta_g1"][None], r["delta_g1"][None], v["gamma_abc_g1"], r["a_query"], r["b_g1_query"],
                              r["h_query"], r["l_query"]])
    g2_rows = np.concatenate([v["beta_g2"][None], v["gamma_g2"][None], v["delta_g2"][None], r["b_g2_query"]])
    _, E1, E2, _, _, _ = gs.CURVES[curve]
    G1, G2 = gs.generators(curve)
    for rows, k, E, G, group in ((g1_rows, g1_scalars, E1, G1, "bw6_761_g1"), (g2_rows, g2_scalars, E2, G2, "bw6_761_g2")):
        assert rows.shape[0] == len(k)
        w = [rng.getrandbits(64) for _ in range(len(k))]
        inf = gp.ark_zero_rows(rows, gs.CURVES[curve][3], 12)
        lhs = co.jac_to_affine(co.msm(group, np.ascontiguousarray(rows), inf, co.ints_to_limbs(w, 6), threads=16), "761")
        assert lhs == E.mul(G, sum(a * b for a, b in zip(w, k)) % p), group
    t = gpu.setup_timings()
    assert t["g1_rows"] > 0 and t["g2_rows"] > 0 and t["wall"] > 0
