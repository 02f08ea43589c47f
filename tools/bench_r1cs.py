"""R1CS matrices on the device (csrc/unit_r1cs.hip): load time, the two products against their floors, the Lagrange step, the skew ratio, and
the chained entry points against the piecewise paths they replace.

  python tools/bench_r1cs.py [--sizes 20,22] [--reps 5] [--proofs 11] [--out profiles/bench_r1cs.json]

Per case (BW6-761 at every --sizes: the squaring chain, random_r1cs of tests/r1cs_cases.py - skewed: column 0 in over half of all
constraints - and an evenly loaded matrix of 4 terms per row; BLS12-377 at the first size: random_r1cs):
  load_ms        groth16_r1cs_load_* (host wall: validation, transposition, binning, copies)
  rows / columns kernel time of the three products (HIP events, best of --reps), non-zeros/s, and the time two floors would take:
      bytes_floor   nnz x (4 + 8 N64) matrix bytes + one gathered vector element per non-zero + the outputs, over the device-to-device copy
                    rate timed in this run (1 GiB copied, read + write counted);
      mul_floor     products over celo_amd_ubench_fp's Fq377 product rate of this run (BW6-761 only: the 253-bit field has no entry there) -
                    for the GENERAL coefficients only (not 0, 1 or p - 1: what a tagged fast path would leave) and for every non-zero (what
                    the kernels do today);
      each as floor / measured (1.0 = at the floor)
  lagrange_ms    the Lagrange kernel
skew: (time per non-zero, random_r1cs) / (time per non-zero, even) for rows and columns.
chained (the first size, BW6-761, chain): median of --proofs runs after a warm-up of groth16_prove_r1cs_with_key against the piecewise path in
the same process with the same key - groth16_witness_map_bw6_761 on host a, b, c (made before, NOT timed) then groth16_prove_with_key - and
one groth16_setup_r1cs against groth16_setup fed from host vectors.  Exit status 1 if the chained proof is slower than 1.03 x piecewise."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: both must share one HIP runtime)
from oracle.py import groth16_prover as gp  # noqa: E402
from oracle import cpu_oracle as co  # noqa: E402
from celo_bls_snark_rs_amd import ffi  # noqa: E402
import groth16_setup_ref as gs  # noqa: E402
import r1cs_cases as rc  # noqa: E402


def copy_rate_gbs():
    n = 1 << 30
    a = torch.zeros(n, dtype=torch.uint8, device="cuda")
    b = torch.empty(n, dtype=torch.uint8, device="cuda")
    b.copy_(a)
    best = None
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); b.copy_(a); e1.record(); e1.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None or ms < best else best
    del a, b
    torch.cuda.empty_cache()
    return 2 * n / (best * 1e-3) / 1e9


def csr_case(curve, mats, n_vars, n_inputs, name):
    return rc.Case(curve, [rc.CsrMatrix(rp.astype(np.uint64), col.astype(np.uint32), kind.astype(np.int64), table) for rp, col, kind, table in mats],
                   n_vars, n_inputs, name)


def chain_case(curve, m):
    """gs.squaring_chain(m) as arrays (x_k x_k = x_(k+1), the last output the public input)"""
    rp, k = np.arange(m + 1), np.arange(m)
    c_col = np.where(k + 1 < m, 3 + k, 1)
    return csr_case(curve, [(rp, 2 + k, np.zeros(m), [1]), (rp, 2 + k, np.zeros(m), [1]), (rp, c_col, np.zeros(m), [1])], m + 2, 2, "chain")


def even_case(curve, m, n_vars, n_inputs, seed, terms=4):
    """every row `terms` uniformly drawn columns, coefficients drawn as random_r1cs draws them: no long list in either direction"""
    table, w = rc.coefficient_table(gs.FIELDS[curve], seed)
    rng = np.random.default_rng(seed)
    mats = []
    for _ in range(3):
        mats.append((np.arange(m + 1) * terms, rng.integers(0, n_vars, size=m * terms), rng.choice(len(table), size=m * terms, p=w), table))
    return csr_case(curve, mats, n_vars, n_inputs, "even")


def general_count(case):
    """non-zeros whose coefficient is not 0, 1 or p - 1"""
    total = 0
    for M in case.mats:
        special = [i for i, v in enumerate(M.table) if v in (0, 1, case.p - 1)]
        total += int(np.count_nonzero(~np.isin(M.kind, special)))
    return total


def measure(case, log_n, reps, copy_gbs, mul_g):
    p, N = case.p, rc.N64[case.curve]
    r = ffi.R1CS.load(case.curve, case.m, case.n_vars, case.n_inputs, case.csr())
    load_ms = ffi.r1cs_timings()["load"]
    info = r.info()
    nnz = info["nnz_a"] + info["nnz_b"] + info["nnz_c"]
    general = general_count(case)
    n = 1 << log_n
    rng = np.random.default_rng(5)
    z = rng.integers(0, 1 << 62, size=(case.n_vars, N), dtype=np.int64).astype(np.uint64)
    z[:, N - 1] &= np.uint64((1 << 56) - 1)
    d_z = torch.from_numpy(z.view(np.int64)).cuda()
    d_o = [torch.empty((n, N), dtype=torch.int64, device="cuda") for _ in range(3)]
    omega, tau = rc.mont([gs.root_of_unity(case.curve, log_n)], p)[0], z[1].copy()
    best = {"rows": None, "lagrange": None, "columns": None}
    for _ in range(reps + 1):                      # the first run is the warm-up
        r.rows_dev(d_z.data_ptr(), log_n, *[o.data_ptr() for o in d_o])
        t_rows = ffi.r1cs_timings()["rows"]
        r.qap_at_tau_dev(log_n, omega, tau, *[o.data_ptr() for o in d_o])
        t = dict(ffi.r1cs_timings(), rows=t_rows)
        for k in best:
            best[k] = t[k] if best[k] is None or t[k] < best[k] else best[k]
    r.release()
    del d_z, d_o
    torch.cuda.empty_cache()
    out = {"case": case.name, "curve": case.curve, "log_n": log_n, "n_constraints": case.m, "n_vars": case.n_vars, "nnz": nnz, "general_coefficients": general,
           "device_bytes": info["device_bytes"], "load_ms": round(load_ms, 2), "lagrange_ms": round(best["lagrange"], 3)}
    for name, outputs in (("rows", 3 * case.m), ("columns", 3 * case.n_vars)):
        ms = best[name]
        byts = nnz * (4 + 8 * N) + nnz * 8 * N + outputs * 8 * N
        d = {"kernel_ms": round(ms, 3), "nnz_per_s": nnz / ms * 1e3, "bytes_floor_ms": byts / (copy_gbs * 1e9) * 1e3}
        d["bytes_floor_frac"] = d["bytes_floor_ms"] / ms
        if mul_g:
            d["mul_floor_general_ms"] = general / (mul_g * 1e9) * 1e3
            d["mul_floor_all_ms"] = nnz / (mul_g * 1e9) * 1e3
            d["mul_floor_general_frac"] = d["mul_floor_general_ms"] / ms
            d["mul_floor_all_frac"] = d["mul_floor_all_ms"] / ms
        out[name] = d
    return out


def chained(log_n, proofs):
    curve, p, N = "bw6_761", gs.FIELDS["bw6_761"], 6
    n = 1 << log_n
    case = chain_case(curve, n - 2)
    z = gs.squaring_witness(case.m, 7, p)
    zm, zc = rc.mont(z, p), np.ascontiguousarray(co.ints_to_limbs(z[1:], N))
    G1, G2 = gs.generators(curve)
    g1, g2 = gs.pack(curve, 1, [G1])[0][0], gs.pack(curve, 2, [G2])[0][0]
    omega, tau, tox = rc.mont([gs.root_of_unity(curve, log_n)], p)[0], rc.mont([0x1234567], p)[0], rc.mont([3, 5, 7, 11], p)
    k = gp.domain_constants(log_n, gs.root_of_unity(curve, log_n), gs.coset_generator(p), p)
    consts = {name: co.to_mont([v], p)[0] for name, v in k.items()}
    names = ("omega", "omega_inv", "coset", "coset_inv", "size_inv", "vanishing_inv")
    r = ffi.R1CS.load(curve, case.m, case.n_vars, case.n_inputs, case.csr())
    res = {"log_n": log_n, "n_constraints": case.m, "n_vars": case.n_vars}
    # setup: from the matrices, and from host vectors (the vectors made before, not timed)
    t0 = time.perf_counter()
    out = ffi.groth16_setup_r1cs(r, log_n, omega, tau, tox, g1, g2, want_vk=False, want_rows=False, want_key=True)
    res["setup_r1cs_s"] = time.perf_counter() - t0
    res["setup_r1cs_qap_ms"] = {k2: round(v, 3) for k2, v in ffi.r1cs_timings().items() if k2 in ("lagrange", "columns")}
    key = out["key"]
    qa, qb, qc, zt = r.qap_at_tau(log_n, omega, tau)
    t0 = time.perf_counter()
    out2 = ffi.groth16_setup(curve, qa, qb, qc, case.n_inputs, zt, tau, n - 1, tox, g1, g2, want_vk=False, want_rows=False, want_key=True)
    res["setup_host_vectors_s"] = time.perf_counter() - t0
    out2["key"].release()
    del qa, qb, qc
    # proofs
    rows = r.rows(zm, log_n)
    lib, P = ffi.lib(), lambda a: a.ctypes.data_as(C.c_void_p)
    kc = [np.ascontiguousarray(consts[nm], dtype=np.uint64) for nm in names]
    outs = [np.zeros(36, dtype=np.uint64) for _ in range(3)]

    def run_chained():
        t0 = time.perf_counter()
        rcode = lib.groth16_prove_r1cs_with_key(key.h, r.h, P(zm), C.c_uint(log_n), *[P(x) for x in kc], *[P(o) for o in outs])
        dt = time.perf_counter() - t0
        assert rcode == 0, rcode
        return dt, [o.copy() for o in outs]

    def run_piecewise():
        bufs = [x.copy() for x in rows]                                  # the witness map works in place: fresh a, b, c, made outside the timer
        t0 = time.perf_counter()
        rcode = lib.groth16_witness_map_bw6_761(P(bufs[0]), P(bufs[1]), P(bufs[2]), C.c_uint(log_n), *[P(x) for x in kc], C.c_int(1))
        assert rcode == 0, rcode
        rcode = lib.groth16_prove_with_key(key.h, P(zc), C.c_size_t(zc.shape[0]), C.c_size_t(case.n_vars - case.n_inputs), P(bufs[0]), C.c_size_t(n),
                                           *[P(o) for o in outs])
        dt = time.perf_counter() - t0
        assert rcode == 0, rcode
        return dt, [o.copy() for o in outs]

    (_, a), (_, b) = run_chained(), run_piecewise()                      # warm-up, and the two paths agree
    assert all(co.jac_to_affine(x, "761") == co.jac_to_affine(y, "761") for x, y in zip(a, b)), "chained proof != piecewise proof"
    tc, tp = [], []
    for _ in range(proofs):                                              # interleaved: both see the same machine state
        tc.append(run_chained()[0])
        tp.append(run_piecewise()[0])
    key.release()
    r.release()
    res["prove_r1cs_with_key_ms"] = {"median": statistics.median(tc) * 1e3, "min": min(tc) * 1e3, "max": max(tc) * 1e3, "runs": proofs}
    res["piecewise_ms"] = {"median": statistics.median(tp) * 1e3, "min": min(tp) * 1e3, "max": max(tp) * 1e3, "runs": proofs,
                           "what": "groth16_witness_map_bw6_761 (host a, b, c precomputed, not timed) + groth16_prove_with_key"}
    res["chained_over_piecewise"] = statistics.median(tc) / statistics.median(tp)
    res["chained_no_slower_within_3_percent"] = bool(res["chained_over_piecewise"] <= 1.03)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,22")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--proofs", type=int, default=11)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.proofs >= 10
    ffi.init(0)
    sizes = [int(x) for x in a.sizes.split(",") if x]
    res = {"copy_rate_GBps": copy_rate_gbs()}
    ub = ffi.ubench_fp()
    res["ubench_fq377_mul_G"] = ub["fq377_mul_G"]
    res["cases"], res["skew"] = [], {}
    for log_n in sizes:
        n = 1 << log_n
        m, n_vars = n - 20, (n * 3) // 5 + 3
        per = {}
        for make in (lambda: chain_case("bw6_761", n - 2), lambda: rc.random_r1cs("bw6_761", m, n_vars, 7, log_n, ffi.R1CS_CHUNK, ffi.R1CS_LONG),
                     lambda: even_case("bw6_761", m, n_vars, 7, log_n)):           # one case in memory at a time
            case = make()
            per[case.name.split("(")[0]] = d = measure(case, log_n, a.reps, res["copy_rate_GBps"], ub["fq377_mul_G"])
            del case
            res["cases"].append(d)
            print(json.dumps(d), file=sys.stderr, flush=True)
        res["skew"][str(log_n)] = {k: (per["random"][k]["kernel_ms"] / per["random"]["nnz"]) / (per["even"][k]["kernel_ms"] / per["even"]["nnz"])
                                   for k in ("rows", "columns")}
    n = 1 << sizes[0]
    d = measure(rc.random_r1cs("bls12_377", n - 20, (n * 3) // 5 + 3, 7, 9, ffi.R1CS_CHUNK, ffi.R1CS_LONG), sizes[0], a.reps, res["copy_rate_GBps"], None)
    res["cases"].append(d)
    res["chained"] = chained(sizes[0], a.proofs)
    js = json.dumps(res, indent=1)
    print(js)
    if a.out:
        with open(a.out, "w") as f:
            f.write(js + "\n")
    return 0 if res["chained"]["chained_no_slower_within_3_percent"] else 1


if __name__ == "__main__":
    sys.exit(main())
