"""The HashToBits circuit on the device (csrc/unit_hashbits.hip): the three kernels, the assignment against its host twin, and the helper proof
in one call against the route without it.

  python tools/bench_hash_helper.py [--epochs 143,17] [--prove-epochs 143] [--runs 3] [--reps 5] [--out profiles/bench_hash_helper.json]

Every figure is taken --runs times (each the best of --reps after a warm-up where it is a kernel time) and reported with its spread.
  kernels      per --epochs entry: trace / expand / pack kernel times (HIP events, celo_amd_hash_helper_last) of hash_to_bits_assignment_bls12_377_dev;
               expand's achieved bytes/s (n_vars x 32 bytes written) beside the device-to-device copy rate of this run (1 GiB, the WRITE side
               alone: a kernel that only writes has that as its ceiling)
  assignment   at the first --epochs entry: the host twin's wall time, the copy of its z to the device, and the device assignment's wall time
  whole call   at --prove-epochs: groth16_hash_helper_prove_bls12_377 (rows in, proof and inputs out) against groth16_prove_r1cs_with_key handed a
               FINISHED host z (the time to make that z not counted: a floor for the route without this unit), interleaved, same key and circuit"""
import argparse
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
from oracle.py import ecc  # noqa: E402
from oracle.py import groth16_prover as gp  # noqa: E402
from oracle import cpu_oracle as co  # noqa: E402
from celo_bls_snark_rs_amd import ffi  # noqa: E402
import groth16_setup_ref as gs  # noqa: E402
import r1cs_cases as rc  # noqa: E402

CURVE, P = "bls12_377", gs.FIELDS["bls12_377"]


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": len(xs)}


def copy_write_rate_gbs():
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
    return n / (best * 1e-3) / 1e9


def rows_for(m):
    return np.random.default_rng(m).integers(0, 256, size=(m, 48), dtype=np.uint8)


def kernels(m, runs, reps, copy_gbs):
    s = ffi.hash_to_bits_size(m)[1]
    d_rows = torch.from_numpy(rows_for(m)).cuda()
    d_z = torch.empty(s["n_vars"] * 4, dtype=torch.int64, device="cuda")
    per = {"trace": [], "expand": [], "pack": []}
    for _ in range(runs):
        best = {}
        for i in range(reps + 1):                     # the first is the warm-up
            ffi.hash_to_bits_assignment_dev(d_rows.data_ptr(), m, 1, d_z.data_ptr())
            t = ffi.hash_helper_last()
            if i:
                for k in per:
                    best[k] = min(best.get(k, t[k]), t[k])
        for k in per:
            per[k].append(best[k])
    out = {"epochs": m, "n_vars": s["n_vars"], "z_bytes": s["n_vars"] * 32, "log_n": s["log_n"]}
    for k in per:
        out[k + "_ms"] = spread(per[k])
    gbs = [s["n_vars"] * 32 / (t * 1e-3) / 1e9 for t in per["expand"]]
    out["expand_GBps"] = spread(gbs)
    out["copy_write_GBps"] = copy_gbs
    out["expand_over_copy"] = statistics.median(gbs) / copy_gbs
    return out


def assignment(m, runs):
    rows = rows_for(m)
    host, up, dev = [], [], []
    d_rows = torch.from_numpy(rows).cuda()
    s = ffi.hash_to_bits_size(m)[1]
    d_z = torch.empty(s["n_vars"] * 4, dtype=torch.int64, device="cuda")
    ffi.hash_to_bits_assignment_dev(d_rows.data_ptr(), m, 1, d_z.data_ptr())
    for _ in range(runs):
        t0 = time.perf_counter(); z = ffi.hash_to_bits_assignment(rows, 1, host=True); host.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter(); d = torch.from_numpy(z.view(np.int64)).cuda(); torch.cuda.synchronize(); up.append((time.perf_counter() - t0) * 1e3)
        del d
        t0 = time.perf_counter(); ffi.hash_to_bits_assignment_dev(d_rows.data_ptr(), m, 1, d_z.data_ptr()); dev.append((time.perf_counter() - t0) * 1e3)
    assert np.array_equal(d_z.cpu().numpy().view(np.uint64).reshape(-1, 4), z), "device assignment != host twin"
    return {"epochs": m, "host_twin_ms": spread(host), "copy_of_z_to_device_ms": spread(up), "device_assignment_wall_ms": spread(dev)}


def whole_call(m, runs):
    s = ffi.hash_to_bits_size(m)[1]
    log_n = s["log_n"]
    res = {"epochs": m, "log_n": log_n, "n_vars": s["n_vars"], "n_constraints": s["n_constraints"]}
    t0 = time.perf_counter(); r = ffi.hash_to_bits_r1cs_load(m); res["r1cs_load_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    out = ffi.groth16_setup_r1cs(r, log_n, rc.mont([gs.root_of_unity(CURVE, log_n)], P)[0], rc.mont([0x1234567], P)[0], rc.mont([3, 5, 7, 11], P),
                                 gs.pack(CURVE, 1, [ecc.G1_377])[0][0], gs.pack(CURVE, 2, [ecc.G2_377])[0][0], want_vk=False, want_rows=False, want_key=True)
    res["setup_r1cs_s"] = time.perf_counter() - t0
    key = out["key"]
    k = gp.domain_constants(log_n, gs.root_of_unity(CURVE, log_n), gs.coset_generator(P), P)
    consts = {name: co.to_mont([v], P)[0] for name, v in k.items()}
    rows = rows_for(m)
    z = ffi.hash_to_bits_assignment(rows, 1, host=True)                    # made before, NOT timed
    new, old, split = [], [], []
    a = ffi.hash_helper_prove(key, r, rows, 1, log_n, consts)[:3]          # warm-up, and the two routes agree
    b = key.prove_r1cs(r, z, log_n, consts)
    names = ("g1_377", "g2_377", "g1_377")
    assert all(co.jac_to_affine(x, n) == co.jac_to_affine(y, n) for x, y, n in zip(a, b, names)), "helper proof != proof from the host z"
    for _ in range(runs):                                                  # interleaved: both see the same machine state
        t0 = time.perf_counter(); ffi.hash_helper_prove(key, r, rows, 1, log_n, consts); new.append((time.perf_counter() - t0) * 1e3)
        split.append(ffi.hash_helper_last())
        t0 = time.perf_counter(); key.prove_r1cs(r, z, log_n, consts); old.append((time.perf_counter() - t0) * 1e3)
    key.release()
    r.release()
    res["hash_helper_prove_ms"] = spread(new)
    res["prove_r1cs_with_key_from_host_z_ms"] = dict(spread(old), what="groth16_prove_r1cs_with_key on a finished host z; making z is not counted")
    res["split_ms"] = {kk: spread([t[kk] for t in split]) for kk in split[0]}
    res["new_over_old"] = statistics.median(new) / statistics.median(old)
    res["slower_by_more_than_the_spread"] = bool(statistics.median(new) - statistics.median(old) > max(max(new) - min(new), max(old) - min(old)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", default="143,17")
    ap.add_argument("--prove-epochs", type=int, default=143)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ffi.init(0)
    ms = [int(x) for x in a.epochs.split(",") if x]
    res = {"copy_write_GBps": copy_write_rate_gbs()}
    res["kernels"] = [kernels(m, a.runs, a.reps, res["copy_write_GBps"]) for m in ms]
    print(json.dumps(res["kernels"]), file=sys.stderr, flush=True)
    res["assignment"] = assignment(ms[0], a.runs)
    print(json.dumps(res["assignment"]), file=sys.stderr, flush=True)
    if a.prove_epochs:
        res["whole_call"] = whole_call(a.prove_epochs, a.runs)
    js = json.dumps(res, indent=1)
    print(js)
    if a.out:
        with open(a.out, "w") as f:
            f.write(js + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
