"""Batch Groth16 verification over BW6-761 or BLS12-377 (csrc/groth16_verify_unit.h): each against combined against the per-proof loop.

  python tools/bench_groth16_verify.py [--curve bw6_761|bls12_377] [--sizes 64,1024,16421] [--reps 5] [--out FILE]

One process, one constructed key with two public inputs (tests/groth16_verify_cases.py, tests/groth16_verify377_cases.py; the proofs'
points come from the library's fixed-base rows), all proofs valid.  Per size m, after a warm-up round, `reps` rounds with the modes
interleaved (each, combined, serialized each; at m = 64 also the piecewise loop: one msm_<curve>_g1 and one pairing_product_is_one per
proof, the only way before these entry points existed).  --curve bls12_377 writes profiles/bench_groth16_verify_377.json unless --out
names another file, and leaves out the multiply-add model of k_g16_inputs, which is BW6-761's.  Reported: the median wall time per mode, the per-proof time, the HIP-event phase times of the `last` record of the
median round, combined / each, the decode share of the serialized entry, and the rate of k_g16_inputs against the celo_amd_ubench_fp
peak of the same run under DESIGN 6f's model (windows x (1 - 2^-c) digits x 14 140 multiply-adds per mixed addition; peak = Fq761
products/s x 1 540).  Prints one JSON document."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: both must share one HIP runtime)
from oracle.py import ecc  # noqa: E402
from oracle import cpu_oracle as co  # noqa: E402
from celo_bls_snark_rs_amd import ffi  # noqa: E402
from tests import groth16_verify_cases as gc761  # noqa: E402
from tests import groth16_verify377_cases as gc377  # noqa: E402

KEY8 = np.arange(8, dtype=np.uint32) + 1
gc = gc761                                   # the case module of the curve under test (main() sets it)
CURVE = "bw6_761"
N64 = {"bw6_761": 6, "bls12_377": 4}


def device_mul(gen, scalars, on_g2):
    xy, inf = ffi.fixed_base_mul(CURVE + ("_g2" if on_g2 else "_g1"), gen, co.ints_to_limbs([int(k) % gc.R for k in scalars], N64[CURVE]))
    xy[inf != 0] = 0
    return xy, inf


def piecewise(key, b):
    """what a caller did before: per proof, the 3-term input MSM and the 4-pair product"""
    ng, nd, na = gc.neg_row(key.gamma), gc.neg_row(key.delta), gc.neg_row(key.alpha)
    one = co.ints_to_limbs([1], N64[CURVE])
    ok = []
    for i in range(b.m):
        jac = ffi.msm(CURVE + "_g1", key.abc, None, np.concatenate([one, b.inputs[i]]))
        if CURVE == "bw6_761":
            acc = co.pack_761([co.jac_to_affine(jac, "761")])[0][0]      # (affine on the host, as Seam A's verify)
        else:
            acc = co.pack_g1_377([co.jac_to_affine(jac, "g1_377")])[0][0]
        g1 = np.stack([b.a[i], acc, b.c[i], na])
        g2 = np.stack([b.b[i], ng, nd, key.beta])
        ok.append((ffi.pairing_product_is_one_bw6 if CURVE == "bw6_761" else ffi.pairing_product_is_one)(g1, None, g2, None))
    return ok


def main():
    global gc, CURVE
    ap = argparse.ArgumentParser()
    ap.add_argument("--curve", default="bw6_761", choices=["bw6_761", "bls12_377"])
    ap.add_argument("--sizes", default="64,1024,16421")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    CURVE = args.curve
    gc = gc761 if CURVE == "bw6_761" else gc377
    if CURVE == "bls12_377" and args.out is None:
        args.out = os.path.join(ROOT, "profiles", "bench_groth16_verify_377.json")
    ffi.init(0)
    peak = ffi.ubench_fp()
    key = gc.Key(2, 0x6116)
    vk = ffi.VerifyingKey(key.alpha, key.beta, key.gamma, key.delta, key.abc, curve=CURVE)
    rng = ecc.SplitMix64(1)
    allb = gc.Batch(key, [gc.valid_proof(key, rng) for _ in range(max(sizes))], mul=device_mul)
    doc = {"curve": CURVE, "device": torch.cuda.get_device_name(0), "reps": args.reps, "n_inputs": 2, "ubench_fp": peak, "sizes": {}}
    for m in sizes:
        b = gc.take(allb, range(m))
        ser = b.serialize() if m <= 1024 else None
        modes = {"each": lambda: vk.verify(b.a, b.b, b.c, b.inputs, mode=0), "combined": lambda: vk.verify(b.a, b.b, b.c, b.inputs, mode=1, key=KEY8)}
        if ser is not None:
            modes["serialized_each"] = lambda: vk.verify_serialized(ser, b.inputs, mode=0)
        if m == 64:
            modes["piecewise_loop"] = lambda: np.array(piecewise(key, b), dtype=np.uint8)
        wall = {k: [] for k in modes}
        last = {k: [] for k in modes}
        for r in range(args.reps + 1):                  # round 0 warms up; the modes take turns inside a round
            for name, fn in modes.items():
                t0 = time.perf_counter()
                ok = fn()
                dt = (time.perf_counter() - t0) * 1e3
                assert ok.all(), (name, m)
                if r:
                    wall[name].append(dt)
                    last[name].append(ffi.groth16_verify_last() if name != "piecewise_loop" else None)
        row = {}
        for name in modes:
            med = statistics.median(wall[name])
            at = min(range(len(wall[name])), key=lambda i: abs(wall[name][i] - med))
            row[name] = {"wall_ms_median": round(med, 3), "wall_ms_min": round(min(wall[name]), 3), "per_proof_ms": round(med / m, 4)}
            if last[name][at] is not None:
                path, c, ms = last[name][at]
                row[name].update({"path": path, "window_bits": c, "phase_ms": dict(zip(("decode", "inputs", "scale", "msm_and_alpha_wall", "pairing", "wall", "transfers"),
                                                                                      [round(x, 3) for x in ms[:7]]))})
        row["combined_over_each"] = round(row["combined"]["wall_ms_median"] / row["each"]["wall_ms_median"], 3)
        if CURVE == "bw6_761":
            c = row["each"]["window_bits"]
            windows = (377 + 1 + c - 1) // c
            madds = m * 2 * windows * (1 - 2.0 ** -c) * 14140
            in_ms = row["each"]["phase_ms"]["inputs"]
            row["inputs_kernel_share_of_peak"] = round(madds / (in_ms * 1e-3) / (peak["fq761_mul_G"] * 1e9 * 1540), 4) if in_ms > 0 else None
        if "serialized_each" in row:
            row["serialized_decode_share"] = round(row["serialized_each"]["phase_ms"]["decode"] / row["serialized_each"]["wall_ms_median"], 3)
        if m == 64:
            row["each_per_proof_below_piecewise"] = row["each"]["per_proof_ms"] < row["piecewise_loop"]["per_proof_ms"]
            row["piecewise_over_each"] = round(row["piecewise_loop"]["per_proof_ms"] / row["each"]["per_proof_ms"], 2)
        doc["sizes"][str(m)] = row
    vk.release()
    doc["note"] = ("wall_ms: host wall time of the whole call, median of the rounds after one warm-up round, modes interleaved; phase_ms: the last record of the "
                   "round nearest the median (HIP events; msm_and_alpha_wall and wall are host clocks); inputs includes the normalisation of the sums; "
                   "inputs_kernel_share_of_peak counts both kernels' time against the multiply-add model, so it understates the lane kernel")
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    # what must hold: the loop pays a latency path per proof, so a batched call that is not cheaper per proof has lost its chaining
    for m, row in doc["sizes"].items():
        if "piecewise_loop" in row and not row["each_per_proof_below_piecewise"]:
            sys.exit("each (%.3f ms per proof) is not below the piecewise loop (%.3f ms per proof) at m = %s"
                     % (row["each"]["per_proof_ms"], row["piecewise_loop"]["per_proof_ms"], m))


if __name__ == "__main__":
    main()
