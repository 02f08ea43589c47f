"""Groth16 verification over BLS12-377 under a WIDE key (509 public inputs: the hash-helper proof of 143 epochs): every lane width of the
input sums against the rule, both modes, against the per-proof loop a caller had to write before.

  python tools/bench_groth16_verify_wide.py [--inputs 509] [--sizes 1,64,1024] [--ab-inputs 65] [--ab-sizes 4096,16384,65536] [--reps 5]
                                             [--epochs 143] [--out FILE]

One process, one constructed key (tests/groth16_verify377_cases.py; the proofs' points come from the library's fixed-base rows), all proofs
valid.  Reported:
  key_load_ms       wall time of groth16_vk_load_bls12_377_wide (the window tables of every input base), median of 3
  sizes[m].lanes    per forced width 1 .. 256 and for the rule (width 0): the `inputs` phase of the last record (HIP events: the lane kernel
                    and the normalisation of its sums) and the wall time of the mode-0 call, medians of `reps` rounds after a warm-up round,
                    the widths taking turns inside a round and the turn starting one slot later from round to round.  The rotation keeps
                    every slot behind the same neighbour: the rule's slot always follows the 256-lane call, behind which a call of a large
                    batch reads up to 1.7 x its time elsewhere - rule_over_same_width_forced shows it, and the rule's cost
                    is to be read from the forced slot of the width it chose; rule_over_best = the rule's inputs time over the best forced width's
  width_ab          the same width table, without the mode tables, for --inputs at --ab-sizes (3 rounds; proofs past the first 1 024 repeat
                    them) and for a key of --ab-inputs inputs at --sizes and the first of --ab-sizes: every row the rule's constants cite
  sizes[m].each / combined   the rule's call per mode with the phase times of the round nearest the median
  sizes[64].piecewise_loop   per proof one msm_bls12_377_g1 over the 510 gamma_abc rows and one four-pair pairing_product_is_one_bls12_377
  helper            one real helper proof of --epochs epochs (setup, groth16_hash_helper_prove_bls12_377, its 192 bytes) through
                    groth16_hash_helper_verify_bls12_377, accepted, and rejected with another chain's rows; 0 skips it
Writes profiles/bench_groth16_verify_wide.json unless --out names another file.  Exits non-zero unless mode 0 at m = 64 is cheaper per
proof than the loop; rule_over_best is reported and not gated."""
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
from tests import groth16_verify377_cases as gc  # noqa: E402
import groth16_setup_ref as gs  # noqa: E402
import r1cs_cases as rc  # noqa: E402

CURVE, P = "bls12_377", gs.FIELDS["bls12_377"]
KEY8 = np.arange(8, dtype=np.uint32) + 1
PHASES = ("decode", "inputs", "scale", "msm_and_alpha_wall", "pairing", "wall", "transfers")


def device_mul(gen, scalars, on_g2):
    xy, inf = ffi.fixed_base_mul(CURVE + ("_g2" if on_g2 else "_g1"), gen, co.ints_to_limbs([int(k) % gc.R for k in scalars], 4))
    xy[inf != 0] = 0
    return xy, inf


def piecewise(key, b):
    """what a caller had to write: per proof, the MSM over gamma_abc and the 4-pair product"""
    ng, nd, na = gc.neg_row(key.gamma), gc.neg_row(key.delta), gc.neg_row(key.alpha)
    one = co.ints_to_limbs([1], 4)
    ok = []
    for i in range(b.m):
        jac = ffi.msm(CURVE + "_g1", key.abc, None, np.concatenate([one, b.inputs[i]]))
        acc = co.pack_g1_377([co.jac_to_affine(jac, "g1_377")])[0][0]
        ok.append(ffi.pairing_product_is_one(np.stack([b.a[i], acc, b.c[i], na]), None, np.stack([b.b[i], ng, nd, key.beta]), None))
    return ok


def timed(fn):
    t0 = time.perf_counter()
    ok = fn()
    return (time.perf_counter() - t0) * 1e3, ok


def width_table(vk, b, m, reps):
    """every forced width and the rule (width 0) on the batch b, mode 0: medians over `reps` rounds after a warm-up round; the turn order is
    rotated by one slot per round"""
    widths = (0,) + ffi.G16_INPUT_LANES
    wall = {L: [] for L in widths}
    inp = {L: [] for L in widths}
    used = {}
    for r in range(reps + 1):                            # round 0 warms up
        for L in widths[r % len(widths):] + widths[:r % len(widths)]:
            ffi.groth16_set_input_lanes(L)
            dt, ok = timed(lambda: vk.verify(b.a, b.b, b.c, b.inputs, mode=0))
            assert ok.all(), (m, L)
            used[L] = ffi.groth16_inputs_last()[0]
            if r:
                wall[L].append(dt)
                inp[L].append(ffi.groth16_verify_last()[2][1])
    ffi.groth16_set_input_lanes(0)
    lanes = {str(L): {"lanes": used[L], "inputs_ms": round(statistics.median(inp[L]), 4), "inputs_ms_min": round(min(inp[L]), 4), "wall_ms": round(statistics.median(wall[L]), 3)}
             for L in widths}
    best = min(ffi.G16_INPUT_LANES, key=lambda L: statistics.median(inp[L]))
    return {"lanes": lanes, "rule_lanes": used[0], "best_forced_lanes": best, "rule_over_best": round(statistics.median(inp[0]) / statistics.median(inp[best]), 3),
            "rule_over_same_width_forced": round(statistics.median(inp[0]) / statistics.median(inp[used[0]]), 3)}


def helper(epochs):
    s = ffi.hash_to_bits_size(epochs)[1]
    log_n = s["log_n"]
    res = {"epochs": epochs, "n_inputs": s["n_inputs"] - 1, "log_n": log_n}
    r = ffi.hash_to_bits_r1cs_load(epochs)
    out = ffi.groth16_setup_r1cs(r, log_n, rc.mont([gs.root_of_unity(CURVE, log_n)], P)[0], rc.mont([0x1234567], P)[0], rc.mont([3, 5, 7, 11], P),
                                 gs.pack(CURVE, 1, [ecc.G1_377])[0][0], gs.pack(CURVE, 2, [ecc.G2_377])[0][0], want_rows=False, want_key=True)
    key, v = out["key"], out["vk"]
    k = gp.domain_constants(log_n, gs.root_of_unity(CURVE, log_n), gs.coset_generator(P), P)
    consts = {name: co.to_mont([x], P)[0] for name, x in k.items()}
    rows = np.random.default_rng(epochs).integers(0, 256, size=(epochs, 48), dtype=np.uint8)
    other = np.random.default_rng(epochs + 1).integers(0, 256, size=(epochs, 48), dtype=np.uint8)
    ser = ffi.groth16_serialize_proof(*ffi.hash_helper_prove(key, r, rows, 1, log_n, consts)[:3], curve=CURVE)
    load_ms, vk = timed(lambda: ffi.VerifyingKey(v["alpha_g1"], v["beta_g2"], v["gamma_g2"], v["delta_g2"], v["gamma_abc_g1"], curve=CURVE, wide=True))
    res["key_load_ms"] = round(load_ms, 3)
    walls = []
    for i in range(4):
        dt, ok = timed(lambda: ffi.hash_helper_verify(vk, rows, epochs, ser, bit_order=1, mode=0))
        assert ok.tolist() == [1], "the helper proof was not accepted"
        if i:
            walls.append(dt)
    res["hash_helper_verify_ms"] = {"median": round(statistics.median(walls), 3), "min": round(min(walls), 3), "runs": len(walls)}
    res["phase_ms"] = dict(zip(PHASES, [round(x, 3) for x in ffi.groth16_verify_last()[2][:7]]))
    res["lanes"], res["window_bits"] = ffi.groth16_inputs_last()[0], ffi.groth16_verify_last()[1]
    assert ffi.hash_helper_verify(vk, other, epochs, ser, bit_order=1, mode=0).tolist() == [0], "the proof was accepted for another chain's rows"
    res["accepted"], res["rejected_for_other_rows"] = True, True
    vk.release(); key.release(); r.release()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", type=int, default=509)
    ap.add_argument("--sizes", default="1,64,1024")
    ap.add_argument("--ab-inputs", type=int, default=65)
    ap.add_argument("--ab-sizes", default="4096,16384,65536")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=143)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_groth16_verify_wide.json"))
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    ab_sizes = [int(s) for s in args.ab_sizes.split(",")] if args.ab_sizes else []
    ffi.init(0)
    key = gc.Key(args.inputs, 0x6116)
    loads = []
    for _ in range(3):
        dt, vk = timed(lambda: ffi.VerifyingKey(key.alpha, key.beta, key.gamma, key.delta, key.abc, curve=CURVE, wide=True))
        loads.append(dt)
        vk.release()
    vk = ffi.VerifyingKey(key.alpha, key.beta, key.gamma, key.delta, key.abc, curve=CURVE, wide=True)
    rng = ecc.SplitMix64(1)
    allb = gc.Batch(key, [gc.valid_proof(key, rng) for _ in range(max(sizes))], mul=device_mul)
    doc = {"curve": CURVE, "device": torch.cuda.get_device_name(0), "reps": args.reps, "n_inputs": args.inputs, "key_load_ms": round(statistics.median(loads), 3),
           "sizes": {}}
    for m in sizes:
        b = gc.take(allb, range(m))
        row = width_table(vk, b, m, args.reps)
        modes = {"each": lambda: vk.verify(b.a, b.b, b.c, b.inputs, mode=0), "combined": lambda: vk.verify(b.a, b.b, b.c, b.inputs, mode=1, key=KEY8)}
        if m == 64:
            modes["piecewise_loop"] = lambda: np.array(piecewise(key, b), dtype=np.uint8)
        mw = {k: [] for k in modes}
        last = {k: [] for k in modes}
        for r in range(args.reps + 1):
            for name, fn in modes.items():
                dt, ok = timed(fn)
                assert ok.all(), (name, m)
                if r:
                    mw[name].append(dt)
                    last[name].append(ffi.groth16_verify_last() if name != "piecewise_loop" else None)
        for name in modes:
            med = statistics.median(mw[name])
            at = min(range(len(mw[name])), key=lambda i: abs(mw[name][i] - med))
            row[name] = {"wall_ms_median": round(med, 3), "wall_ms_min": round(min(mw[name]), 3), "per_proof_ms": round(med / m, 4)}
            if last[name][at] is not None:
                path, c, ms = last[name][at]
                row[name].update({"path": path, "window_bits": c, "phase_ms": dict(zip(PHASES, [round(x, 3) for x in ms[:7]]))})
        row["combined_over_each"] = round(row["combined"]["wall_ms_median"] / row["each"]["wall_ms_median"], 3)
        if m == 64:
            row["each_per_proof_below_piecewise"] = row["each"]["per_proof_ms"] < row["piecewise_loop"]["per_proof_ms"]
            row["piecewise_over_each"] = round(row["piecewise_loop"]["per_proof_ms"] / row["each"]["per_proof_ms"], 2)
        doc["sizes"][str(m)] = row
    # the rows the rule's constants cite beyond the mode tables: larger batches of the same key (the first max(sizes) proofs repeated), and a
    # key of few inputs
    doc["width_ab"] = {}
    pool = max(sizes)
    big = {}
    for m in ab_sizes:
        big[str(m)] = width_table(vk, gc.take(allb, [i % pool for i in range(m)]), m, 3)
    doc["width_ab"][str(args.inputs)] = big
    vk.release()
    if args.ab_inputs:
        key2 = gc.Key(args.ab_inputs, 0x6117)
        vk2 = ffi.VerifyingKey(key2.alpha, key2.beta, key2.gamma, key2.delta, key2.abc, curve=CURVE, wide=True)
        rng2 = ecc.SplitMix64(2)
        allb2 = gc.Batch(key2, [gc.valid_proof(key2, rng2) for _ in range(pool)], mul=device_mul)
        doc["width_ab"][str(args.ab_inputs)] = {str(m): width_table(vk2, gc.take(allb2, [i % pool for i in range(m)]), m, args.reps if m <= pool else 3)
                                                for m in sizes + ab_sizes[:1]}
        vk2.release()
    if args.epochs:
        doc["helper"] = helper(args.epochs)
    doc["note"] = ("inputs_ms: the `inputs` phase of the last record (HIP events around the input-sum kernel and the normalisation of its sums), median of the rounds "
                   "after one warm-up round, the widths interleaved and their order rotated by one slot per round; rule_over_same_width_forced: the rule's slot over the forced slot of the "
                   "width the rule chose (the same launch: 1.0 but for noise); wall_ms: host wall time of the whole mode-0 call; lanes '0' is the rule")
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    for m, row in doc["sizes"].items():
        if "piecewise_loop" in row and not row["each_per_proof_below_piecewise"]:
            sys.exit("each (%.3f ms per proof) is not below the piecewise loop (%.3f ms per proof) at m = %s"
                     % (row["each"]["per_proof_ms"], row["piecewise_loop"]["per_proof_ms"], m))


if __name__ == "__main__":
    main()
