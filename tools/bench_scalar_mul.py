"""Batched variable-base scalar multiplication (scalar_mul_batch_*, csrc/unit_varbase.hip) and batched signing (sign_batch_bls12_377).

  python tools/bench_scalar_mul.py [--sizes 16,20] [--runs 3] [--out profiles/bench_scalar_mul.json]

Per group and size: --runs runs after one warm-up, the kernel time split by the library's own timers (celo_amd_scalar_mul_last_ms: table build,
ladder, normalisation) with its spread, and the wall time of the host-pointer call.  The multiplier roofline is measured in the same process
(celo_amd_ubench_fp); the multiply-add count per row comes from the formulas that run (products_per_row below) and is written next to the result.
Same-run comparisons, none against a threshold fixed in advance:
  - the subgroup (GLV) entry against the plain entry on the same BLS12-377 G1 inputs;
  - the window width c over every width the setter accepts, per entry, at 2^16 rows;
  - fixed_base_mul_bls12_377_g1 on as many rows (one generator, no doublings);
  - sign_batch_bls12_377 at 2^16 direct messages, with the shares of the hash, the multiplication, the encoding and the rest (the hash rows
    crossing to the host and back, the host's packing), against a loop over Seam A's sign_message on one core.
Prints one JSON document."""
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
import torch  # noqa: E402,F401  (before the library: both must share one HIP runtime)
from oracle.py import ecc  # noqa: E402
from oracle import cpu_oracle as co  # noqa: E402
from celo_bls_snark_rs_amd import ffi  # noqa: E402
import groth16_setup_ref as gs  # noqa: E402

DEFAULT_C = {"bls12_377_g1": 4, "bls12_377_g2": 3, "bw6_761_g1": 3, "bw6_761_g2": 3}      # csrc/unit_varbase.hip vb_default_c
# products of one group operation of csrc/curve.h, a square counted as a product: xyzz_dbl 6 M + 3 S, xyzz_madd 8 M + 2 S
DBL, MADD = 9, 10
# multiply-adds of one product: 2 L^2 - L for the L-limb Montgomery product; an Fq2 product is four base products (fp2.h)
MADDS = {"bls12_377_g1": 378, "bls12_377_g2": 4 * 378, "bw6_761_g1": 1540, "bw6_761_g2": 1540}
PEAK_KEY = {"bls12_377_g1": "fq377_mul_G", "bls12_377_g2": "fq377_mul_G", "bw6_761_g1": "fq761_mul_G", "bw6_761_g2": "fq761_mul_G"}
PEAK_MADDS = {"fq377_mul_G": 378, "fq761_mul_G": 1540}


def windows(bits, c):
    return (bits + 1 + c - 1) // c


def products_per_row(bits, c, glv):
    """the field products one row costs, from the formulas of csrc/var_base.h (inversions, additions and the integer recoding not counted):
    table: 2 (from_ark) + (H - 1) mixed additions + 2 per entry for the running product + 7 per entry on the way back;
    ladder: c doublings per window below the top one + one mixed addition per nonzero digit ((1 - 2^-c) of them; the first lands on the
    identity and is free); the subgroup form has two digits per window of a 127-bit half and one more product (beta x) for the image;
    normalisation: 3 for the prefix / suffix products, 2 for the denominator (computed twice), 4 for the coordinates."""
    H = 1 << (c - 1)
    table = 2 + (H - 1) * (MADD + 2 + 7)
    nz = 1 - 2.0 ** -c
    if glv:
        W = windows(127, c)
        ladder = (W - 1) * c * DBL + 2 * W * nz * MADD - MADD + W * nz
    else:
        W = windows(bits, c)
        ladder = (W - 1) * c * DBL + W * nz * MADD - MADD
    return {"table": table, "ladder": ladder, "normalize": 9, "total": table + ladder + 9}


def uniform_scalars(r, n, rng, limbs):
    s = rng.integers(0, 1 << 63, size=(n, limbs), dtype=np.int64).astype(np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, limbs), dtype=np.int64).astype(np.uint64)
    top = r >> (64 * (limbs - 1))
    s[:, limbs - 1] %= np.uint64(top)                  # strictly below r's top limb: below r
    return s


def spread(vals):
    return {"min": round(min(vals), 4), "median": round(statistics.median(vals), 4), "max": round(max(vals), 4)}


def run_entry(name, subgroup, xy, sc, runs):
    ffi.scalar_mul_batch(name, xy[:256], None, sc[:256], subgroup=subgroup)       # warm-up (code objects)
    recs = []
    for _ in range(runs):
        t0 = time.perf_counter()
        ffi.scalar_mul_batch(name, xy, None, sc, subgroup=subgroup)
        wall = (time.perf_counter() - t0) * 1e3
        ms = ffi.scalar_mul_last_ms()
        recs.append(dict(ms, kernels=ms["table"] + ms["ladder"] + ms["normalize"], python_wall=wall))
    return {k: spread([r[k] for r in recs]) for k in recs[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,20")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--sign-log-n", type=int, default=16)
    ap.add_argument("--seam-a-messages", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ffi.init(0)
    sizes = [int(x) for x in a.sizes.split(",") if x]
    rng = np.random.default_rng(7)
    peak = ffi.ubench_fp()
    doc = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "default_window_bits": DEFAULT_C, "ubench_fp": peak,
           "model": {"products_per_doubling": DBL, "products_per_mixed_addition": MADD, "madds_per_product": MADDS,
                     "note": "a square counts as a product; inversions (one per row in the table kernel, one per 8 / 4 rows in the normaliser) are not counted"},
           "groups": {}, "window_ab_2p16": {}}
    inputs = {}
    for name in sorted(gs.GROUPS):
        _, curve, g, sw, aw = gs.GROUPS[name]
        r = gs.CURVES[curve][0]
        n = 1 << max(sizes)
        gen = gs.pack(curve, g, [gs.generators(curve)[g - 1]])[0][0]
        xy, inf = ffi.fixed_base_mul(name, gen, uniform_scalars(r, n, rng, sw))     # n points of the prime-order subgroup
        assert not inf.any()
        inputs[name] = (xy, uniform_scalars(r, n, rng, sw), r)
    entries = [(name, False) for name in sorted(gs.GROUPS)] + [("bls12_377_g1", True)]
    for name, subgroup in entries:
        xy, sc, r = inputs[name]
        label = name + ("_subgroup" if subgroup else "")
        print("[bench_scalar_mul] %s" % label, file=sys.stderr, flush=True)
        model = products_per_row(r.bit_length(), DEFAULT_C[name], subgroup)
        peak_madds = peak[PEAK_KEY[name]] * 1e9 * PEAK_MADDS[PEAK_KEY[name]]
        out = {"products_per_row": {k: round(v, 1) for k, v in model.items()}, "madds_per_row": round(model["total"] * MADDS[name]), "sizes": {}}
        for lg in sizes:
            n = 1 << lg
            t = run_entry(name, subgroup, xy[:n], sc[:n], a.runs)
            rows_s = n / (t["kernels"]["median"] * 1e-3)
            t.update({"rows_per_s_kernels": rows_s, "rows_per_s_wall": n / (t["wall"]["median"] * 1e-3),
                      "achieved_madds_per_s": rows_s * model["total"] * MADDS[name], "peak_madds_per_s": peak_madds,
                      "roofline_share": rows_s * model["total"] * MADDS[name] / peak_madds})
            out["sizes"]["2^%d" % lg] = t
        doc["groups"][label] = out
        # the window width, every accepted value, same inputs, 2^16 rows
        ab = {}
        n = 1 << 16
        for c in ffi.SCALAR_MUL_WINDOWS:
            ffi.set_scalar_mul_window(c)
            t = run_entry(name, subgroup, xy[:n], sc[:n], 2)
            ab[str(c)] = {"table_ms": t["table"]["min"], "ladder_ms": t["ladder"]["min"], "normalize_ms": t["normalize"]["min"], "kernels_ms": t["kernels"]["min"]}
        ffi.set_scalar_mul_window(0)
        ab["best"] = min(ffi.SCALAR_MUL_WINDOWS, key=lambda c: ab[str(c)]["kernels_ms"])
        doc["window_ab_2p16"][label] = ab
    g1 = doc["groups"]
    doc["subgroup_vs_plain_bls12_377_g1"] = {k: {"plain_kernels_ms": g1["bls12_377_g1"]["sizes"][k]["kernels"]["median"],
                                                  "subgroup_kernels_ms": g1["bls12_377_g1_subgroup"]["sizes"][k]["kernels"]["median"],
                                                  "speedup": g1["bls12_377_g1"]["sizes"][k]["kernels"]["median"] / g1["bls12_377_g1_subgroup"]["sizes"][k]["kernels"]["median"]}
                                              for k in g1["bls12_377_g1"]["sizes"]}
    # fixed_base_mul_bls12_377_g1 of the same run: one generator's table, no doublings
    fb = {}
    gen = co.pack_g1_377([ecc.G1_377])[0][0]
    for lg in sizes:
        n = 1 << lg
        sc = inputs["bls12_377_g1"][1][:n]
        ffi.fixed_base_mul("bls12_377_g1", gen, sc[:256])
        ts = []
        for _ in range(a.runs):
            ffi.fixed_base_mul("bls12_377_g1", gen, sc)
            t = ffi.setup_timings()
            ts.append(t["table"] + t["g1_rows"] + t["normalize"])
        fb["2^%d" % lg] = {"kernels_ms": spread(ts), "rows_per_s_kernels": n / (statistics.median(ts) * 1e-3)}
    doc["fixed_base_mul_bls12_377_g1"] = fb
    # sign_batch at 2^sign_log_n direct messages, one key per message
    print("[bench_scalar_mul] sign_batch", file=sys.stderr, flush=True)
    n = 1 << a.sign_log_n
    msgs = [b"block %08d of the benchmark chain" % i for i in range(n)]
    extras = [b"\x01\x02"] * n
    sk = inputs["bls12_377_g1"][1][:n]
    ffi.sign_batch(sk[:256], ffi.SIG_DOMAIN, msgs[:256], extras[:256], 0)
    recs = []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        sig, att = ffi.sign_batch(sk, ffi.SIG_DOMAIN, msgs, extras, 0)
        wall = (time.perf_counter() - t0) * 1e3
        ms = ffi.scalar_mul_last_ms()
        recs.append({"python_wall": wall, "call_wall": ms["wall"], "hash_kernels": ffi.hash_last_ms(), "multiply_kernels": ms["table"] + ms["ladder"] + ms["normalize"],
                     "encode_kernel": ffi.wire_encode_last_ms()})
    best = min(recs, key=lambda r: r["call_wall"])
    rest = best["call_wall"] - best["hash_kernels"] - best["multiply_kernels"] - best["encode_kernel"]
    doc["sign_batch"] = {"messages": n, "mode": "direct", "keys": "one per message", "ms": {k: spread([r[k] for r in recs]) for k in recs[0]},
                         "shares_of_the_best_call": {"hash": best["hash_kernels"] / best["call_wall"], "multiply": best["multiply_kernels"] / best["call_wall"],
                                                     "encode": best["encode_kernel"] / best["call_wall"], "rows_across_pcie_and_host": rest / best["call_wall"]},
                         "signatures_per_s": n / (best["call_wall"] * 1e-3),
                         "note": "rows_across_pcie_and_host: what the call spends outside its kernels - the hash rows to the host and back (96 B per message each "
                                 "way), the keys in, the signatures out, allocations and the hash unit's host staging"}
    # the parent's only way to sign: Seam A sign_message in a loop on one core
    lib = C.CDLL(ffi.LIB_PATH)
    for f in ("deserialize_private_key", "sign_message", "destroy_signature", "destroy_private_key"):
        getattr(lib, f).restype = C.c_bool
    m = min(a.seam_a_messages, n)
    keys = co.limbs_to_ints(sk[:m], 4)
    handles = []
    for k in keys:
        h = C.c_void_p()
        assert lib.deserialize_private_key(k.to_bytes(32, "little"), C.c_int(32), C.byref(h))
        handles.append(h)
    t0 = time.perf_counter()
    for i in range(m):
        s = C.c_void_p()
        assert lib.sign_message(handles[i], msgs[i], C.c_int(len(msgs[i])), extras[i], C.c_int(2), C.c_bool(False), C.c_bool(False), C.byref(s))
        lib.destroy_signature(s)
    per = (time.perf_counter() - t0) / m
    for h in handles:
        lib.destroy_private_key(h)
    doc["seam_a_sign_message_loop"] = {"messages": m, "s_per_signature": per, "signatures_per_s": 1 / per, "threads": 1}
    doc["sign_batch_vs_seam_a_loop"] = doc["sign_batch"]["signatures_per_s"] * per
    js = json.dumps(doc, indent=1)
    print(js)
    if a.out:
        with open(a.out, "w") as f:
            f.write(js + "\n")


if __name__ == "__main__":
    main()
