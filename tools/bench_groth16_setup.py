"""Wall time of a BW6-761 Groth16 setup (groth16_setup_bw6_761, csrc/unit_setup.hip) and the fixed-base kernel's rate against the multiplier peak.

  python tools/bench_groth16_setup.py [--log-n 20] [--windows 6,8,10] [--out profiles/bench_groth16_setup.json]

A setup with n_vars = 2^log_n variables (2 of them inputs), n_h = 2^log_n - 1 and random QAP values (the device work does not depend on the
circuit): wall time and its breakdown (table build, Fr preparation, G1 rows, G2 rows, normalisation, key tables) from the library's own timers,
best of --reps after one warm-up.  The fixed-base kernel (k_fbm_rows<G_761>): rows/s, and its share of the multiplier roofline - the model
counts W windows x (1 - 2^-c) nonzero digits per row x 14 140 multiply-adds per mixed addition of the 28-limb field,
the peak is celo_amd_ubench_fp's Fq761 products/s x 1 540 multiply-adds, measured in the same process.  --windows: the same-box A/B of the
window width c on 2^log_n G1 rows (fixed_base_mul_bw6_761_g1).  The CPU comparison is an ESTIMATE: the host oracle's time per row on sampled
rows (one double-and-add scalar multiplication each, one thread) times the setup's row count.  Prints one JSON document."""
import argparse
import json
import os
import random
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

MADDS_PER_MIXED_ADD_761 = 14140
MADDS_PER_PRODUCT_761 = 1540         # 2 L^2 - L multiply-adds of one 28-limb Montgomery product (378 for L = 14)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--windows", default="6,8,10,12")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ffi.init(0)
    p = ecc.Q377
    n, n_in = 1 << a.log_n, 2
    rng = np.random.default_rng(1)

    def felts(k):
        x = rng.integers(0, 1 << 62, size=(k, 6), dtype=np.int64).astype(np.uint64)
        x[:, 5] &= np.uint64((1 << 56) - 1)
        return x
    qa, qb, qc = felts(n), felts(n), felts(n)
    zt, tau, tox = felts(1)[0], felts(1)[0], felts(4)
    G1, G2 = gs.generators("bw6_761")
    g1, g2 = co.pack_761([G1])[0][0], co.pack_761([G2])[0][0]
    res = {"curve": "bw6_761", "n_vars": n, "n_inputs": n_in, "n_h": n - 1}
    n1, n2 = 3 + n_in + 2 * n + (n - 1) + (n - n_in), 3 + n
    res["rows"] = {"g1": n1, "g2": n2}
    ffi.groth16_setup("bw6_761", qa[:1024], qb[:1024], qc[:1024], n_in, zt, tau, 1023, tox, g1, g2)        # warm-up (code objects, pools)
    best = None
    for _ in range(a.reps):
        t0 = time.perf_counter()
        out = ffi.groth16_setup("bw6_761", qa, qb, qc, n_in, zt, tau, n - 1, tox, g1, g2, want_vk=True, want_rows=True, want_key=True)
        wall = time.perf_counter() - t0
        t = ffi.setup_timings()
        out["key"].release()
        del out
        if best is None or t["wall"] < best["wall"]:
            best = dict(t, python_wall_s=wall)
    res["setup_ms"] = {k: round(v, 3) for k, v in best.items()}
    res["setup_ms"]["note"] = ("table / fr_prep / g1_rows / g2_rows / normalize: kernel time (HIP events); key_tables: wall time of the four fixed-base "
                               "MSM tables built from the device rows; wall: the whole call, transfers of the QAP in and of every row out included")
    peak = ffi.ubench_fp()
    peak_madds = peak["fq761_mul_G"] * 1e9 * MADDS_PER_PRODUCT_761
    rows_s = (n1 + n2) / (best["g1_rows"] + best["g2_rows"]) * 1e3
    c = 10                             # the library's default (unit_setup.hip FB_DEFAULT_C)
    W = -(-(377 + 1) // c)
    model = W * (1 - 2.0 ** -c) * MADDS_PER_MIXED_ADD_761
    res["fixed_base_kernel"] = {"window_bits": c, "windows": W, "rows_per_s": rows_s, "model_madds_per_row": model,
                                "achieved_madds_per_s": rows_s * model, "ubench_fq761_mul_G": peak["fq761_mul_G"], "peak_madds_per_s": peak_madds,
                                "roofline_share": rows_s * model / peak_madds}
    # same-box A/B of the window width on 2^log_n G1 rows
    ab = {}
    sc = co.ints_to_limbs([random.Random(3).randrange(p) for _ in range(1 << min(a.log_n, 18))], 6)
    sc = np.tile(sc, (n // sc.shape[0], 1))
    for cw in [int(x) for x in a.windows.split(",") if x]:
        ffi.set_fixed_base_window(cw)
        ffi.fixed_base_mul("bw6_761_g1", g1, sc[:1024])
        ts = []
        for _ in range(a.reps):
            ffi.fixed_base_mul("bw6_761_g1", g1, sc)
            ts.append(ffi.setup_timings())
        tb = min(ts, key=lambda t: t["g1_rows"])
        ab[str(cw)] = {"table_ms": round(tb["table"], 3), "rows_ms": round(tb["g1_rows"], 3), "normalize_ms": round(tb["normalize"], 3),
                       "rows_per_s": n / tb["g1_rows"] * 1e3}
    ffi.set_fixed_base_window(0)
    res["window_ab_g1_rows"] = ab
    # CPU estimate: the host oracle's scalar multiplication on sampled rows
    E = ecc.E1_761
    ks = [random.Random(4).randrange(p) for _ in range(16)]
    t0 = time.perf_counter()
    for k in ks:
        E.mul(G1, k)
    per_row = (time.perf_counter() - t0) / len(ks)
    res["cpu_estimate"] = {"python_oracle_s_per_row": per_row, "rows": n1 + n2, "estimated_s": per_row * (n1 + n2),
                           "note": "ESTIMATE, not a measured setup: one python double-and-add scalar multiplication per row, one thread, times the row count; "
                                   "ark's windowed fixed-base multiplication on many cores is faster than this by a large factor"}
    js = json.dumps(res, indent=1)
    print(js)
    if a.out:
        with open(a.out, "w") as f:
            f.write(js + "\n")


if __name__ == "__main__":
    main()
