"""Same-run A/B of the two BW6-761 subgroup tests - [a]P + [b]phi(P) == O (csrc/wire761.h w761_in_subgroup_endo, hook 0) against the r P
ladder (w761_in_subgroup, hook 1) - and the throughput of the bulk point validator check_points_* for all four groups.

  python tools/bench_subgroup.py [--log-n 20] [--reps 3] [--out profiles/bench_subgroup.json]

n = 2^log_n subgroup points per group (k_i G from celo_amd_gen_points_*_dev).  Kernel time from HIP events (the entries' own "last call"
records), `reps` runs per setting after one warm-up, the hook alternating 0, 1, 0, 1 ... in one process:
  - check_points_bw6_761_*_dev at level 2 (the bare test is that minus level 1, which is measured too),
  - decompress_bw6_761_*_dev checked and decode_uncompressed_bw6_761_* checked,
  - the load of a serialized ProvingKey<BW6_761> with n points per query (the key of tools/bench_wire761.py),
  - check_points_* of all four groups at level 1 and level 2 (hook 0).
The yardstick is the ladder in the same run.  "keeps_default" applies the rule the decoders' default follows: the endomorphism form stays
the default only where its median beats the ladder's by more than the spread (max - min) of the ladder's own runs.  Prints one JSON document."""
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
from oracle import cpu_oracle as co  # noqa: E402
from celo_bls_snark_rs_amd import ffi  # noqa: E402
import bw6_serial as bs  # noqa: E402

# field products per point, counted (9 per XYZZ doubling, 10 per mixed addition): the ladder's 376 doublings and 134 additions, the
# endomorphism form's 189 and 73
COUNTED = {"ladder_products": 376 * 9 + 134 * 10, "endo_products": 189 * 9 + 73 * 10}


def ab(run, reps):
    """run() -> ms under hook 0 and hook 1 alternately: {"endo_ms": [...], "ladder_ms": [...], ...}"""
    out = {0: [], 1: []}
    for rep in range(reps + 1):
        for form in (0, 1):
            ffi.wire761_set_subgroup_test(form)
            ms = run()
            if rep:
                out[form].append(round(ms, 3))
    ffi.wire761_set_subgroup_test(0)
    e, l = statistics.median(out[0]), statistics.median(out[1])
    spread = max(out[1]) - min(out[1])
    return {"endo_ms": out[0], "ladder_ms": out[1], "ladder_spread_ms": round(spread, 3), "ratio_ladder_over_endo": round(l / e, 3),
            "keeps_default": bool(l - e > spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ffi.init(0)
    n = 1 << a.log_n
    res = {"n": n, "device": torch.cuda.get_device_name(0), "reps": a.reps, "counted": dict(COUNTED, ratio=round(COUNTED["ladder_products"] / COUNTED["endo_products"], 3)),
           "bw6_761": {}, "check_points": {}}
    gens = {"bw6_761_g1": co.pack_761([ecc.deser_point(ecc.E1_761, bs.reference_points()[0][1])])[0][0],
            "bw6_761_g2": co.pack_761([ecc.deser_point(ecc.E2_761, bs.reference_points()[1][1])])[0][0],
            "bls12_377_g1": co.pack_g1_377([ecc.G1_377])[0][0], "bls12_377_g2": co.pack_g2_377([ecc.G2_377])[0][0]}
    d_st = torch.empty(n, dtype=torch.uint8, device="cuda")
    enc = {}
    for group, words in ffi.CHECK_GROUPS.items():
        d_xy = torch.empty(n * words, dtype=torch.int64, device="cuda")
        ffi.gen_points_dev(group, d_xy.data_ptr(), n, 41 + len(group) + words, gens[group])
        torch.cuda.synchronize()

        def validate(level):
            first = ffi.check_points_dev(group, d_xy.data_ptr(), 0, n, d_st.data_ptr(), level)
            assert first == n, (group, level, first)
            return ffi.check_points_last_ms()
        lv = {}
        for level in (1, 2):
            validate(level)
            runs = [round(validate(level), 3) for _ in range(a.reps)]
            lv["level%d_ms" % level] = runs
            lv["level%d_points_per_s" % level] = round(n / (statistics.median(runs) * 1e-3))
        res["check_points"][group] = lv
        print(group, lv, flush=True)
        if not group.startswith("bw6"):
            continue
        g = group[-2:]
        curve = ecc.E1_761 if g == "g1" else ecc.E2_761
        r = {"check_points_level2": ab(lambda: validate(2), a.reps)}
        lvl1 = statistics.median(lv["level1_ms"])
        r["bare_test_ms"] = {k: round(statistics.median(r["check_points_level2"][k + "_ms"]) - lvl1, 3) for k in ("endo", "ladder")}
        r["bare_test_ratio"] = round(r["bare_test_ms"]["ladder"] / r["bare_test_ms"]["endo"], 3)
        pts = bs.rows_to_points(d_xy.cpu().numpy().view(np.uint64).reshape(n, 24))
        comp = b"".join(ecc.ser_point(curve, P) for P in pts)
        unc = b"".join(ecc.ser_point(curve, P, compressed=False) for P in pts)
        enc[g] = comp
        d_c = torch.from_numpy(np.frombuffer(comp, dtype=np.uint8).copy()).cuda()
        d_out = torch.empty(n * 24, dtype=torch.int64, device="cuda")

        def decompress():
            ffi.decompress_dev(group, d_c.data_ptr(), n, d_out.data_ptr(), d_st.data_ptr(), check_subgroup=True)
            assert not d_st.any().item()
            return ffi.wire761_last_timings()[0]

        def decode_uncompressed():
            _, st = ffi.decode_uncompressed(group, unc, check=True)
            assert not st.any()
            return ffi.wire761_last_timings()[0]
        r["decompress_checked"] = ab(decompress, a.reps)
        r["decode_uncompressed_checked"] = ab(decode_uncompressed, a.reps)
        for k in ("decompress_checked", "decode_uncompressed_checked"):
            r[k]["points_per_s_endo"] = round(n / (statistics.median(r[k]["endo_ms"]) * 1e-3))
            r[k]["points_per_s_ladder"] = round(n / (statistics.median(r[k]["ladder_ms"]) * 1e-3))
        res["bw6_761"][g] = r
        print(group, r, flush=True)
        del d_c, d_out, unc, pts
    # the key of tools/bench_wire761.py: n points per query behind the reference's VK, compressed
    vk = bs.reference_vk()
    g1c, g2c = enc["g1"], enc["g2"]
    vec = lambda b: (len(b) // 96).to_bytes(8, "little") + b  # noqa: E731
    key = vk + g1c[:96] + g1c[96:192] + vec(g1c) + vec(g1c) + vec(g2c) + vec(g1c) + vec(g1c)
    walls = {0: [], 1: []}

    def load():
        t = time.perf_counter()
        k = ffi.ProvingKey.from_serialized(key, 0)
        walls[ffi_form[0]].append(round((time.perf_counter() - t) * 1e3, 1))
        ms = ffi.wire761_last_timings()
        k.release()
        return ms[2]
    ffi_form = [0]
    out = {0: [], 1: []}
    for rep in range(a.reps):
        for form in (0, 1):
            ffi.wire761_set_subgroup_test(form)
            ffi_form[0] = form
            out[form].append(round(load(), 1))
    ffi.wire761_set_subgroup_test(0)
    spread = max(out[1]) - min(out[1])
    res["key_load"] = {"points_per_query": n, "decode_ms_endo": out[0], "decode_ms_ladder": out[1], "wall_ms_endo": walls[0], "wall_ms_ladder": walls[1],
                       "ratio_ladder_over_endo_decode": round(statistics.median(out[1]) / statistics.median(out[0]), 3),
                       "keeps_default": bool(statistics.median(out[1]) - statistics.median(out[0]) > spread)}
    res["decoders_keep_the_endomorphism_default"] = bool(res["key_load"]["keeps_default"] and all(
        res["bw6_761"][g][k]["keeps_default"] for g in ("g1", "g2") for k in ("decompress_checked", "decode_uncompressed_checked")))
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
