"""Key de-duplication (decompress_bls12_377_g2_dedup_dev, csrc/unit_dedup.hip) against the plain decoder in the same process on the same keys.

  python tools/bench_key_dedup.py [--runs 3] [--out profiles/bench_key_dedup.json] [--sweep-max-log 22] [--skip-big]

Shapes (G2 keys, device resident, subgroup check on; valid keys are made on the device by fixed_base_mul + compress):
  epoch          4 926 300 keys from a pool of 300      the shape of tools/bench_epoch_inputs.py (16 421 x 2 x 150)
  transitions    225 280 keys from a pool of 220        the shape of tools/bench_transitions.py
  all_distinct   2^20 keys, all distinct                the worst case for overhead
  all_equal      2^20 keys, all equal                   the worst case for contention: every lane on one slot's two atomics
  sweep          2^6 .. 2^sweep-max-log keys, all distinct: the rule N0 of csrc/dedup.h key_dedup_pick - the smallest power of two from which
                 the de-duplicating call's kernel time (median) stays within the plain call's own max over the runs; 0 if there is none
  crafted        2^16 .. 2^18 distinct strings that share ONE home slot (tests/dedup_ref.py solves the mix for them), against as many random
                 strings: that the probe cap holds the time down
Per shape: --runs runs after one warm-up; kernel time per stage (HIP events, celo_amd_key_dedup_last) and of the plain decoder
(celo_amd_decompress_last_ms) with min / median / max; the wall time of both calls, whose difference from the kernel time holds the 8-byte
round trip that sizes the decoder's launch.  The outputs of both calls are compared whole.  Prints one JSON document."""
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
import dedup_ref as R  # noqa: E402

STAGES = ("table", "gather", "decode", "scatter")


def spread(vals):
    return {"min": round(min(vals), 4), "median": round(statistics.median(vals), 4), "max": round(max(vals), 4)}


def valid_keys(n, start=3):
    """n distinct valid compressed G2 keys, made on the device in pieces of 2^20"""
    gen = co.pack_g2_377([ecc.G2_377])[0][0]
    out = []
    for lo in range(0, n, 1 << 20):
        k = np.arange(lo, min(n, lo + (1 << 20)), dtype=np.uint64) + np.uint64(start)
        sc = np.zeros((len(k), 4), dtype=np.uint64)
        sc[:, 0] = k
        rows, inf = ffi.fixed_base_mul("bls12_377_g2", gen, sc)
        enc, st = ffi.encode_points("g2", rows, inf)
        assert not st.any()
        out.append(enc)
    return np.concatenate(out)


def measure(keys, runs, compare=True):
    """keys: (n, 96) uint8 on the host.  Both decoders on the same device buffer."""
    n = len(keys)
    d_in = torch.from_numpy(np.ascontiguousarray(keys).reshape(-1)).cuda()
    d_xy = torch.zeros(n * 24, dtype=torch.int64, device="cuda")
    d_st = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_xy2 = torch.zeros(n * 24, dtype=torch.int64, device="cuda")
    d_st2 = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    plain, plain_wall, dd, dd_wall, decoded = [], [], [], [], 0
    for r in range(runs + 1):                                          # the first is the warm-up
        t0 = time.perf_counter()
        ffi.decompress_dev("g2", d_in.data_ptr(), n, d_xy.data_ptr(), d_st.data_ptr())
        t1 = time.perf_counter()
        pm = ffi.decompress_last_ms()
        t2 = time.perf_counter()
        decoded = ffi.decompress_dedup_dev("g2", d_in.data_ptr(), n, d_xy2.data_ptr(), d_st2.data_ptr())
        t3 = time.perf_counter()
        if r:
            plain.append(pm); plain_wall.append((t1 - t0) * 1e3)
            dd.append(ffi.key_dedup_last()[2]); dd_wall.append((t3 - t2) * 1e3)
    if compare:
        assert torch.equal(d_xy, d_xy2) and torch.equal(d_st, d_st2), "the de-duplicating decoder differs from the plain one"
    total = [sum(x) for x in dd]
    out = {"keys": n, "decoded": decoded, "plain_kernel_ms": spread(plain), "plain_wall_ms": spread(plain_wall), "dedup_kernel_ms": spread(total),
           "dedup_wall_ms": spread(dd_wall), "dedup_stage_ms": {s: spread([x[i] for x in dd]) for i, s in enumerate(STAGES)},
           "dedup_wall_minus_kernel_ms": round(statistics.median(dd_wall) - statistics.median(total), 4),
           "plain_wall_minus_kernel_ms": round(statistics.median(plain_wall) - statistics.median(plain), 4),
           "plain_over_dedup_kernel": round(statistics.median(plain) / statistics.median(total), 3)}
    return out


def dump(doc, path):
    js = json.dumps(doc, indent=1)
    if path:
        with open(path, "w") as f:
            f.write(js + "\n")
    return js


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sweep-max-log", type=int, default=22)
    ap.add_argument("--skip-big", action="store_true", help="leave out the 4.93 M key shape")
    a = ap.parse_args()
    ffi.init(0)
    doc = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "settings": dict(zip(("on", "slack_log", "max_probes"), ffi.key_dedup_get())),
           "timer": "kernel: HIP events on the call's stream (celo_amd_key_dedup_last, celo_amd_decompress_last_ms); wall: around the _dev wrapper, "
                    "which returns after the stream has drained", "shapes": {}}
    note = lambda s: print("[bench_key_dedup] %s" % s, file=sys.stderr, flush=True)
    distinct = valid_keys(1 << max(20, a.sweep_max_log))
    shapes = [("transitions", distinct[np.arange(225280) % 220]), ("all_distinct", distinct[:1 << 20]), ("all_equal", distinct[np.zeros(1 << 20, dtype=np.int64)])]
    if not a.skip_big:
        shapes.append(("epoch", distinct[np.arange(16421 * 2 * 150) % 300]))
    for label, keys in shapes:
        note(label)
        doc["shapes"][label] = measure(keys, a.runs)
        dump(doc, a.out)
    # the rule: all distinct, where the table can only lose
    sweep, n0 = {}, 0
    for lg in range(6, a.sweep_max_log + 1):
        note("sweep 2^%d" % lg)
        rec = measure(distinct[:1 << lg], a.runs)
        rec["inside_plain_spread"] = rec["dedup_kernel_ms"]["median"] <= rec["plain_kernel_ms"]["max"]
        sweep["2^%d" % lg] = rec
        n0 = (n0 or (1 << lg)) if rec["inside_plain_spread"] else 0
    doc["sweep_all_distinct"] = sweep
    doc["N0_by_this_run"] = n0
    doc["N0_rule"] = "the smallest power of two from which, at every larger size of the sweep, the de-duplicating call's median kernel time is at most the plain call's max; 0: none"
    doc["N0_built_in"] = R.N0
    dump(doc, a.out)
    # crafted: one home slot for every key
    crafted = {}
    for lg in (16, 17, 18):
        note("crafted 2^%d" % lg)
        n = 1 << lg
        crowd = R.same_home(n, R.slots(n), 96, seed=lg)
        rnd = R.random_keys(n, 96, seed=100 + lg)
        crafted["2^%d" % lg] = {"one_home_slot": measure(crowd, a.runs), "random_strings": measure(rnd, a.runs),
                                "note": "strings, not keys: most do not decode, so the decode stage is short in both rows; compare the table stage"}
    doc["crafted"] = crafted
    print(dump(doc, a.out))


if __name__ == "__main__":
    main()
