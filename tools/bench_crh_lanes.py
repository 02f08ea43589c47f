"""Lanes per message of the composite hasher's CRH kernel (composite_crh_bls12_377; csrc/unit_hash.hip k_pedersen_crh, csrc/unit_hash_lanes.hip k_pedersen_crh_lanes,
the width rule crh_pick_lanes of csrc/pedersen.h).

  python tools/bench_crh_lanes.py [--runs 3] [--measured own.json] [--baseline parent.json [parent_again.json]] [--out profiles/bench_crh_lanes.json]

Shapes, random bytes: 1 x 14 200 B, 64 x 10 400 B, 143 x 14 200 B, 2 048 x 10 400 B (inner epoch encodings), 65 536 x 127 B, 65 537 x 12 B (the bulk
short-message calls), and 64 x 400 B and 64 x 100 B, where the device is empty and the messages short: the work term of the rule alone.  Per shape, in one process: every forced width 1 ... 256 and the rule (width 0), --runs calls after one warm-up each;
the time is the kernel's (celo_amd_hash_last_ms, HIP events around the launch), medians with spread, and every width's output is compared
with the first one's.

On a build without celo_amd_crh_set_lanes the widths are skipped and the one kernel there is timed: copy this file into a checkout of the
parent commit, run it there with --out parent.json in the same run, before this build's run and again after it, and hand the files to
--baseline (their samples are pooled) together with --measured, this build's own output of that run, which is then not measured again.
Those numbers, not width 1 of this build, are the `parent` entry of every shape and the numerator of `parent_over_rule`.  Same-run comparisons; nothing is asserted on a time."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: both must share one HIP runtime)
from celo_bls_snark_rs_amd import ffi  # noqa: E402

SHAPES = (("one_1x14200", 1, 14200), ("small_64x10400", 64, 10400), ("proof_143x14200", 143, 14200), ("sync_2048x10400", 2048, 10400),
          ("bulk_65536x127", 65536, 127), ("bulk_65537x12", 65537, 12), ("work_64x400", 64, 400), ("work_64x100", 64, 100))
WIDTHS = (1, 2, 4, 8, 16, 32, 64, 128, 256)


def spread(vals):
    return {"min": round(min(vals), 4), "median": round(statistics.median(vals), 4), "max": round(max(vals), 4)}


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def measure(runs, only=None):
    ffi.init(0)
    lib = ffi.lib()
    has_setter = hasattr(ffi, "crh_set_lanes")
    doc = {"device": torch.cuda.get_device_name(0), "runs": runs, "has_setter": has_setter, "shapes": {}}
    rng = np.random.default_rng(2026)

    def timed(data, off, n, out):
        ms = []
        for i in range(runs + 1):
            assert lib.composite_crh_bls12_377(p(data), p(off), C.c_size_t(n), p(out)) == 0
            if i:
                ms.append(ffi.hash_last_ms())
        return ms

    try:
        for name, n, size in SHAPES:
            if only and name not in only:
                continue
            data = rng.integers(0, 256, size=n * size, dtype=np.uint8)
            off = np.arange(n + 1, dtype=np.uint64) * size
            rec = {"messages": n, "bytes": size, "chunks": (size * 8 + 2) // 3}
            first = None
            if not has_setter:
                out = np.zeros((n, 48), dtype=np.uint8)
                rec["samples_ms"] = [round(x, 4) for x in timed(data, off, n, out)]
                rec["kernel_ms"] = spread(rec["samples_ms"])
            else:
                rec["widths"] = {}
                for L in WIDTHS + (0,):
                    ffi.crh_set_lanes(L)
                    out = np.zeros((n, 48), dtype=np.uint8)
                    ms = spread(timed(data, off, n, out))
                    if first is None:
                        first = out
                    assert np.array_equal(out, first), (name, L)
                    if L:
                        assert ffi.crh_last_lanes() == L
                        rec["widths"][str(L)] = ms
                    else:
                        rec["rule"] = {"lanes": ffi.crh_last_lanes(), "kernel_ms": ms}
                best = min(WIDTHS, key=lambda L: rec["widths"][str(L)]["median"])
                rec["best_width"] = best
                rec["rule_over_best"] = round(rec["rule"]["kernel_ms"]["median"] / rec["widths"][str(best)]["median"], 3)
            doc["shapes"][name] = rec
    finally:
        if has_setter:
            ffi.crh_set_lanes(0)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--baseline", nargs="+", default=[], help="the JSON files this tool wrote on the parent commit's build in the same run")
    ap.add_argument("--shapes", nargs="+", default=None, help="only these shapes (by name), e.g. to time the bulk shapes in a process that ran nothing else")
    ap.add_argument("--measured", default=None, help="this build's own output of the same run: attach the baseline to it and measure nothing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_crh_lanes.json"))
    a = ap.parse_args()
    base = []
    for path in a.baseline:
        with open(path) as f:
            base.append(json.load(f))
    if a.measured:
        with open(a.measured) as f:
            doc = json.load(f)
    else:
        doc = measure(a.runs, a.shapes)
    for name, rec in doc["shapes"].items():
        if base and "rule" in rec:
            samples = [x for b in base if name in b["shapes"] for x in b["shapes"][name]["samples_ms"]]
            rec["parent"] = {"kernel_ms": spread(samples), "samples_ms": samples}
            rec["rule_over_parent"] = round(rec["rule"]["kernel_ms"]["median"] / rec["parent"]["kernel_ms"]["median"], 3)
            rec["parent_over_rule"] = round(rec["parent"]["kernel_ms"]["median"] / rec["rule"]["kernel_ms"]["median"], 3)
    text = json.dumps(doc, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
