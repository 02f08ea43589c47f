"""Masked segmented point sums (aggregate_by_bitmap_*, csrc/unit_seals.hip): the aggregated key of every seal of a batch from its bitmap.

  python tools/bench_seals.py [--runs 3] [--out profiles/bench_seals.json]

Shapes: 17 280 seals over one shared set of 110 keys (the blocks of one epoch; seeded bitmaps of 2/3 + 1 .. all signers), 4 096 seals with
per-seal sets of 256 keys, 64 seals over a shared set of 110.  Per shape, in one process: the sums at every lane width the hook accepts and
by rule, with the complement by rule, never and always (shared sets); --runs runs after one warm-up, kernel time from the library's HIP-event
timer (celo_amd_seals_last) with its spread, and the wall time of the host-pointer call.  Same-run comparisons, none against a threshold fixed in
advance: msm_batch_bls12_377_g2_subgroup with 0 / 1 scalars + normalize on the same inputs (what a caller could do before), and BLS12-377 G1 rows
(Signature::aggregate over a bitmap) at the epoch shape.
Then verify_aggregated_seals_bls12_377 on the same seals (signed in the run by sign_batch_bls12_377 under the summed keys): both modes with
the stage split of celo_amd_seals_last, against what a caller could chain before - msm_batch with 0 / 1 scalars + normalize + hash_to_g1_direct +
decompress + pairing_product_is_one_batch - and, on the 64 seals, a loop of Seam A aggregate_public_keys + verify_signature.
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
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before the library: both must share one HIP runtime)
from oracle.py import ecc  # noqa: E402
from oracle import cpu_oracle as co  # noqa: E402
from celo_bls_snark_rs_amd import ffi  # noqa: E402


def spread(vals):
    return {"min": round(min(vals), 4), "median": round(statistics.median(vals), 4), "max": round(max(vals), 4)}


def uniform_scalars(n, rng):
    s = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.int64).astype(np.uint64)
    s[:, 3] %= np.uint64(ecc.R377 >> 192)               # strictly below r's top limb: below r
    return s


def epoch_bitmaps(m, n, rng):
    """signer counts uniform in 2/3 n + 1 .. n, the absent validators at seeded places"""
    bits = np.ones((m, n), dtype=np.uint8)
    lo = 2 * n // 3 + 1
    for i, k in enumerate(rng.integers(lo, n + 1, size=m)):
        bits[i, rng.permutation(n)[:n - int(k)]] = 0
    return bits


def run_sums(group, xy, offsets, bits, runs):
    ffi.aggregate_by_bitmap(group, xy, None, offsets, bits)                      # warm-up (code objects, first allocations)
    recs = []
    for _ in range(runs):
        t0 = time.perf_counter()
        ffi.aggregate_by_bitmap(group, xy, None, offsets, bits)
        wall = (time.perf_counter() - t0) * 1e3
        rec = ffi.seals_last()
        recs.append({"kernels": rec["ms"]["sums"], "call_wall": rec["ms"]["wall"], "python_wall": wall, "lanes": rec["lanes"]})
    out = {k: spread([r[k] for r in recs]) for k in ("kernels", "call_wall", "python_wall")}
    out["lanes"] = recs[0]["lanes"]
    return out


def sweep(group, xy, offsets, bits, shared, runs):
    out = {}
    for complement in ((-1, 0, 1) if shared else (-1,)):
        ffi.set_aggregate_complement(complement)
        per = {}
        for lanes in (0,) + ffi.AGGREGATE_LANES:
            ffi.set_aggregate_lanes(lanes)
            per["rule" if lanes == 0 else str(lanes)] = run_sums(group, xy, offsets, bits, runs)
        per["best_width"] = min(ffi.AGGREGATE_LANES, key=lambda L: per[str(L)]["kernels"]["median"])
        per["rule_over_best"] = per["rule"]["kernels"]["median"] / per[str(per["best_width"])]["kernels"]["median"]
        out[{-1: "complement_by_rule", 0: "complement_never", 1: "complement_always"}[complement]] = per
    ffi.set_aggregate_lanes(0)
    ffi.set_aggregate_complement(-1)
    return out


def msm_baseline(xy, offsets, bits, shared, runs):
    """the same sums through msm_batch_bls12_377_g2_subgroup with 0 / 1 scalars and normalize_bls12_377_g2 (host pointers, as our call)"""
    if shared:
        n = int(offsets[1] - offsets[0])
        m = bits.shape[0]
        bases = np.tile(xy[:n], (m, 1))
        off = (np.arange(m + 1, dtype=np.uint64) * n).astype(np.uint32)
    else:
        bases, off, m = xy, offsets, offsets.shape[0] - 1
    sc = np.zeros((bases.shape[0], 4), dtype=np.uint64)
    sc[:, 0] = (bits.reshape(-1) != 0)
    walls = []
    for r in range(runs + 1):
        t0 = time.perf_counter()
        rows, inf = ffi.normalize("g2", ffi.msm_batch("bls12_377_g2", bases, None, sc, off, subgroup=True))
        if r:
            walls.append((time.perf_counter() - t0) * 1e3)
    return ({"python_wall": spread(walls)} if walls else None), rows, inf


NEG_G2 = co.pack_g2_377([ecc.E2_377.neg(ecc.G2_377)])[0][0]


def run_verify(xy, offsets, bits, msgs, sigs, mode, runs):
    recs = []
    for r in range(runs + 1):                                        # the first is the warm-up
        t0 = time.perf_counter()
        ok, st = ffi.verify_aggregated_seals(xy, None, offsets, bits, None, ffi.SIG_DOMAIN, msgs, None, sigs, NEG_G2, mode=mode)
        wall = (time.perf_counter() - t0) * 1e3
        assert ok.all() and not st.any()
        rec = ffi.seals_last()
        if r:
            recs.append(dict(rec["ms"], python_wall=wall, path=rec["path"], lanes=rec["lanes"]))
    out = {k: spread([x[k] for x in recs]) for k in recs[0] if k not in ("path", "lanes")}
    out.update(path=recs[0]["path"], lanes=recs[0]["lanes"])
    return out


def chained_before(xy, offsets, bits, shared, msgs, sigs, runs):
    """the pieces that existed before, chained through the host: 0 / 1-scalar batched MSM + normalize, hashes, decoded signatures, m products"""
    m = len(msgs)
    walls = []
    for r in range(runs + 1):
        t0 = time.perf_counter()
        _, apk, ainf = msm_baseline(xy, offsets, bits, shared, 0)
        hxy, att = ffi.hash_to_g1_direct(ffi.SIG_DOMAIN, msgs, None)
        sxy, sst = ffi.decompress("g1", sigs.tobytes())
        g1 = np.stack([sxy, hxy], axis=1).reshape(2 * m, 12)
        g2 = np.stack([np.broadcast_to(NEG_G2, apk.shape), apk], axis=1).reshape(2 * m, 24)
        i2 = np.stack([np.zeros(m, dtype=np.uint8), ainf], axis=1).reshape(2 * m)
        ok = ffi.pairing_product_is_one_batch(g1, None, g2, i2, np.arange(0, 2 * m + 1, 2, dtype=np.uint32))
        if r:
            walls.append((time.perf_counter() - t0) * 1e3)
        assert ok.all() and not sst.any()
    return {"python_wall": spread(walls)}


def seam_a_loop(xy, bits, msgs, sigs):
    """one aggregate_public_keys + verify_signature per seal on key handles, one thread"""
    lib = C.CDLL(ffi.LIB_PATH)
    for f in ("deserialize_public_key", "deserialize_signature", "aggregate_public_keys", "verify_signature", "destroy_public_key", "destroy_signature"):
        getattr(lib, f).restype = C.c_bool
    enc, st = ffi.encode_points("g2", xy)
    handles = []
    for i in range(xy.shape[0]):
        h = C.c_void_p()
        assert lib.deserialize_public_key(enc[i].tobytes(), C.c_int(96), C.byref(h))
        handles.append(h)
    t0 = time.perf_counter()
    for i, msg in enumerate(msgs):
        chosen = [handles[j].value for j in np.flatnonzero(bits[i])]
        arr = (C.c_void_p * len(chosen))(*chosen)
        apk, s, v = C.c_void_p(), C.c_void_p(), C.c_bool(False)
        assert lib.aggregate_public_keys(arr, C.c_int(len(chosen)), C.byref(apk))
        assert lib.deserialize_signature(sigs[i].tobytes(), C.c_int(48), C.byref(s))
        assert lib.verify_signature(apk, msg, C.c_int(len(msg)), b"", C.c_int(0), s, C.c_bool(False), C.c_bool(False), C.byref(v)) and v.value
        lib.destroy_public_key(apk); lib.destroy_signature(s)
    per = (time.perf_counter() - t0) * 1e3 / len(msgs)
    for h in handles:
        lib.destroy_public_key(h)
    return {"seals": len(msgs), "ms_per_seal": per, "ms_total": per * len(msgs), "threads": 1}


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
    a = ap.parse_args()
    ffi.init(0)
    rng = np.random.default_rng(11)
    gen2 = co.pack_g2_377([ecc.G2_377])[0][0]
    gen1 = co.pack_g1_377([ecc.G1_377])[0][0]
    doc = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "timer": "kernels: HIP events around count + sums + normalisation (celo_amd_seals_last)", "shapes": {}}
    shapes = [("epoch_17280x110_shared", 17280, 110, True), ("sets_4096x256", 4096, 256, False), ("small_64x110_shared", 64, 110, True)]
    for label, m, n, shared in shapes:
        print("[bench_seals] %s" % label, file=sys.stderr, flush=True)
        rows = n if shared else m * n
        ks = uniform_scalars(rows, rng)
        xy, inf = ffi.fixed_base_mul("bls12_377_g2", gen2, ks)
        assert not inf.any()
        bits = epoch_bitmaps(m, n, rng)
        offsets = np.array([0, n], dtype=np.uint32) if shared else (np.arange(m + 1, dtype=np.uint64) * n).astype(np.uint32)
        call_bits = bits if shared else bits.reshape(-1)
        ones = np.count_nonzero(bits, axis=1)
        rec = {"seals": m, "set_size": n, "shared_set": shared, "signers": {"min": int(ones.min()), "max": int(ones.max())},
               "most_rows_added": {"ones": int(ones.max()), "complement": int((n - ones).max())},
               "bls12_377_g2": sweep("bls12_377_g2", xy, offsets, call_bits, shared, a.runs)}
        if label.startswith("epoch"):
            xy1, inf1 = ffi.fixed_base_mul("bls12_377_g1", gen1, uniform_scalars(rows, rng))
            rec["bls12_377_g1"] = sweep("bls12_377_g1", xy1, offsets, call_bits, shared, a.runs)
        doc["shapes"][label] = rec
        dump(doc, a.out)                                 # (what has been measured so far survives a failure further on)
        got = ffi.aggregate_by_bitmap("bls12_377_g2", xy, None, offsets, call_bits)
        print("[bench_seals] %s: the MSM path" % label, file=sys.stderr, flush=True)
        base, brows, binf = msm_baseline(xy, offsets, bits, shared, min(a.runs, 2))
        assert np.array_equal(got[0], np.where(binf[:, None] != 0, 0, brows)) and np.array_equal(got[1], binf), "the two paths disagree"
        rec["msm_batch_0_1_scalars_plus_normalize"] = base
        rec["msm_path_over_rule_python_wall"] = base["python_wall"]["median"] / rec["bls12_377_g2"]["complement_by_rule"]["rule"]["python_wall"]["median"]
        dump(doc, a.out)
        # the same seals to verdicts: signed here under the summed keys
        print("[bench_seals] %s: verdicts" % label, file=sys.stderr, flush=True)
        sk = co.limbs_to_ints(ks, 4)
        sums = [sum(sk[(0 if shared else i * n) + int(j)] for j in np.flatnonzero(bits[i])) % ecc.R377 for i in range(m)]
        msgs = [b"block %08d of the benchmark chain" % i for i in range(m)]
        sigs, att = ffi.sign_batch(co.ints_to_limbs(sums, 4), ffi.SIG_DOMAIN, msgs, None, 0)
        assert (att != 255).all()
        ver = {"each": run_verify(xy, offsets, call_bits, msgs, sigs, 0, a.runs), "combined": run_verify(xy, offsets, call_bits, msgs, sigs, 1, a.runs)}
        ver["combined_over_each_wall"] = ver["combined"]["wall"]["median"] / ver["each"]["wall"]["median"]
        ver["chained_before"] = chained_before(xy, offsets, bits, shared, msgs, sigs, min(a.runs, 2))
        ver["chained_before_over_each_python_wall"] = ver["chained_before"]["python_wall"]["median"] / ver["each"]["python_wall"]["median"]
        if m <= 64:
            ver["seam_a_loop"] = seam_a_loop(xy, bits, msgs, sigs)
            ver["seam_a_loop_over_each_python_wall"] = ver["seam_a_loop"]["ms_total"] / ver["each"]["python_wall"]["median"]
        rec["verify_aggregated_seals"] = ver
        dump(doc, a.out)
    print(dump(doc, a.out))


if __name__ == "__main__":
    main()
