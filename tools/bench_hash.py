#!/usr/bin/env python3
"""Batched hash-to-G1 over the direct hasher (hash_to_g1_direct_bls12_377): kernel time from HIP events (the entry point takes
host buffers; the copies are outside the events), hashes/s for 32-byte messages + 2 bytes of extra data (an epoch hash and a
round/epoch tag), and the host-core implementation of Seam A (celo_amd_hash_to_g1 on one thread, bounded sample) beside it.

--g2: the hash-to-G2 leg instead (hash_to_g2_direct_bls12_377) at 2^16 messages seeded like the G1 leg: three runs, each with the whole
call's wall time, the kernel time and its split into candidate rounds and the cofactor kernel; the G1 leg of the same run beside it; and the
cofactor kernel's share of the multiplier roofline (celo_amd_ubench_fp of this run), from the multiply-add count of the form that runs."""
import ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from celo_bls_snark_rs_amd import ffi

# Multiply-adds per message of the two cofactor kernels, counted as bench.py MADS counts the curve formulas (14-limb field: product sweep 196,
# symmetric sweep 105, reduction sweep 182).
FQ_MUL, FQ_SQR, FQ_MULSUB = 196 + 182, 105 + 182, 2 * 196 + 182
FQ2_MUL, FQ2_SQR, FQ2_MULSUB = 2 * (2 * 196 + 182), (2 * 105 + 182) + (196 + 182), 2 * (4 * 196 + 182)
# xyzz_dbl: squarings of U, X, M; products U V, X V, V ZZ, W ZZZ; Y3 in one pass.  xyzz_madd: six products, two squarings, Y3 in one pass.
DBL = {"g1": 3 * FQ_SQR + 4 * FQ_MUL + FQ_MULSUB, "g2": 3 * FQ2_SQR + 4 * FQ2_MUL + FQ2_MULSUB}
MADD = {"g1": 6 * FQ_MUL + 2 * FQ_SQR + FQ_MULSUB, "g2": 6 * FQ2_MUL + 2 * FQ2_SQR + FQ2_MULSUB}
H1 = 0x170b5d44300000000000000000000000
H2 = 0x26ba558ae9562addd88d99a6f6a829fbb36b00e1dcc40c8c505634fae2e189d693e8c36676bd09a0f3622fba094800452217cc900000000000000000000001
# the form that runs for both groups: the MSB-first ladder over the cofactor (bits - 1 doublings, weight - 1 mixed additions)
LADDER_MADS = {g: (h.bit_length() - 1) * DBL[g] + (bin(h).count("1") - 1) * MADD[g] for g, h in (("g1", H1), ("g2", H2))}


def inputs(log_n, rng):
    n = 1 << log_n
    raw = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    return [raw[i].tobytes() for i in range(n)], [b"\x01\x02"] * n


def spread(vals):
    return {"runs": vals, "min": min(vals), "max": max(vals), "spread_frac": (max(vals) - min(vals)) / min(vals)}


def g2_leg(log_n=16):
    n = 1 << log_n
    msgs, extras = inputs(log_n, np.random.default_rng(1))
    ffi.hash_to_g2_direct(b"ULforxof", msgs[:64], extras[:64])            # first use: constants, scratch
    runs = {"call_ms": [], "kernel_ms": [], "candidates_ms": [], "finish_ms": []}
    for _ in range(3):
        t0 = time.perf_counter()
        xy, att = ffi.hash_to_g2_direct(b"ULforxof", msgs, extras)
        runs["call_ms"].append((time.perf_counter() - t0) * 1e3)
        runs["kernel_ms"].append(ffi.hash_last_ms())
        c, f = ffi.hash_g2_last_split()
        runs["candidates_ms"].append(c)
        runs["finish_ms"].append(f)
    assert (att < 255).all()
    rounds = ffi.hash_last_rounds()
    g1 = []
    for _ in range(3):
        _, att1 = ffi.hash_to_g1_direct(b"ULforxof", msgs, extras)
        g1.append(ffi.hash_last_ms())
    u = ffi.ubench_fp()
    peak_tmads = u["fq377_mul_G"] * FQ_MUL / 1e3
    fin = min(runs["finish_ms"])
    achieved = n * LADDER_MADS["g2"] / (fin * 1e-3) / 1e12
    k = min(runs["kernel_ms"])
    return {"n": n, "g2": {key: spread(v) for key, v in runs.items()}, "g2_hashes_per_s": n / (k * 1e-3), "g2_rounds": rounds,
            "g2_mean_attempts": float(att.mean()) + 1.0, "g1_kernel_ms": spread(g1), "g1_hashes_per_s": n / (min(g1) * 1e-3),
            "g1_mean_attempts": float(att1.mean()) + 1.0, "g2_over_g1_kernel_time": k / min(g1),
            "finish_form": "MSB-first ladder over the 502-bit cofactor: 501 doublings + 195 mixed additions in Fq2 (no faster form ships)",
            "finish_multiply_adds_per_message": LADDER_MADS["g2"], "g1_finish_multiply_adds_per_message": LADDER_MADS["g1"],
            "finish_valu_roofline": {"achieved_tmads": achieved, "peak_tmads": peak_tmads, "frac": achieved / peak_tmads,
                                     "note": "n x ladder multiply-adds / best finish-kernel time against celo_amd_ubench_fp's Fq product loop of this run "
                                             "(%.1f G products/s x 378); the affine normalisation (one inversion per message) is not counted" % u["fq377_mul_G"]}}


def main():
    ffi.init(0)
    args = sys.argv[1:]
    if args and args[0] == "--g2":
        print(json.dumps(g2_leg(int(args[1]) if len(args) > 1 else 16)))
        return
    out = {}
    rng = np.random.default_rng(1)
    for log_n in [int(a) for a in args] or [8, 12, 16, 18, 20]:
        n = 1 << log_n
        msgs, extras = inputs(log_n, rng)
        best = None
        for _ in range(3):
            xy, att = ffi.hash_to_g1_direct(b"ULforxof", msgs, extras)
            ms = ffi.hash_last_ms()
            best = ms if best is None or ms < best else best
        assert (att < 255).all()
        res = {"kernel_ms": best, "hashes_per_s": n / (best * 1e-3), "mean_attempts": float(att.mean()) + 1.0,
               "alg_GBps": n * (8 + 35 + 96) / (best * 1e-3) / 1e9}
        res["hbm_roofline_frac"] = res["alg_GBps"] / 8000.0
        if log_n == 12:
            lib = ffi.lib()
            lib.celo_amd_hash_to_g1.restype = C.c_bool
            o = (C.c_ubyte * 48)()
            a = C.c_int(0)
            t0 = time.perf_counter()
            for i in range(512):
                assert lib.celo_amd_hash_to_g1(False, False, b"ULforxof", msgs[i], 32, extras[i], 2, o, C.byref(a))
            res["host_1core_hashes_per_s"] = 512 / (time.perf_counter() - t0)
        if log_n in (12, 16):
            best = None
            for _ in range(3):
                ffi.composite_crh(msgs)
                ms = ffi.hash_last_ms()
                best = ms if best is None or ms < best else best
            res["pedersen_crh_kernel_ms"] = best
            res["pedersen_crh_per_s"] = n / (best * 1e-3)
        out[f"2^{log_n}"] = res
    print(json.dumps(out))


main()
