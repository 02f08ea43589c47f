"""Epoch blocks to Groth16 public inputs and verdicts on the device (verify_epoch_proofs_bw6_761, csrc/unit_epoch.hip).

  python tools/bench_epoch_inputs.py [--runs 3] [--out profiles/bench_epoch_inputs.json] [--batches 64,1024,16421] [--keys 110,150]

Batches of 64 / 1 024 / 16 421 proofs with blocks of 110 and of 150 keys (n_keys = maximum_validators).  The blocks and proofs repeat a pool of
four (first, last) pairs with one proof each, valid BY CONSTRUCTION for the oracle's inputs of its pair (tests/groth16_verify_cases.py), so every
verdict is 1 and every stage does its whole work.  Per shape, in one process: --runs calls after one warm-up; the stage times of
celo_amd_epoch_last (HIP events; the verifier and the whole call are wall clocks) with their spread, and the wall time seen from Python.
key_dedup: the call with the key de-duplication switch (celo_amd_key_dedup_set) at 0, -1 and 1 in the same run.
In the same run, what the call replaces:
  seam_a_loop        one Seam A `verify` per proof (64 proofs; host decoding, encoding and hashing, GPU input MSM and product)
  pieces_through_host decompress_bls12_377_g2 for every key, the blocks encoded and hashed on the host - by the Python restatement
                     (oracle/py/epoch.py), the only host encoder of many blocks in the tree, at 64 proofs - and
                     groth16_verify_batch_bw6_761_serialized; the device pieces are timed at every batch size
No threshold is fixed in advance.  Prints one JSON document."""
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
from oracle.py import epoch as ep  # noqa: E402
from celo_bls_snark_rs_amd import ffi  # noqa: E402
import epoch_cases as EC  # noqa: E402
import groth16_verify_cases as gc  # noqa: E402

POOL = 4
STAGES = ("decode", "sums", "pack", "hash", "transfers", "verify", "wall")


def spread(vals):
    return {"min": round(min(vals), 4), "median": round(statistics.median(vals), 4), "max": round(max(vals), 4)}


def pair_pool(n_keys):
    """POOL (first, last) pairs of n_keys keys each, drawn from 2 n_keys pool keys at rotating starts"""
    out = []
    for p in range(POOL):
        f = EC.Case(100 + p, 1, EC.entropy(40 + p), EC.entropy(50 + p), n_keys // 3, n_keys, [(7 * p + j) % (2 * n_keys) for j in range(n_keys)])
        l = EC.Case(101 + p, 2, EC.entropy(60 + p), EC.entropy(70 + p), n_keys // 3, n_keys, [(11 * p + 3 + j) % (2 * n_keys) for j in range(n_keys)])
        out.append((f, l))
    return out


class EpochBlockFFI(C.Structure):
    _fields_ = [("index", C.c_uint16), ("round", C.c_uint8), ("epoch_entropy", C.c_char_p), ("parent_entropy", C.c_char_p), ("pubkeys", C.c_char_p),
                ("pubkeys_num", C.c_size_t), ("maximum_non_signers", C.c_uint32), ("maximum_validators", C.c_size_t)]


def seam_a_loop(key, pairs, sers, m):
    lib = C.CDLL(ffi.LIB_PATH)
    lib.verify.restype = C.c_bool
    lib.verify.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, EpochBlockFFI, EpochBlockFFI]
    vk = key.serialize()
    seam = lambda c: EpochBlockFFI(c.index, c.round, c.ee, c.pe, b"".join(EC.pool_bytes(k) for k in c.keys), len(c.keys), c.mns, c.maxv)
    blocks = [(seam(f), seam(l)) for f, l in pairs]
    assert lib.verify(vk, len(vk), sers[0], 288, *blocks[0])                     # warm-up
    t0 = time.perf_counter()
    for i in range(m):
        assert lib.verify(vk, len(vk), sers[i % POOL], 288, *blocks[i % POOL])
    total = (time.perf_counter() - t0) * 1e3
    return {"proofs": m, "ms_total": round(total, 3), "ms_per_proof": round(total / m, 3)}


def pieces_through_host(vk, pairs, sers, m, runs, with_host_encoding):
    firsts, lasts = [pairs[i % POOL][0] for i in range(m)], [pairs[i % POOL][1] for i in range(m)]
    keys = b"".join(EC.pool_bytes(k) for c in firsts + lasts for k in c.keys)
    proofs = b"".join(sers[i % POOL] for i in range(m))
    x = EC.inputs_limbs([pairs[i % POOL] for i in range(m)])
    rec = {"decompress_wall": [], "verify_serialized_wall": []}
    for r in range(runs + 1):
        t0 = time.perf_counter()
        rows, st = ffi.decompress("g2", keys)
        t1 = time.perf_counter()
        ok = vk.verify_serialized(proofs, x, mode=0)
        t2 = time.perf_counter()
        assert not st.any() and ok.all()
        if r:
            rec["decompress_wall"].append((t1 - t0) * 1e3)
            rec["verify_serialized_wall"].append((t2 - t1) * 1e3)
    out = {k: spread(v) for k, v in rec.items()}
    if with_host_encoding:
        t0 = time.perf_counter()
        for f, l in zip(firsts, lasts):                                          # every block afresh: no cache of the pool's bytes
            bits = ep.hash_to_bits(f.block().encode_first_epoch_to_bytes_cip22()) + ep.hash_to_bits(l.block().encode_last_epoch_to_bytes_with_aggregated_pk_cip22())
            ep.pack(bits)
        out["host_encode_hash_python_wall"] = round((time.perf_counter() - t0) * 1e3, 3)
        out["total_wall"] = round(out["decompress_wall"]["median"] + out["verify_serialized_wall"]["median"] + out["host_encode_hash_python_wall"], 3)
    return out


def run_shape(vk, pairs, sers, m, runs):
    idx = [i % POOL for i in range(m)]
    bf = ffi.EpochBlocks(**EC.arrays([pairs[i][0] for i in idx]))
    bl = ffi.EpochBlocks(**EC.arrays([pairs[i][1] for i in idx]))
    proofs = b"".join(sers[i] for i in idx)
    recs = []
    for r in range(runs + 1):                                                    # the first is the warm-up
        t0 = time.perf_counter()
        ok, st = ffi.verify_epoch_proofs(vk, proofs, bf, bl, mode=0)
        wall = (time.perf_counter() - t0) * 1e3
        assert ok.all() and not st.any()
        if r:
            recs.append(dict(ffi.epoch_last(), python_wall=wall))
    out = {k: spread([x[k] for x in recs]) for k in STAGES + ("python_wall",)}
    med = {k: out[k]["median"] for k in STAGES}
    out["dominant_stage"] = max(("decode", "sums", "pack", "hash", "transfers", "verify"), key=lambda k: med[k])
    out["pack_plus_hash_over_decode"] = round((med["pack"] + med["hash"]) / med["decode"], 4)
    out["inputs_over_verify"] = round((med["wall"] - med["verify"]) / med["verify"], 4)
    # the inputs alone, device resident outputs copied back
    walls = []
    for r in range(runs + 1):
        t0 = time.perf_counter()
        x, st = ffi.epoch_public_inputs(bf, bl)
        if r:
            walls.append((time.perf_counter() - t0) * 1e3)
    assert np.array_equal(x, EC.inputs_limbs([pairs[i] for i in idx[:POOL]])[[i for i in idx]])
    out["epoch_public_inputs_python_wall"] = spread(walls)
    return out


def run_key_dedup(vk, pairs, sers, m, runs):
    """verify_epoch_proofs with the key de-duplication switch (celo_amd_key_dedup_set) at 0 (never), -1 (the rule) and 1 (always), in one run:
    the "decode" slot of celo_amd_epoch_last, the wall clock inside the call and the one seen from Python"""
    idx = [i % POOL for i in range(m)]
    bf = ffi.EpochBlocks(**EC.arrays([pairs[i][0] for i in idx]))
    bl = ffi.EpochBlocks(**EC.arrays([pairs[i][1] for i in idx]))
    proofs = b"".join(sers[i] for i in idx)
    out = {}
    try:
        for label, on in (("off", 0), ("rule", -1), ("always", 1)):
            ffi.key_dedup_set(on)
            recs = []
            for r in range(runs + 1):
                t0 = time.perf_counter()
                ok, st = ffi.verify_epoch_proofs(vk, proofs, bf, bl, mode=0)
                wall = (time.perf_counter() - t0) * 1e3
                assert ok.all() and not st.any()
                if r:
                    recs.append(dict(ffi.epoch_last(), python_wall=wall))
            out[label] = {"decode_ms": spread([x["decode"] for x in recs]), "wall_ms": spread([x["wall"] for x in recs]), "python_wall_ms": spread([x["python_wall"] for x in recs])}
        out["last_dedup_call"] = dict(zip(("keys", "decoded", "stage_ms"), ffi.key_dedup_last()))
    finally:
        ffi.key_dedup_set(-1)
    out["decode_off_over_always"] = round(out["off"]["decode_ms"]["median"] / out["always"]["decode_ms"]["median"], 3)
    out["wall_off_over_always"] = round(out["off"]["wall_ms"]["median"] / out["always"]["wall_ms"]["median"], 3)
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
    ap.add_argument("--batches", default="64,1024,16421")
    ap.add_argument("--keys", default="110,150", help="keys per block")
    a = ap.parse_args()
    ffi.init(0)
    key = gc.Key(2, 0xBE7C)
    vk = ffi.VerifyingKey(key.alpha, key.beta, key.gamma, key.delta, key.abc)
    doc = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "mode": "each",
           "timer": "stages: HIP events on the call's stream (celo_amd_epoch_last); verify, wall: wall clocks inside the call; python_wall: around the wrapper",
           "shapes": {}}
    for n_keys in [int(v) for v in a.keys.split(",")]:
        pairs = pair_pool(n_keys)
        rng = ecc.SplitMix64(n_keys)
        batch = gc.Batch(key, [gc.valid_proof(key, rng, x=EC.expected_inputs(f, l)) for f, l in pairs])
        ser = batch.serialize()
        sers = [ser[288 * i:288 * i + 288] for i in range(POOL)]
        for m in [int(v) for v in a.batches.split(",")]:
            label = "%dx%d" % (m, n_keys)
            print("[bench_epoch_inputs] %s" % label, file=sys.stderr, flush=True)
            rec = {"proofs": m, "keys_per_block": n_keys, "keys": 2 * m * n_keys, "verify_epoch_proofs": run_shape(vk, pairs, sers, m, a.runs)}
            rec["key_dedup"] = run_key_dedup(vk, pairs, sers, m, a.runs)
            rec["pieces_through_host"] = pieces_through_host(vk, pairs, sers, m, min(a.runs, 2), m <= 64)
            ours = rec["verify_epoch_proofs"]["python_wall"]["median"]
            if m <= 64:
                rec["seam_a_loop"] = seam_a_loop(key, pairs, sers, m)
                rec["seam_a_loop_over_ours"] = round(rec["seam_a_loop"]["ms_total"] / ours, 2)
                rec["pieces_through_host_over_ours"] = round(rec["pieces_through_host"]["total_wall"] / ours, 2)
            rec["device_pieces_over_ours"] = round((rec["pieces_through_host"]["decompress_wall"]["median"] + rec["pieces_through_host"]["verify_serialized_wall"]["median"]) / ours, 3)
            doc["shapes"][label] = rec
            dump(doc, a.out)                             # (what has been measured so far survives a failure further on)
    vk.release()
    print(dump(doc, a.out))


if __name__ == "__main__":
    main()
