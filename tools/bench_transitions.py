"""Chains of epoch transitions to verdicts (verify_epoch_transitions_bls12_377, csrc/unit_transitions.hip) and the device-resident hash path
under it (csrc/unit_hash.hip).

  python tools/bench_transitions.py [--runs 3] [--out profiles/bench_transitions.json]

Shapes: one chain of 143 transitions x 150 keys (a proof's range), 2 048 transitions x 110 keys in chains of 143 (a sync), 64 x 110.  Keys are
seeded secrets from a pool, 2/3 + 1 .. all of a set sign, every transition is valid (signed in the run by sign_batch_bls12_377, composite CIP22).
Per shape, in one process, --runs runs after one warm-up, with spread:
  the call in both modes with the stage split of celo_amd_transitions_last;
  the call with the key de-duplication switch (celo_amd_key_dedup_set) at 0, -1 and 1: the "decode" slot and the wall time of each;
  the same job through the pieces that were there before, via the host: decompress_bls12_377_g2 + epoch_encode_blocks_bls12_377 (inner) +
  verify_aggregated_seals_bls12_377 (hash mode 3, per-seal sets) - the keys decoded twice, the hash rows through the host;
  at 64 transitions, a loop of the Seam A calls (encode_epoch_block_to_bytes_cip22 + aggregate_public_keys + verify_signature).
Then hash_to_g1_composite_bls12_377_dev (CIP22) against its host form at 2^16 messages of 127 bytes.
Same-run comparisons, none against a threshold fixed in advance.  Prints one JSON document."""
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
import torch  # noqa: E402  (before the library: both must share one HIP runtime)
from oracle.py import ecc  # noqa: E402
from oracle import cpu_oracle as co  # noqa: E402
from celo_bls_snark_rs_amd import ffi  # noqa: E402

POOL = 512
NEG_G2 = co.pack_g2_377([ecc.E2_377.neg(ecc.G2_377)])[0][0]


def spread(vals):
    return {"min": round(min(vals), 4), "median": round(statistics.median(vals), 4), "max": round(max(vals), 4)}


def pool(rng):
    sks = [int(rng.integers(1, 1 << 62)) * int(rng.integers(1, 1 << 62)) % ecc.R377 for _ in range(POOL)]
    rows, inf = ffi.fixed_base_mul("bls12_377_g2", co.pack_g2_377([ecc.G2_377])[0][0], co.ints_to_limbs(sks, 4))
    enc, st = ffi.encode_points("g2", rows)
    assert not inf.any() and not st.any()
    return sks, rows, enc


def world(n_tr, n_keys, per_chain, sks, enc, rng):
    """valid chains: (EpochBlocks, chain_off, bits, signatures, and what the host path needs)"""
    lens = [per_chain] * (n_tr // per_chain) + ([n_tr % per_chain] if n_tr % per_chain else [])
    chain_off = np.concatenate([[0], np.cumsum([l + 1 for l in lens])]).astype(np.uint32)
    nb = int(chain_off[-1])
    initial = np.zeros(nb, dtype=bool)
    initial[chain_off[:-1]] = True
    pos = np.arange(nb) - np.repeat(chain_off[:-1], [l + 1 for l in lens])
    index = (100 + pos + 300 * np.repeat(np.arange(len(lens)), [l + 1 for l in lens])) % 65000
    ee = rng.integers(1, 256, size=(nb, 16), dtype=np.uint8)
    pe = np.roll(ee, 1, axis=0)
    which = np.stack([rng.permutation(POOL)[:n_keys] for _ in range(nb)])
    bits = np.ones((nb, n_keys), dtype=np.uint8)
    for i, k in enumerate(rng.integers(2 * n_keys // 3 + 1, n_keys + 1, size=nb)):
        bits[i, rng.permutation(n_keys)[:n_keys - int(k)]] = 0
    key_off = np.arange(nb + 1, dtype=np.uint32) * n_keys
    blocks = ffi.EpochBlocks(index, rng.integers(0, 256, size=nb), np.full(nb, n_keys // 3, dtype=np.uint32), np.full(nb, n_keys, dtype=np.uint32), ee, pe,
                             enc[which.reshape(-1)], key_off)
    msgs, extras, est, _ = ffi.epoch_encode_blocks(blocks, "inner")
    assert not est.any()
    sk = [0 if initial[i] else sum(sks[j] for j, x in zip(which[i - 1], bits[i - 1]) if x) % ecc.R377 for i in range(nb)]
    sig, att = ffi.sign_batch(co.ints_to_limbs(sk, 4), ffi.SIG_DOMAIN, msgs, [e.tobytes() for e in extras], 3)
    assert (att != 255).all()
    return dict(blocks=blocks, chain_off=chain_off, bits=bits.reshape(-1), sig=sig, nb=nb, initial=initial, n_keys=n_keys, which=which, bits2=bits, ee=ee, pe=pe)


def timed(fn, runs):
    fn()
    walls, recs = [], []
    for _ in range(runs):
        t0 = time.perf_counter()
        recs.append(fn())
        walls.append((time.perf_counter() - t0) * 1e3)
    return walls, recs


def run_call(w, mode, runs):
    def once():
        r = ffi.verify_epoch_transitions(w["blocks"], w["chain_off"], w["bits"], w["sig"], ffi.SIG_DOMAIN, NEG_G2, mode=mode, want=("status",))
        assert r["ok"].all()
        return ffi.transitions_last()
    walls, recs = timed(once, runs)
    out = {"python_wall_ms": spread(walls), "path": recs[-1]["path"]}
    out["stages_ms"] = {k: spread([r["ms"][k] for r in recs]) for k in recs[-1]["ms"]}
    return out


def run_key_dedup(w, runs):
    """the call (mode each) with the key de-duplication switch at 0 (never), -1 (the rule) and 1 (always), in one run: the "decode" slot of
    celo_amd_transitions_last and the wall time"""
    out = {}
    try:
        for label, on in (("off", 0), ("rule", -1), ("always", 1)):
            ffi.key_dedup_set(on)
            r = run_call(w, 0, runs)
            out[label] = {"decode_ms": r["stages_ms"]["decode"], "wall_ms": r["stages_ms"]["wall"], "python_wall_ms": r["python_wall_ms"]}
        out["last_dedup_call"] = dict(zip(("keys", "decoded", "stage_ms"), ffi.key_dedup_last()))
    finally:
        ffi.key_dedup_set(-1)
    out["decode_off_over_always"] = round(out["off"]["decode_ms"]["median"] / out["always"]["decode_ms"]["median"], 3)
    out["wall_off_over_always"] = round(out["off"]["wall_ms"]["median"] / out["always"]["wall_ms"]["median"], 3)
    return out


def run_pieces(w, runs):
    """decode the keys, encode the blocks (which decodes them again), then the seals entry with the predecessor's rows per seal"""
    b, nk = w["blocks"], w["n_keys"]
    tr = np.flatnonzero(~w["initial"])
    offsets = (np.arange(len(tr) + 1) * nk).astype(np.uint32)
    mins = np.full(len(tr), nk - nk // 3, dtype=np.uint32)
    split = {"decode": [], "encode": [], "seals": []}

    def once():
        t0 = time.perf_counter()
        rows, st = ffi.decompress("g2", b.keys.tobytes())
        t1 = time.perf_counter()
        msgs, extras, est, _ = ffi.epoch_encode_blocks(b, "inner")
        t2 = time.perf_counter()
        pk = rows.reshape(w["nb"], nk, 24)[tr - 1].reshape(-1, 24)
        ok, _ = ffi.verify_aggregated_seals(pk, None, offsets, w["bits2"][tr - 1].reshape(-1), mins, ffi.SIG_DOMAIN, [msgs[i] for i in tr], [extras[i].tobytes() for i in tr],
                                            w["sig"][tr], NEG_G2, hash_mode=3, mode=0)
        t3 = time.perf_counter()
        assert ok.all() and not st.any()
        for k, v in zip(("decode", "encode", "seals"), (t1 - t0, t2 - t1, t3 - t2)):
            split[k].append(v * 1e3)
    walls, _ = timed(once, runs)
    return {"python_wall_ms": spread(walls), "split_ms": {k: spread(v[1:]) for k, v in split.items()}}


def run_seam_a(w, enc, runs):
    lib = C.CDLL(ffi.LIB_PATH)
    for name in ("deserialize_public_key", "deserialize_signature", "aggregate_public_keys", "verify_signature", "destroy_public_key", "destroy_signature",
                 "encode_epoch_block_to_bytes_cip22", "free_vec"):
        getattr(lib, name).restype = C.c_bool
    handles = []
    for e in enc:
        h = C.c_void_p()
        assert lib.deserialize_public_key(e.tobytes(), C.c_int(96), C.byref(h))
        handles.append(h)
    b = w["blocks"]

    def once():
        for i in np.flatnonzero(~w["initial"]):
            own = (C.c_void_p * w["n_keys"])(*[handles[j].value for j in w["which"][i]])
            ob, ol, xb, xl = C.POINTER(C.c_uint8)(), C.c_int(0), C.POINTER(C.c_uint8)(), C.c_int(0)
            assert lib.encode_epoch_block_to_bytes_cip22(C.c_ushort(int(b.index[i])), C.c_ubyte(int(b.round[i])), w["ee"][i].tobytes(), w["pe"][i].tobytes(), C.c_uint(int(b.mns[i])),
                                                         C.c_uint(int(b.maxv[i])), own, C.c_int(w["n_keys"]), C.byref(ob), C.byref(ol), C.byref(xb), C.byref(xl))
            chosen = [handles[j] for j, x in zip(w["which"][i - 1], w["bits2"][i - 1]) if x]
            arr = (C.c_void_p * len(chosen))(*[h.value for h in chosen])
            apk, s, verdict = C.c_void_p(), C.c_void_p(), C.c_bool(False)
            assert lib.aggregate_public_keys(arr, C.c_int(len(chosen)), C.byref(apk))
            assert lib.deserialize_signature(w["sig"][i].tobytes(), C.c_int(48), C.byref(s))
            assert lib.verify_signature(apk, ob, ol, xb, xl, s, C.c_bool(True), C.c_bool(True), C.byref(verdict)) and verdict.value
            lib.destroy_public_key(apk), lib.destroy_signature(s), lib.free_vec(ob, ol), lib.free_vec(xb, xl)
    walls, _ = timed(once, runs)
    for h in handles:
        lib.destroy_public_key(h)
    return {"python_wall_ms": spread(walls)}


def run_hash(runs, rng):
    n = 1 << 16
    data = rng.integers(0, 256, size=n * 127, dtype=np.uint8)
    ex = rng.integers(0, 256, size=n * 7, dtype=np.uint8)
    moff, eoff = np.arange(n + 1, dtype=np.uint64) * 127, np.arange(n + 1, dtype=np.uint64) * 7
    d_m, d_e = torch.from_numpy(data).cuda(), torch.from_numpy(ex).cuda()
    d_xy = torch.zeros(n * 96, dtype=torch.uint8, device="cuda")
    d_att = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    dom = np.frombuffer(ffi.SIG_DOMAIN, dtype=np.uint8)
    xy, att = np.zeros((n, 12), dtype=np.uint64), np.zeros(n, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def host():          # the C entry on packed arrays: no Python packing inside the timed region
        assert ffi.lib().hash_to_g1_composite_bls12_377(p(dom), p(data), p(moff), p(ex), p(eoff), C.c_size_t(n), C.c_int(1), p(xy), p(att)) == 0
        return ffi.hash_last_ms()

    def dev():
        assert ffi.hash_to_g1_dev(ffi.SIG_DOMAIN, d_m.data_ptr(), moff, d_e.data_ptr(), eoff, n, d_xy.data_ptr(), d_att.data_ptr(), mode=3) == 0
        return ffi.hash_last_ms()
    hw, hk = timed(host, runs)
    dw, dk = timed(dev, runs)
    assert np.array_equal(d_xy.cpu().numpy().view(np.uint64).reshape(n, 12), xy) and np.array_equal(d_att.cpu().numpy(), att)
    return {"n": n, "message_bytes": 127, "host_form": {"wall_ms": spread(hw), "rounds_kernel_ms": spread(hk)}, "device_form": {"wall_ms": spread(dw), "rounds_kernel_ms": spread(dk)},
            "host_over_device_wall": round(statistics.median(hw) / statistics.median(dw), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_transitions.json"))
    a = ap.parse_args()
    ffi.init(0)
    rng = np.random.default_rng(2025)
    sks, rows, enc = pool(rng)
    doc = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "shapes": {}}
    for name, n_tr, n_keys, per in (("proof_143x150", 143, 150, 143), ("sync_2048x110", 2048, 110, 143), ("small_64x110", 64, 110, 64)):
        w = world(n_tr, n_keys, per, sks, enc, rng)
        rec = {"transitions": n_tr, "keys": n_keys, "chains": len(w["chain_off"]) - 1, "each": run_call(w, 0, a.runs), "chain": run_call(w, 1, a.runs),
               "pieces_via_host": run_pieces(w, a.runs), "key_dedup": run_key_dedup(w, a.runs)}
        if n_tr == 64:
            rec["seam_a_loop"] = run_seam_a(w, enc, a.runs)
        each, chain, pieces = (rec[k]["python_wall_ms"]["median"] for k in ("each", "chain", "pieces_via_host"))
        rec["pieces_over_each"] = round(pieces / each, 3)
        rec["each_over_chain"] = round(each / chain, 3)
        stages = rec["each"]["stages_ms"]
        rec["dominant_stage_each"] = max((k for k in stages if k != "wall"), key=lambda k: stages[k]["median"])
        doc["shapes"][name] = rec
    doc["hash_composite_cip22_2^16"] = run_hash(a.runs, rng)
    text = json.dumps(doc, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
