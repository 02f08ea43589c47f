"""Throughput of the BW6-761 point decoders (csrc/unit_wire761.hip) and wall time of the serialized proving-key loader.

  python tools/bench_wire761.py [--log-n 20] [--reps 3] [--out FILE]

Six modes, G1 / G2 x compressed-checked / uncompressed-checked / uncompressed-unchecked, on n = 2^log_n subgroup points each (k_i G from
celo_amd_gen_points_bw6_761_dev, serialized here), decoded from device memory (decompress_bw6_761_*_dev, and the host entry for the uncompressed
forms): points/s from the kernel time (HIP events) and from the call's wall time.  Then a ProvingKey<BW6_761> with 2^log_n points in each
query (a, b_g1, b_g2, h, l), compressed, loaded by groth16_load_key_bw6_761_serialized: wall time split into the transfer of the bytes, the
decoding of every section and the fixed-base table build.  Prints one JSON document."""
import argparse
import json
import os
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


def encodings(curve, n, seed):
    G = ecc.deser_point(curve, bs.reference_points()[0 if curve is ecc.E1_761 else 1][1])
    d = torch.empty(n * 24, dtype=torch.int64, device="cuda")
    ffi.gen_points_dev("bw6_761_g1", d.data_ptr(), n, seed, co.pack_761([G])[0][0])
    pts = bs.rows_to_points(d.cpu().numpy().view(np.uint64).reshape(n, 24))
    return b"".join(ecc.ser_point(curve, P) for P in pts), b"".join(ecc.ser_point(curve, P, compressed=False) for P in pts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ffi.init(0)
    n = 1 << a.log_n
    res = {"n": n, "device": torch.cuda.get_device_name(0), "modes": {}}
    enc = {}
    for g, curve in (("g1", ecc.E1_761), ("g2", ecc.E2_761)):
        t = time.time()
        enc[g] = encodings(curve, n, 5 + (g == "g2"))
        res["serialize_s_" + g] = round(time.time() - t, 1)
        comp, unc = enc[g]
        group = "bw6_761_" + g
        d_c = torch.from_numpy(np.frombuffer(comp, dtype=np.uint8).copy()).cuda()
        d_out = torch.empty(n * 24, dtype=torch.int64, device="cuda")
        d_st = torch.empty(n, dtype=torch.uint8, device="cuda")
        for mode in ("compressed_checked", "uncompressed_checked", "uncompressed_unchecked"):
            kms, walls = [], []
            for _ in range(a.reps + 1):
                t = time.perf_counter()
                if mode == "compressed_checked":
                    ffi.decompress_dev(group, d_c.data_ptr(), n, d_out.data_ptr(), d_st.data_ptr(), check_subgroup=True)
                    st = d_st.cpu().numpy()
                else:
                    _, st = ffi.decode_uncompressed(group, unc, check=(mode == "uncompressed_checked"))
                walls.append(time.perf_counter() - t)
                kms.append(ffi.wire761_last_timings()[0])
                assert (st == 0).all(), mode
            km, wall = min(kms[1:]), min(walls[1:])
            res["modes"]["%s_%s" % (g, mode)] = {"kernel_ms": round(km, 3), "points_per_s_kernel": round(n / (km * 1e-3)),
                                                  "wall_ms": round(wall * 1e3, 3), "points_per_s_wall": round(n / wall)}
            print(g, mode, res["modes"]["%s_%s" % (g, mode)], flush=True)
    # a key of n points per query: the same encodings reused for a / b_g1 / h / l (G1) and b_g2 (G2) behind the reference's VK
    vk = bs.reference_vk()
    g1c, g2c = enc["g1"][0], enc["g2"][0]
    vec = lambda b: (len(b) // 96).to_bytes(8, "little") + b  # noqa: E731
    key = vk + g1c[:96] + g1c[96:192] + vec(g1c) + vec(g1c) + vec(g2c) + vec(g1c) + vec(g1c)
    loads = []
    for _ in range(2):
        t = time.perf_counter()
        k = ffi.ProvingKey.from_serialized(key, 0)
        wall = time.perf_counter() - t
        ms = ffi.wire761_last_timings()
        k.release()
        loads.append({"wall_ms": round(wall * 1e3, 1), "transfer_ms": round(ms[1], 1), "decode_ms": round(ms[2], 1), "table_build_ms": round(ms[3], 1)})
    res["key_load"] = {"points_per_query": n, "bytes": len(key), "points": 5 * n + 4 + 2 + (int.from_bytes(vk[384:392], "little")), "runs": loads}
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
