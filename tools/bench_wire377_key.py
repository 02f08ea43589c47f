"""Kernel time of the uncompressed BLS12-377 point decoders (csrc/unit_wire.hip k_decode377u) beside the compressed ones, and the phases of
the serialized ProvingKey<Bls12_377> writer and loader.

  python tools/bench_wire377_key.py [--log-n 20] [--log-vars 18] [--reps 3] [--out profiles/bench_wire377_key.json]

Points: n = 2^log_n subgroup points per group (k_i G from celo_amd_gen_points_bls12_377_*_dev), encoded on the device in both forms
(compress_* / encode_uncompressed_*_dev), decoded from device memory.  Per group: decode_uncompressed checked and unchecked, and
decompress_* checked on the same points in the same run, kernel time by HIP events (celo_amd_decompress_last_ms), best of --reps after a
warm-up; the ratio compressed / uncompressed (checked) is stated.
Key: 2^log_vars variables, 2 inputs, n_h = 2^log_vars - 1, rows taken from the same points.  groth16_serialize_key in forms 0 and 1 (rows in,
encode, bytes out), then groth16_load_key_bls12_377_serialized of those bytes in forms 0, 1 and 2 (bytes in, decode, table build) beside
groth16_load_key_bls12_377 from the limb rows (wall).  Prints one JSON document and writes it to --out."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: both must share one HIP runtime)
from oracle.py import ecc  # noqa: E402
from oracle import cpu_oracle as co  # noqa: E402
from celo_bls_snark_rs_amd import ffi  # noqa: E402

GROUPS = {"g1": ("bls12_377_g1", 12, 48), "g2": ("bls12_377_g2", 24, 96)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--log-vars", type=int, default=18)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_wire377_key.json"))
    a = ap.parse_args()
    ffi.init(0)
    n, n_vars = 1 << a.log_n, 1 << a.log_vars
    assert n_vars <= n
    res = {"n": n, "device": torch.cuda.get_device_name(0), "reps": a.reps, "decode": {}}
    rows = {}
    for g, (gen_group, words, size) in GROUPS.items():
        gen = co.pack_g1_377([ecc.G1_377])[0][0] if g == "g1" else co.pack_g2_377([ecc.G2_377])[0][0]
        d_rows = torch.empty(n * words, dtype=torch.int64, device="cuda")
        ffi.gen_points_dev(gen_group, d_rows.data_ptr(), n, 377 + (g == "g2"), gen)
        d_st = torch.empty(n, dtype=torch.uint8, device="cuda")
        d_enc = {c: torch.empty(n * size * (1 if c else 2), dtype=torch.uint8, device="cuda") for c in (True, False)}
        for c in (True, False):
            ffi.encode_points_dev(g, d_rows.data_ptr(), 0, n, d_enc[c].data_ptr(), d_st.data_ptr(), compressed=c)
            torch.cuda.synchronize()
            assert int(d_st.max()) == 0
        d_out = torch.empty(n * words, dtype=torch.int64, device="cuda")
        for mode, comp, check in (("uncompressed_checked", False, True), ("uncompressed_unchecked", False, False), ("compressed_checked", True, True)):
            kms = []
            for _ in range(a.reps + 1):
                d_out.zero_()
                if comp:
                    ffi.decompress_dev(g, d_enc[True].data_ptr(), n, d_out.data_ptr(), d_st.data_ptr(), check_subgroup=check)
                else:
                    assert ffi.decode_uncompressed_dev(g, d_enc[False].data_ptr(), n, d_out.data_ptr(), d_st.data_ptr(), check=check) == 0
                torch.cuda.synchronize()
                kms.append(ffi.decompress_last_ms())
                assert int(d_st.max()) == 0 and torch.equal(d_out, d_rows), mode     # every point decodes to the row it was encoded from
            km = min(kms[1:])
            res["decode"]["%s_%s" % (g, mode)] = {"kernel_ms": round(km, 3), "points_per_s": round(n / (km * 1e-3))}
            print(g, mode, res["decode"]["%s_%s" % (g, mode)], flush=True)
        res["decode"][g + "_compressed_over_uncompressed_checked"] = round(
            res["decode"][g + "_compressed_checked"]["kernel_ms"] / res["decode"][g + "_uncompressed_checked"]["kernel_ms"], 2)
        rows[g] = d_rows.cpu().numpy().view(np.uint64).reshape(n, words)
    # the key: limb rows in the order of groth16_setup_bls12_377's out_vk / out_rows
    n_inputs, n_h = 2, n_vars - 1
    g1, g2 = rows["g1"], rows["g2"]
    vk = np.concatenate([g1[0], g2[0], g2[1], g2[2], g1[1:1 + n_inputs].reshape(-1)])
    q = {"a_query": g1[:n_vars], "b_g1_query": g1[n_vars:2 * n_vars], "b_g2_query": g2[:n_vars], "h_query": g1[2 * n_vars:2 * n_vars + n_h],
         "l_query": g1[3 * n_vars:3 * n_vars + n_vars - n_inputs]}
    flat = np.concatenate([g1[3], g1[4]] + [q[k].reshape(-1) for k in ("a_query", "b_g1_query", "b_g2_query", "h_query", "l_query")])
    res["key"] = {"n_vars": n_vars, "n_inputs": n_inputs, "n_h": n_h, "write": {}, "load": {}}
    data = {}
    for form in (0, 1):
        runs = []
        for _ in range(2):
            t = time.perf_counter()
            data[form] = ffi.groth16_serialize_key(vk, flat, n_vars, n_h, form, curve="bls12_377")
            wall = time.perf_counter() - t
            ms = ffi.wire_encode_key_timings()
            runs.append({"wall_ms": round(wall * 1e3, 1), "rows_in_ms": round(ms[0], 2), "encode_ms": round(ms[1], 2), "bytes_out_ms": round(ms[2], 2)})
        res["key"]["write"]["form%d" % form] = {"bytes": len(data[form]), "runs": runs}
    for form in (0, 1, 2):
        runs = []
        for _ in range(2):
            t = time.perf_counter()
            k = ffi.ProvingKey.from_serialized(data[min(form, 1)], form, curve="bls12_377")
            wall = time.perf_counter() - t
            ms = ffi.wire761_last_timings()
            k.release()
            runs.append({"wall_ms": round(wall * 1e3, 1), "bytes_in_ms": round(ms[1], 2), "decode_ms": round(ms[2], 2), "table_build_ms": round(ms[3], 1)})
        res["key"]["load"]["form%d" % form] = {"bytes": len(data[min(form, 1)]), "runs": runs}
    runs = []
    for _ in range(2):
        t = time.perf_counter()
        k = ffi.ProvingKey("bls12_377", q["a_query"], q["b_g2_query"], q["h_query"], q["l_query"], g1[0], g2[0])
        runs.append({"wall_ms": round((time.perf_counter() - t) * 1e3, 1)})
        k.release()
    res["key"]["load"]["limb_rows"] = {"runs": runs}
    print(json.dumps(res, indent=1))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
