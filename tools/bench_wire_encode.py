"""Throughput of the point encoders (csrc/unit_wire_encode.hip) and the phases of the serialized proving-key writer.

  python tools/bench_wire_encode.py [--log-n 20] [--reps 20] [--out FILE]

Four groups (BLS12-377 G1 / G2, BW6-761 G1 / G2) x two forms (compressed, uncompressed) on n = 2^log_n points each (k_i G from
celo_amd_gen_points_*_dev), encoded from device memory to device memory (compress_*_dev / encode_uncompressed_*_dev).  Per mode: kernel time
(HIP events inside the call; the minimum and the median of the repetitions after two warm-up calls), points/s, the bytes the kernel moves
(rows read, bytes and status written) per second, and a device-to-device copy moving the same number of bytes, timed in the same run: the
ratio kernel / copy says how far the kernel is from a plain stream.  The first points are compared against oracle/py/ecc.ser_point.

Then a ProvingKey<BW6_761> with 2^log_n points in each query (n_vars = n_h = 2^log_n), from host limb rows, through
groth16_serialize_key_bw6_761 in both forms: rows to the device, encoding, bytes back, and the call's wall time.  Prints one JSON document."""
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

GROUPS = {  # name: (gen_points group, encoder group, u64 per row, compressed bytes, curve, packer)
    "bls12_377_g1": ("bls12_377_g1", "g1", 12, 48, ecc.E1_377, co.pack_g1_377),
    "bls12_377_g2": ("bls12_377_g2", "g2", 24, 96, ecc.E2_377, co.pack_g2_377),
    "bw6_761_g1": ("bw6_761_g1", "bw6_761", 24, 96, ecc.E1_761, co.pack_761),
    "bw6_761_g2": ("bw6_761_g2", "bw6_761", 24, 96, ecc.E2_761, co.pack_761),
}


def generator(name):
    if name.startswith("bw6"):
        curve = GROUPS[name][4]
        return ecc.deser_point(curve, bs.reference_points()[0 if curve is ecc.E1_761 else 1][1])
    return ecc.G1_377 if name.endswith("g1") else ecc.G2_377


def copy_ms(nbytes, reps):
    """a device-to-device copy that moves nbytes in all (half read, half written): the minimum over reps, by events"""
    half = nbytes // 2
    src = torch.empty(half, dtype=torch.uint8, device="cuda").random_(0, 256)
    dst = torch.empty_like(src)
    out = []
    for i in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            out.append(e0.elapsed_time(e1))
    return min(out)


def to_points(name, rows):
    q = GROUPS[name][4].p
    w = 6 if q == ecc.Q377 else 12
    v = co.from_mont(rows.reshape(-1, w), q)
    k = len(v) // rows.shape[0]
    return [(v[k * i], v[k * i + 1]) if k == 2 else ((v[4 * i], v[4 * i + 1]), (v[4 * i + 2], v[4 * i + 3])) for i in range(rows.shape[0])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-key", action="store_true")
    a = ap.parse_args()
    ffi.init(0)
    n = 1 << a.log_n
    res = {"n": n, "device": torch.cuda.get_device_name(0), "reps": a.reps, "modes": {}}
    rows761 = {}
    for name, (gen_group, enc_group, words, size, curve, pack) in GROUPS.items():
        d_rows = torch.empty(n * words, dtype=torch.int64, device="cuda")
        ffi.gen_points_dev(gen_group, d_rows.data_ptr(), n, 11 + len(name), pack([generator(name)])[0][0])
        torch.cuda.synchronize()
        head = d_rows[:8 * words].cpu().numpy().view(np.uint64).reshape(8, words)
        if name.startswith("bw6"):
            rows761[name] = d_rows.cpu().numpy().view(np.uint64).reshape(n, words)
        d_st = torch.empty(n, dtype=torch.uint8, device="cuda")
        for compressed in (True, False):
            ob = size * (1 if compressed else 2)
            d_out = torch.empty(n * ob, dtype=torch.uint8, device="cuda")
            ms = []
            for rep in range(a.reps + 2):                                  # two warm-up calls
                ffi.encode_points_dev(enc_group, d_rows.data_ptr(), 0, n, d_out.data_ptr(), d_st.data_ptr(), compressed)
                if rep >= 2:
                    ms.append(ffi.wire_encode_last_ms())
            assert not d_st.any()
            want = b"".join(ecc.ser_point(curve, P, compressed=compressed) for P in to_points(name, head))
            assert d_out[:8 * ob].cpu().numpy().tobytes() == want, name
            moved = n * (words * 8 + ob + 1)
            cms = copy_ms(moved, a.reps)
            km, med = min(ms), statistics.median(ms)
            r = {"bytes_moved": moved, "copy_same_bytes_ms": round(cms, 4), "copy_GB_per_s": round(moved / cms / 1e6, 1),
                 "kernel_ms_min": round(km, 4), "kernel_ms_median": round(med, 4), "points_per_s": round(n / (km * 1e-3)),
                 "GB_per_s": round(moved / km / 1e6, 1), "kernel_over_copy": round(km / cms, 2)}
            res["modes"]["%s_%s" % (name, "compressed" if compressed else "uncompressed")] = r
            print(name, "compressed" if compressed else "uncompressed", r, flush=True)
            del d_out
        del d_rows
    if not a.no_key:
        # n_vars = n_h = n, two public inputs: a, b_g1, h, l from the G1 rows, b_g2 from the G2 rows
        g1, g2 = rows761["bw6_761_g1"], rows761["bw6_761_g2"]
        n_in = 2
        vk = np.concatenate([g1[:1], g2[:3], g1[:n_in]])
        rows = np.concatenate([g1[:2], g1, g1, g2, g1, g1[:n - n_in]])
        runs = {}
        for form in (0, 1):
            runs["form_%d" % form] = []
            for _ in range(3):
                t = time.perf_counter()
                data = ffi.groth16_serialize_key(vk, rows, n, n, form)
                wall = time.perf_counter() - t
                ph = ffi.wire_encode_key_timings()
                runs["form_%d" % form].append({"wall_ms": round(wall * 1e3, 1), "rows_in_ms": round(ph[0], 1), "encode_ms": round(ph[1], 2), "bytes_out_ms": round(ph[2], 1)})
            rc, layout = ffi.groth16_key_layout(data, form)
            assert rc == 0 and int(layout[15]) == vk.shape[0] + rows.shape[0]
            P = 96 if form == 0 else 192
            assert data[:P] == ecc.ser_point(ecc.E1_761, bs.rows_to_points(g1[:1])[0], compressed=(form == 0))
            runs["form_%d" % form].append({"bytes": len(data)})
        res["key_write"] = {"points_per_query": n, "points": int(vk.shape[0] + rows.shape[0]), "row_bytes_in": int(rows.nbytes + vk.nbytes), "runs": runs}
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
