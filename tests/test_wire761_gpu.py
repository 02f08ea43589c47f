"""GPU: bulk decoding of serialized BW6-761 points (decompress_bw6_761_*, decode_uncompressed_bw6_761_*; csrc/unit_wire761.hip) against the
oracle (oracle/py/ecc.deser_point, co.pack_761), bit for bit: the reference's VK and proof points, random curve points outside the subgroup,
malformed encodings in all three forms, and a 2^18 batch of subgroup points with every 97th row spoiled, through the host and _dev entries."""
import numpy as np
import pytest
import torch  # before the library: both must share one HIP runtime
from oracle.py import ecc
from oracle import cpu_oracle as co
import bw6_serial as bs

pytestmark = pytest.mark.gpu
Q = ecc.Q761


def run(gpu, curve, data, form):
    group = "bw6_761_g2" if curve is ecc.E2_761 else "bw6_761_g1"
    if form == 0:
        return gpu.decompress(group, data, check_subgroup=True)
    return gpu.decode_uncompressed(group, data, check=(form == 1))


def oracle_rows(curve, encs, form):
    sts, rows = [], []
    for e in encs:
        st, P = bs.oracle_status(curve, e, form == 0, form != 2)
        if form == 2 and st == 2 and int.from_bytes(e[:96], "little") < Q and e[-1] & 0xC0 == 0 and \
                int.from_bytes(e[96:], "little") < Q:
            st, P = 0, (int.from_bytes(e[:96], "little"), int.from_bytes(e[96:], "little"))   # deserialize_unchecked: no curve equation
        sts.append(st)
        rows.append(co.pack_761([P])[0][0] if st == 0 else np.zeros(24, dtype=np.uint64))
    return np.array(sts, dtype=np.uint8), np.array(rows, dtype=np.uint64).reshape(-1, 24)


@pytest.mark.parametrize("curve", [ecc.E1_761, ecc.E2_761], ids=["g1", "g2"])
def test_cases_match_oracle(gpu, curve):
    ref = [ecc.deser_point(c, d) for c, d in bs.reference_points() if c is curve]
    rnd = bs.random_curve_points(curve, 32, 5 + (curve is ecc.E2_761))
    P = rnd[0]
    for form in (0, 1, 2):
        encs = [bs.ser(curve, X, form) for X in ref + rnd + [None]]
        both = bytearray(bs.ser(curve, P, form)); both[-1] |= 0xC0
        big = bytearray(bs.ser(curve, P, form)); big[0:96] = (Q + 7).to_bytes(96, "little")
        encs += [bytes(both), bytes(big)]
        if form == 0:
            encs.append(bs.non_residue_x(curve, 3).to_bytes(96, "little"))
        else:
            encs.append(P[0].to_bytes(96, "little") + ((P[1] + 1) % Q).to_bytes(96, "little"))   # off the curve
        xy, st = run(gpu, curve, b"".join(encs), form)
        want_st, want_xy = oracle_rows(curve, encs, form)
        assert np.array_equal(st, want_st) and np.array_equal(xy, want_xy), form
        assert (st[:len(ref)] == 0).all() and st[len(ref) + len(rnd)] == 1
        assert (st[len(ref):len(ref) + len(rnd)] == (0 if form == 2 else 3)).all()
        assert st[-1] == (0 if form == 2 else 2)


def test_reference_points_reencode(gpu):
    for curve, data in bs.reference_points():
        xy, st = run(gpu, curve, data, 0)
        assert st[0] == 0
        assert ecc.ser_point(curve, bs.rows_to_points(xy)[0]) == data


def _flip_y(curve, P):
    return (P[0], (-P[1]) % Q)


@pytest.mark.wall_clock(900)
@pytest.mark.parametrize("curve", [ecc.E1_761, ecc.E2_761], ids=["g1", "g2"])
def test_batch_2_18_with_spoiled_rows(gpu, curve):
    """2^18 subgroup points k_i G (G = the reference VK's alpha_g1 / beta_g2), serialized here, every 97th row spoiled in one of six ways."""
    n = 1 << 18
    group = "bw6_761_g2" if curve is ecc.E2_761 else "bw6_761_g1"
    G = ecc.deser_point(curve, bs.reference_points()[0 if curve is ecc.E1_761 else 1][1])
    d_pts = torch.empty(n * 24, dtype=torch.int64, device="cuda")
    gpu.gen_points_dev("bw6_761_g1", d_pts.data_ptr(), n, 97 + (curve is ecc.E2_761), co.pack_761([G])[0][0])
    rows = d_pts.cpu().numpy().view(np.uint64).reshape(n, 24)
    pts = bs.rows_to_points(rows)
    encs = [ecc.ser_point(curve, X) for X in pts]
    want_st = np.zeros(n, dtype=np.uint8)
    want_xy = rows.copy()
    outside = bs.random_curve_points(curve, 8, 11)
    x_nr = bs.non_residue_x(curve, 12)
    kinds = {}
    for j, i in enumerate(range(0, n, 97)):
        k = j % 6
        kinds[i] = k
        e = bytearray(encs[i])
        if k == 0:
            e[-1] |= 0xC0; want_st[i] = 2
        elif k == 1:
            e[-1] = (e[-1] & 0x3F) | 0x40; want_st[i] = 1
        elif k == 2:
            e[0:96] = (Q + i).to_bytes(96, "little"); e[95] |= encs[i][95] & 0x80; want_st[i] = 2
        elif k == 3:
            e[-1] ^= 0x80; want_xy[i] = co.pack_761([_flip_y(curve, pts[i])])[0][0]        # -P: still in the subgroup
        elif k == 4:
            e = bytearray(ecc.ser_point(curve, outside[j % 8])); want_st[i] = 3
        else:
            e = bytearray(x_nr.to_bytes(96, "little")); want_st[i] = 2
        encs[i] = bytes(e)
        if want_st[i]:
            want_xy[i] = 0
    data = b"".join(encs)
    xy, st = gpu.decompress(group, data, check_subgroup=True)
    assert np.array_equal(st, want_st)
    assert np.array_equal(xy, want_xy)
    # every decoded row is on the curve and re-encodes to its input
    ok = np.nonzero(st == 0)[0]
    dec = bs.rows_to_points(xy[ok])
    for i, P in zip(ok.tolist(), dec):
        assert curve.on_curve(P) and ecc.ser_point(curve, P) == encs[i]
    # the subgroup verdict against the oracle's r P == O on a sample of 256 rows (the spoiled-outside ones among them)
    unchecked, st_u = gpu.decompress(group, data, check_subgroup=False)
    sample = sorted(set([i for i in kinds if kinds[i] in (3, 4)][:64]) | set(i for i in range(1, n, n // 256) if kinds.get(i, 3) in (3, 4)))
    assert len(sample) >= 256
    for i in sample:
        assert st_u[i] == 0
        P = bs.rows_to_points(unchecked[i:i + 1])[0]
        assert (st[i] == 0) == curve.in_subgroup(P) and st[i] in (0, 3)
    # the device-pointer entry gives the same rows and statuses
    d_in = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    d_out = torch.zeros(n * 24, dtype=torch.int64, device="cuda")
    d_st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    gpu.decompress_dev(group, d_in.data_ptr(), n, d_out.data_ptr(), d_st.data_ptr(), check_subgroup=True)
    torch.cuda.synchronize()
    assert np.array_equal(d_st.cpu().numpy(), want_st)
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64).reshape(n, 24), want_xy)


@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("curve", [ecc.E1_761, ecc.E2_761], ids=["g1", "g2"])
def test_host_and_device_forms_return_the_same_bytes(gpu, curve, n):
    """n = 1 and one row past a 64-lane workgroup over the reference's points, the last encoding spoiled: decompress_bw6_761_* and its _dev
    form agree on rows and statuses; a refused device call (no output pointer) writes nothing, and the call after it is a normal one"""
    import ctypes as C
    group = "bw6_761_g2" if curve is ecc.E2_761 else "bw6_761_g1"
    ref = [d for c, d in bs.reference_points() if c is curve]
    enc = [ref[i % len(ref)] for i in range(n)]
    enc[-1] = (Q + 7).to_bytes(96, "little")
    data = b"".join(enc)
    xy, st = gpu.decompress(group, data, check_subgroup=True)
    assert st.tolist() == [0] * (n - 1) + [2] and xy[:-1].any(axis=1).all() and not xy[-1].any()

    def dev_call(with_out):
        d_in = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
        d_out = torch.full((n * 24,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
        d_st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc = getattr(gpu.lib(), "decompress_%s_dev" % group)(C.c_void_p(d_in.data_ptr()), C.c_size_t(n), C.c_int(1), C.c_void_p(d_out.data_ptr() if with_out else 0),
                                                            C.c_void_p(d_st.data_ptr()), C.c_void_p(0))
        torch.cuda.synchronize()
        return rc, d_out.cpu().numpy().view(np.uint64).reshape(n, 24), d_st.cpu().numpy()
    rc, out, dst = dev_call(False)
    assert rc == 2 and (out == 0x5A5A5A5A).all() and (dst == 0xEE).all()
    rc, out, dst = dev_call(True)
    assert rc == 0 and np.array_equal(out, xy) and np.array_equal(dst, st)
