"""GPU (-m gpu): bulk decoding of compressed BLS12-377 points through the C ABI (include/celo_bls_amd.h:
decompress_bls12_377_g1 / _g2) vs the oracle's restatement of arkworks' GroupAffine::deserialize (oracle/py/ecc.py:
deser_point) - SURVEY.md section 8f row f2.

What it replaces: the per-key work of PublicKey::deserialize / Signature::deserialize (crates/bls-crypto/src/bls/
public.rs:123-149, signature.rs:31-57) and of the per-validator loop in crates/bls-snark-sys/src/snark/epoch_block.rs:187-196.
Pinned on the reference's own compressed points (crates/bls-crypto/src/hash_to_curve/mod.rs:412-513, committed in
tests/golden/reference_vectors.json): each decodes, lies in the subgroup and re-encodes to the same bytes.  Integer work:
bit-exact."""
import numpy as np
import pytest
import torch  # before the library: both must share one HIP runtime
from oracle.py import ecc
from oracle import cpu_oracle as co
from helpers import seeded_points

pytestmark = pytest.mark.gpu
Q = ecc.Q377


def _g1_rows(pts):
    return co.pack_g1_377(pts)[0]


def _g2_rows(pts):
    return co.pack_g2_377(pts)[0]


def test_reference_points_decode(gpu, golden):
    h = golden["hash_to_curve"]
    g1 = [bytes.fromhex(x) for k in ("g1_compat", "g1_noncompat") if k in h for x in h[k]["points"]]
    g2 = [bytes.fromhex(x) for x in h["g2_noncompat"]["points"]]
    assert len(g1) >= 20 and len(g2) >= 10
    xy, st = gpu.decompress("g1", b"".join(g1))
    assert st.tolist() == [0] * len(g1)
    want = [ecc.deser_point(ecc.E1_377, b, check_subgroup=True) for b in g1]
    assert np.array_equal(xy, _g1_rows(want))
    xy, st = gpu.decompress("g2", b"".join(g2))
    assert st.tolist() == [0] * len(g2)
    want = [ecc.deser_point(ecc.E2_377, b, check_subgroup=True) for b in g2]
    assert np.array_equal(xy, _g2_rows(want))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_random_points_round_trip(gpu, n):
    """encode (oracle) -> decode (GPU) gives the same affine coordinates, both signs of y, ragged launch sizes."""
    p1 = seeded_points(ecc.E1_377, ecc.G1_377, n, 31 + n)
    p1 = [P if i % 2 else ecc.E1_377.neg(P) for i, P in enumerate(p1)]
    xy, st = gpu.decompress("g1", b"".join(ecc.ser_point(ecc.E1_377, P) for P in p1))
    assert not st.any() and np.array_equal(xy, _g1_rows(p1))
    m = min(n, 96)
    p2 = seeded_points(ecc.E2_377, ecc.G2_377, m, 77 + n)
    p2 = [P if i % 2 else ecc.E2_377.neg(P) for i, P in enumerate(p2)]
    xy, st = gpu.decompress("g2", b"".join(ecc.ser_point(ecc.E2_377, P) for P in p2))
    assert not st.any() and np.array_equal(xy, _g2_rows(p2))


def _off_subgroup(curve, f2):
    """an on-curve point outside the prime-order subgroup (cofactor not cleared)"""
    x = 7
    while True:
        X = (x, 1) if f2 else x
        rhs = curve._add(curve._mul(curve._mul(X, X), X), curve.b)
        y = curve.f2.sqrt(rhs) if f2 else ecc.sqrt_fp(rhs, Q)
        if y is not None and not curve.in_subgroup((X, y)):
            return (X, y)
        x += 1


def _no_y(curve, f2):
    x = 5
    while True:
        X = (x, 3) if f2 else x
        rhs = curve._add(curve._mul(curve._mul(X, X), X), curve.b)
        y = curve.f2.sqrt(rhs) if f2 else ecc.sqrt_fp(rhs, Q)
        if y is None:
            return X
        x += 1


def test_status_codes_mixed_batch(gpu):
    """every verdict of GroupAffine::deserialize in ONE launch, neighbours unaffected: ok / infinity / x >= q / x not on the
    curve / on the curve but outside the subgroup (accepted when the check is off, as deserialize_unchecked would)."""
    good = seeded_points(ecc.E1_377, ecc.G1_377, 3, 5)
    off = _off_subgroup(ecc.E1_377, False)
    enc = [ecc.ser_point(ecc.E1_377, good[0]), ecc.ser_point(ecc.E1_377, None), Q.to_bytes(48, "little"),
           _no_y(ecc.E1_377, False).to_bytes(48, "little"), ecc.ser_point(ecc.E1_377, off), ecc.ser_point(ecc.E1_377, good[1]),
           ((1 << 382) - 1).to_bytes(48, "little"), ecc.ser_point(ecc.E1_377, good[2])]
    xy, st = gpu.decompress("g1", b"".join(enc))
    assert st.tolist() == [0, 1, 2, 2, 3, 0, 2, 0]
    assert np.array_equal(xy[[0, 5, 7]], _g1_rows(good)) and not xy[[1, 2, 3, 4, 6]].any()
    xy, st = gpu.decompress("g1", b"".join(enc), check_subgroup=False)
    assert st.tolist() == [0, 1, 2, 2, 0, 0, 2, 0] and np.array_equal(xy[4:5], _g1_rows([off]))

    good = seeded_points(ecc.E2_377, ecc.G2_377, 2, 6)
    off = _off_subgroup(ecc.E2_377, True)
    nx = _no_y(ecc.E2_377, True)
    enc = [ecc.ser_point(ecc.E2_377, good[0]), ecc.ser_point(ecc.E2_377, None), (1).to_bytes(48, "little") + Q.to_bytes(48, "little"),
           nx[0].to_bytes(48, "little") + nx[1].to_bytes(48, "little"), ecc.ser_point(ecc.E2_377, off), ecc.ser_point(ecc.E2_377, good[1])]
    xy, st = gpu.decompress("g2", b"".join(enc))
    assert st.tolist() == [0, 1, 2, 2, 3, 0]
    assert np.array_equal(xy[[0, 5]], _g2_rows(good)) and not xy[1:5].any()
    xy, st = gpu.decompress("g2", b"".join(enc), check_subgroup=False)
    assert st.tolist() == [0, 1, 2, 2, 0, 0] and np.array_equal(xy[4:5], _g2_rows([off]))


def test_empty_and_many_waves(gpu):
    """the empty call; 4120 G2 encodings (several waves per SIMD) decode like their 40 distinct sources"""
    xy, st = gpu.decompress("g2", b"")
    assert xy.shape == (0, 24) and st.shape == (0,)
    pts = seeded_points(ecc.E2_377, ecc.G2_377, 40, 9)
    enc = [ecc.ser_point(ecc.E2_377, P) for P in pts]
    big = enc * 103  # 4120 points: several waves per SIMD
    xy, st = gpu.decompress("g2", b"".join(big))
    assert not st.any()
    assert np.array_equal(xy, np.tile(_g2_rows(pts), (103, 1)))


@pytest.mark.parametrize("group,n", [("g1", 1 << 13), ("g2", 1 << 11)])
def test_bulk_matches_oracle_c(gpu, group, n):
    """thousands of distinct encodings with ~3 % spoiled ones (bit flips in x: most land off the curve, some on it but
    outside the subgroup) against the C restatement: same verdict and same coordinates for every entry."""
    curve, gen, size = (ecc.E1_377, ecc.G1_377, 48) if group == "g1" else (ecc.E2_377, ecc.G2_377, 96)
    base = seeded_points(curve, gen, 64, 1000 + n)
    rng = ecc.SplitMix64(n)
    enc = []
    P = base[0]
    for i in range(n):
        P = curve.add(P, base[rng.next() % 64])        # a walk through the subgroup: distinct points, cheap to make
        b = bytearray(ecc.ser_point(curve, P))
        r = rng.next()
        if r % 32 == 0:
            b[(r >> 8) % (size - 1)] ^= 1 << ((r >> 20) % 8)
        enc.append(bytes(b))
    data = b"".join(enc)
    xy, st = gpu.decompress(group, data)
    wxy, wst = co.decompress(group, data, threads=8)
    assert np.array_equal(st, wst) and np.array_equal(xy, wxy)
    assert 0 < int((st != 0).sum()) < n // 8


@pytest.mark.parametrize("group,n", [("g1", 1), ("g1", 7), ("g1", 8), ("g1", 9), ("g1", 1000), ("g2", 1), ("g2", 5), ("g2", 333)])
def test_batch_normalisation_matches_oracle(gpu, group, n):
    """normalize_bls12_377_g1/_g2 (Montgomery's trick inside a lane over 8 / 4 points) vs the oracle's restatement of
    batch_normalization_into_affine: random Jacobian representatives (x z^2, y z^3, z), identities (Z = 0) and already-affine
    points (Z = 1) mixed, ragged group sizes; and the affine values are the points we started from."""
    curve, gen, kind, words, pack = ((ecc.E1_377, ecc.G1_377, "g1_377", 6, co.pack_g1_377) if group == "g1"
                                     else (ecc.E2_377, ecc.G2_377, "g2_377", 12, co.pack_g2_377))
    rng = ecc.SplitMix64(4000 + n)
    base = seeded_points(curve, gen, 16, 17)
    q = ecc.Q377
    pts, rows = [], []
    P = base[0]
    for i in range(n):
        P = curve.add(P, base[rng.next() % 16])
        r = rng.next() % 8
        z = 1 if r == 0 else ecc.random_scalar(rng, q - 1) + 1
        if r == 1:
            pts.append(None)
            rows.append([rng.next(), rng.next(), 0] if group == "g1" else [rng.next(), 1, rng.next(), 2, 0, 0])   # arbitrary X, Y with Z = 0
            continue
        pts.append(P)
        if group == "g1":
            rows.append([P[0] * z * z % q, P[1] * z * z * z % q, z])
        else:
            f2 = ecc.F2_377
            zz = (z, 0)
            z2 = f2.mul(zz, zz)
            X, Y = f2.mul(P[0], z2), f2.mul(P[1], f2.mul(z2, zz))
            rows.append([X[0], X[1], Y[0], Y[1], z, 0])
    jac = co.to_mont([v for r in rows for v in r], q).reshape(n, 3 * words)
    xy, inf = gpu.normalize(group, jac)
    wxy, winf = co.normalize(kind, jac)
    assert np.array_equal(inf, winf) and np.array_equal(xy, wxy)
    exy, einf = pack(pts)
    exy[einf != 0] = 0
    assert np.array_equal(inf, einf) and np.array_equal(xy, exy)


def test_flag_byte_0xc0_is_no_encoding(gpu):
    """The top two bits of the last byte are (0x80: y is the larger root, 0x40: infinity).  Both set - 0xC0 - is REJECTED (status 2), for
    G1 and G2, whatever the x bits hold, on the GPU and in the oracle (VERDICT r3 item 9 asked for the case with its rationale):
    * ark-serialize 0.1 at the pinned revision (arkworks-rs/algebra#8d76d181, Cargo.lock:251-253) decodes the flags with
      SWFlags::from_u8, whose match has arms for 0x00 / 0x80 (the two signs) and 0x40 (infinity) and returns None for both bits set;
      GroupAffine::deserialize maps None to SerializationError::UnexpectedFlags, PublicKey::deserialize / Signature::deserialize
      (crates/bls-crypto/src/bls/public.rs:123-149, signature.rs:31-57) hand the error on, the FFI returns false;
    * the reference's own serialiser never emits it: infinity is written as the single flag 0x40 over an all-zero x (what
      test_status_codes_mixed_batch pins), so accepting 0xC0 would admit a SECOND encoding of the identity - malleable wire data in a
      consensus rule.  The source of that revision is not on disk, so this is the documented behaviour of the
      pinned crate, not a vector the reference holds; the choice is the conservative one either way: reject."""
    for group, size, words in (("g1", 48, 12), ("g2", 96, 24)):
        zero_c0 = bytes(size - 1) + b"\xC0"                       # the identity's x with both flags
        cur, gen = (ecc.E1_377, ecc.G1_377) if group == "g1" else (ecc.E2_377, ecc.G2_377)
        good = ecc.ser_point(cur, cur.mul(gen, 77))
        both = good[:-1] + bytes([good[-1] | 0xC0])               # a valid x with both flags
        data = zero_c0 + both + good
        xy, st = gpu.decompress(group, data, check_subgroup=True)
        wxy, wst = co.decompress(group, data, True)
        assert st.tolist() == [2, 2, 0] and wst.tolist() == [2, 2, 0]
        assert np.array_equal(xy, wxy) and not xy[:2].any()


@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("group", ["g1", "g2"])
def test_host_and_device_forms_return_the_same_bytes(gpu, group, n):
    """n = 1 and one row past a 64-lane workgroup, the last encoding spoiled: decompress_* and decompress_*_dev agree on rows and statuses; a
    refused device call (no output pointer) writes nothing, and the call after it is a normal one"""
    import ctypes as C
    curve, gen, size, words = (ecc.E1_377, ecc.G1_377, 48, 12) if group == "g1" else (ecc.E2_377, ecc.G2_377, 96, 24)
    enc = [ecc.ser_point(curve, P) for P in seeded_points(curve, gen, min(n, 5), 900 + n)]
    enc = [enc[i % len(enc)] for i in range(n)]
    enc[-1] = bytes([enc[-1][0] ^ 1]) + enc[-1][1:]
    data = b"".join(enc)
    xy, st = gpu.decompress(group, data)
    assert st[:-1].tolist() == [0] * (n - 1) and xy[:-1].any(axis=1).all()

    def dev_call(with_out):
        d_in = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
        d_out = torch.full((n * words,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
        d_st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc = getattr(gpu.lib(), "decompress_bls12_377_%s_dev" % group)(C.c_void_p(d_in.data_ptr()), C.c_size_t(n), C.c_int(1),
                                                                      C.c_void_p(d_out.data_ptr() if with_out else 0), C.c_void_p(d_st.data_ptr()), C.c_void_p(0))
        torch.cuda.synchronize()
        return rc, d_out.cpu().numpy().view(np.uint64).reshape(n, words), d_st.cpu().numpy()
    rc, out, dst = dev_call(False)
    assert rc == 2 and (out == 0x5A5A5A5A).all() and (dst == 0xEE).all()
    rc, out, dst = dev_call(True)
    assert rc == 0 and np.array_equal(out, xy) and np.array_equal(dst, st)
