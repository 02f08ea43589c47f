"""CPU (-m "not gpu"): pins the oracle on the reference's own golden vectors and
cross-checks its three layers (Python big-int  <->  C++ arkworks-style restatement)."""
import numpy as np
import pytest
from oracle.py import ecc, pairing as pp, epoch as ep
from oracle import cpu_oracle as co
from tests import helpers as H


def test_constants_and_generators():
    assert ecc.E1_377.on_curve(ecc.G1_377) and ecc.E1_377.mul(ecc.G1_377, ecc.R377) is None
    assert ecc.E2_377.on_curve(ecc.G2_377) and ecc.E2_377.mul(ecc.G2_377, ecc.R377) is None


@pytest.mark.parametrize("key", ["g1_compat", "g1_compat_cip22", "g1_noncompat", "g2_noncompat"])
def test_reference_hash_vectors_decode(golden, key):
    """crates/bls-crypto/src/hash_to_curve/mod.rs:412-513: every expected hash is a valid compressed
    point of the r-torsion and re-encodes to the same bytes (pins moduli, curve b, twist b', sqrt, sign flag)."""
    cur = ecc.E2_377 if key.startswith("g2") else ecc.E1_377
    for hx in golden["hash_to_curve"][key]["points"]:
        b = bytes.fromhex(hx)
        P = ecc.deser_point(cur, b)
        assert cur.in_subgroup(P)
        assert ecc.ser_point(cur, P) == b


def test_reference_epoch_encodings(golden):
    """crates/epoch-snark/src/epoch_block.rs:243-320 (pins the G2 generator and the y-sign convention)."""
    e = golden["epoch_encoding"]
    pk10 = [ecc.G2_377] * 10
    f, g = bytes([255] * 16), bytes([254] * 16)
    assert ep.EpochBlock(120, 5, f, g, 3, 10, pk10).encode_first_epoch_to_bytes_cip22().hex() == e["EXPECTED_ENCODING_WITH_ENTROPY"]
    assert ep.EpochBlock(120, 5, None, None, 3, 10, pk10).encode_first_epoch_to_bytes_cip22().hex() == e["EXPECTED_ENCODING_WITHOUT_ENTROPY"]
    assert ep.EpochBlock(120, 10, None, None, 3, 10, pk10).encode_to_bytes().hex() == e["EXPECTED_ENCODING_BEFORE_DONUT"]
    assert ep.EpochBlock(120, 5, f, g, 3, 11, pk10).encode_first_epoch_to_bytes_cip22().hex() == e["EXPECTED_ENCODING_WITH_ENTROPY_PADDED"]


def test_reference_groth16_vector_accepts(golden):
    """crates/bls-snark-sys/src/snark/mod.rs:52-119 — the only end-to-end pairing known-answer vector:
    the C++ BW6-761 pairing restatement must ACCEPT it and REJECT any tampering."""
    vk, pr, inputs = H.groth16_setup(golden)
    for P in [vk["alpha_g1"], pr["a"], pr["c"]] + vk["gamma_abc_g1"]:
        assert ecc.E1_761.in_subgroup(P)
    for P in [vk["beta_g2"], vk["gamma_g2"], vk["delta_g2"], pr["b"]]:
        assert ecc.E2_761.in_subgroup(P)
    pairs = ep.groth16_pairs(vk, pr, inputs)
    g1, i1 = co.pack_761([p for p, _ in pairs])
    g2, i2 = co.pack_761([q for _, q in pairs])
    _, ok = co.pairing_product_761(g1, i1, g2, i2)
    assert ok
    bad = ep.groth16_pairs(vk, pr, [inputs[0] ^ 1, inputs[1]])
    g1b, _ = co.pack_761([p for p, _ in bad])
    _, ok = co.pairing_product_761(g1b, i1, g2, i2)
    assert not ok
    bad_pr = dict(pr, c=ecc.E1_761.add(pr["c"], pr["c"]))
    pairs = ep.groth16_pairs(vk, bad_pr, inputs)
    g1c, _ = co.pack_761([p for p, _ in pairs])
    _, ok = co.pairing_product_761(g1c, i1, g2, i2)
    assert not ok


def test_cpp_bw6_pairing_value_vs_python_textbook(golden):
    """C++ optimal-ate value == (Python flat-field optimal ate)^k, k = (R0(x)+q R1(x)) / ((q^2-q+1)/r)."""
    vk, _, _ = H.groth16_setup(golden)
    P, Q = vk["alpha_g1"], vk["beta_g2"]
    x, q, r = ecc.X, ecc.Q761, ecc.R761
    f1 = pp.miller_loop_761(P, Q, loop=x + 1)
    f2 = pp.miller_loop_761(P, Q, loop=x ** 3 - x ** 2 - x)
    F = pp.F6_761
    f = F.mul(f1, F.frob(f2, 1))
    tb = F.pow(f, (q ** 6 - 1) // r)
    R0 = -103 * x**7 + 70 * x**6 + 269 * x**5 - 197 * x**4 - 314 * x**3 - 73 * x**2 - 263 * x - 220
    R1 = 103 * x**9 - 276 * x**8 + 77 * x**7 + 492 * x**6 - 445 * x**5 - 65 * x**4 + 452 * x**3 - 181 * x**2 + 34 * x + 229
    h = (q * q - q + 1) // r
    assert (R0 + q * R1) % h == 0
    k = (R0 + q * R1) // h
    g1, i1 = co.pack_761([P])
    g2, i2 = co.pack_761([Q])
    gt, one = co.pairing_product_761(g1, i1, g2, i2)
    assert not one
    assert co.gt761_to_flat(gt) == F.pow(tb, k)


def test_cpp_msm_matches_definition():
    """Pippenger restatement == naive sum of scalar muls == Python, with edge scalars,
    an infinity base and a repeated base; 1 and several threads."""
    n = 70
    pts = H.seeded_points(ecc.E1_377, ecc.G1_377, n, 11)
    pts[9] = None
    pts[10] = pts[11]
    sc = H.seeded_scalars(n, 12, ecc.R377)
    exp = ecc.E1_377.msm(pts, sc)
    xy, inf = co.pack_g1_377(pts)
    s = H.scalars_np(sc, 4)
    for naive in (False, True):
        for th in (1, 3):
            assert co.jac_to_affine(co.msm("bls12_377_g1", xy, inf, s, threads=th, naive=naive), "g1_377") == exp
    pts2 = H.seeded_points(ecc.E2_377, ecc.G2_377, 33, 13)
    sc2 = H.seeded_scalars(33, 14, ecc.R377)
    xy2, inf2 = co.pack_g2_377(pts2)
    assert co.jac_to_affine(co.msm("bls12_377_g2", xy2, inf2, H.scalars_np(sc2, 4), threads=2), "g2_377") == ecc.E2_377.msm(pts2, sc2)


def test_cpp_msm_bw6(golden):
    vk, pr, _ = H.groth16_setup(golden)
    base_pts = [vk["alpha_g1"], pr["a"], pr["c"]] + vk["gamma_abc_g1"]
    rng = ecc.SplitMix64(3)
    pts = [ecc.E1_761.mul(base_pts[i % len(base_pts)], rng.next() | 1) for i in range(20)]
    sc = H.seeded_scalars(20, 15, ecc.R761)
    xy, inf = co.pack_761(pts)
    got = co.jac_to_affine(co.msm("bw6_761_g1", xy, inf, H.scalars_np(sc, 6), threads=2), "761")
    assert got == ecc.E1_761.msm(pts, sc)


def test_cpp_bls12_pairing_is_cube_of_textbook():
    """arkworks' BLS12 final exponentiation returns the cube of the reduced pairing."""
    rng = ecc.SplitMix64(21)
    P = ecc.E1_377.mul(ecc.G1_377, rng.next())
    Q = ecc.E2_377.mul(ecc.G2_377, rng.next())
    g1, i1 = co.pack_g1_377([P])
    g2, i2 = co.pack_g2_377([Q])
    gt, _ = co.pairing_product_377(g1, i1, g2, i2)
    tb = pp.pairing_377(P, Q)
    assert co.gt377_to_flat(gt) == pp.F12_377.pow(tb, 3)
    # miller loop then final exp separately == product_of_pairings
    ml = co.miller_loop_377(g1, i1, g2, i2)
    assert np.array_equal(co.final_exp_377(ml), gt)


def test_cpp_pairing_product_accept_reject():
    """sign -> verify shape of crates/bls-crypto/src/bls/public.rs:94-120: e(sig,-g2) * e(H,pk) == 1."""
    sk, h = 0x1234567890ABCDEF1234, 0xCAFEBABE
    Hm = ecc.E1_377.mul(ecc.G1_377, h)
    sig = ecc.E1_377.mul(Hm, sk)
    pk = ecc.E2_377.mul(ecc.G2_377, sk)
    g1, i1 = co.pack_g1_377([sig, Hm])
    g2, i2 = co.pack_g2_377([ecc.E2_377.neg(ecc.G2_377), pk])
    assert co.pairing_product_377(g1, i1, g2, i2)[1]
    g2b, _ = co.pack_g2_377([ecc.E2_377.neg(ecc.G2_377), ecc.E2_377.mul(ecc.G2_377, sk + 1)])
    assert not co.pairing_product_377(g1, i1, g2b, i2)[1]
    # pairs with a point at infinity are skipped (ark-ec bls12 miller_loop)
    g1c, i1c = co.pack_g1_377([sig, Hm, None])
    g2c, i2c = co.pack_g2_377([ecc.E2_377.neg(ecc.G2_377), pk, pk])
    assert co.pairing_product_377(g1c, i1c, g2c, i2c)[1]


def test_reference_direct_hasher_vectors(golden):
    """crates/bls-crypto/src/hashers/direct.rs:88-96 (CRH of the empty message) and :149-172 (three BLAKE2X vectors):
    pins the hand-rolled Blake2s parameter block and the node-offset XOF construction."""
    from oracle.py import hashing as hs
    import hashlib
    d = golden["direct_hasher"]
    assert hs.direct_crh(b"", b"", 96).hex() == d["crh_empty_xof96"]
    assert len(d["blake2x_hash_vectors"]) == 3
    for v in d["blake2x_hash_vectors"]:
        assert hs.direct_hash(b"", bytes.fromhex(v["input"]), len(v["output"]) // 2).hex() == v["output"]
    for msg in (b"", b"abc", bytes(range(200))):
        assert hs.blake2s(msg) == hashlib.blake2s(msg).digest()
        assert hs.blake2s(msg, personal=b"ULforxof", digest_length=20) == hashlib.blake2s(msg, person=b"ULforxof", digest_size=20).digest()


def _xorshift_bytes(seed0, n):
    from oracle.py import composite as comp
    rng = comp.XorShiftRng(bytes([seed0]) + XORSHIFT_SEED_TAIL)
    return bytes(rng.gen_u8() for _ in range(n))


XORSHIFT_SEED_TAIL = bytes([0xbe, 0x62, 0x59, 0x8d, 0x31, 0x3d, 0x76, 0x32, 0x37, 0xdb, 0x17, 0xe5, 0xbc, 0x06, 0x54])


def test_reference_composite_hasher_vectors(golden):
    """crates/bls-crypto/src/hashers/composite.rs:105-190: Bowe-Hopwood CRH of the empty and of a XorShift-seeded message,
    then the Blake2Xs XOF at 96 / 768 / 769 bytes (pins ChaCha20Rng, Fq::rand, the Edwards generators and the chunk encoding)."""
    from oracle.py import composite as comp, hashing as hs
    for name, v in golden["composite_hasher"].items():
        msg = _xorshift_bytes(v["seed0"], v["msg_len"]) if v["seed0"] is not None else b""
        if name == "test_hash_random":
            continue  # 4910-byte message: covered through the C ABI (tests/test_seam_a.py); too slow for the Python oracle
        c = comp.composite_crh(msg)
        got = c if v["out_bytes"] is None else hs.direct_xof(b"ULforxof", c, v["out_bytes"])
        assert got.hex() == v["expected"], name


def reference_hash_test_inputs(n):
    """hash_to_curve/mod.rs:215-234 generate_test_data under XorShiftRng::from_seed(RNG_SEED): (domain, msg, extra) triples."""
    from oracle.py import composite as comp
    rng = comp.XorShiftRng(bytes([0x5d]) + XORSHIFT_SEED_TAIL)
    out = []
    for _ in range(n):
        msg = bytes(rng.gen_u8() for _ in range(rng.gen_u8()))
        dom = bytes(rng.gen_u8() for _ in range(8))
        extra = bytes(rng.gen_u8() for _ in range(rng.gen_u8()))
        out.append((dom, msg, extra))
    return out


@pytest.mark.parametrize("key,cip22", [("g1_compat", False), ("g1_compat_cip22", True)])
def test_reference_composite_hash_to_g1_vectors(golden, key, cip22):
    """hash_to_curve/mod.rs:412-455: the deployed (compat) try-and-increment over the composite hasher, before and after Donut."""
    from oracle.py import hashing as hs
    pts = golden["hash_to_curve"][key]["points"]
    for (dom, msg, extra), hx in zip(reference_hash_test_inputs(len(pts)), pts):
        P, _ = hs.hash_to_g1(dom, msg, extra, composite=True, cip22=cip22)
        assert ecc.ser_point(ecc.E1_377, P).hex() == hx


@pytest.mark.parametrize("log_n", [1, 3, 6])
def test_oracle_ntt_restatement_matches_definition(log_n):
    """oracle/cpu orc_ntt_fq377 (decimation in time, the checker of tests/test_ntt_gpu.py) against the O(n^2) definition of the
    transform (oracle/py/ntt.py), forward / inverse / coset variants.  The reference holds no NTT vector (parity unpinned there)."""
    from oracle.py import ntt as ontt
    from oracle import cpu_oracle as co
    Q = ecc.Q377
    rng = ecc.SplitMix64(5 + log_n)
    n, w = 1 << log_n, ontt.root_of_unity(log_n)
    assert pow(w, n, Q) == 1 and pow(w, n // 2, Q) == Q - 1
    x = [ecc.random_scalar(rng, Q) for _ in range(n)]
    X = co.from_mont(co.ntt_fq377(co.to_mont(x, Q), log_n, w), Q)
    assert X == ontt.dft(x, w)
    back = co.from_mont(co.ntt_fq377(co.to_mont(X, Q), log_n, pow(w, -1, Q), scale=pow(n, -1, Q)), Q)
    assert back == x
    g = 7
    Xc = co.from_mont(co.ntt_fq377(co.to_mont(x, Q), log_n, w, coset=g), Q)
    assert Xc == ontt.dft([xi * pow(g, i, Q) % Q for i, xi in enumerate(x)], w)
    xb = co.from_mont(co.ntt_fq377(co.to_mont(Xc, Q), log_n, pow(w, -1, Q), coset=pow(g, -1, Q), coset_after=True, scale=pow(n, -1, Q)), Q)
    assert xb == x


def test_reference_direct_hasher_random_vectors(golden):
    """crates/bls-crypto/src/hashers/direct.rs:99-147: crh / xof / hash of XorShift-seeded messages (the remaining DirectHasher vectors)."""
    from oracle.py import hashing as hs
    for name, v in golden["direct_hasher_random"].items():
        msg = _xorshift_bytes(v["seed0"], v["msg_len"])
        if name == "test_crh_random":
            got = hs.direct_crh(b"", msg, 96)
        elif name == "test_xof_random_96":
            got = hs.direct_xof(b"ULforxof", hs.direct_crh(b"", msg, 96), 96)
        else:
            got = hs.direct_hash(b"ULforxof", msg, 96)
        assert got.hex() == v["expected"], name
    assert hs.hash_length(48) == 64 and hs.hash_length(96) == 96      # hash_to_curve/mod.rs:176 test_hash_length


def test_oracle_c_decompress_matches_python_and_reference_points(golden):
    """orc_decompress_bls12_377 (the full-size checker of tests/test_wire_gpu.py) against the Python restatement of arkworks'
    GroupAffine::deserialize on the reference's own compressed points (hash_to_curve/mod.rs:412-513) and on every failure
    verdict: infinity, x >= q, x with no y, a point outside the subgroup."""
    from oracle import cpu_oracle as co
    h = golden["hash_to_curve"]
    g1 = [bytes.fromhex(x) for k in ("g1_compat", "g1_noncompat", "g1_compat_cip22") for x in h[k]["points"]]
    g2 = [bytes.fromhex(x) for x in h["g2_noncompat"]["points"]]
    xy1, st = co.decompress("g1", b"".join(g1), threads=2)
    assert not st.any() and np.array_equal(xy1, co.pack_g1_377([ecc.deser_point(ecc.E1_377, b, check_subgroup=True) for b in g1])[0])
    xy, st = co.decompress("g2", b"".join(g2), threads=2)
    assert not st.any() and np.array_equal(xy, co.pack_g2_377([ecc.deser_point(ecc.E2_377, b, check_subgroup=True) for b in g2])[0])
    # re-encoding the decoded points gives the reference's bytes back
    for b, row in zip(g1, xy1):
        x, y = co.from_mont(row.reshape(2, 6), ecc.Q377)
        assert ecc.ser_point(ecc.E1_377, (x, y)) == b
    q = ecc.Q377
    x = 5
    while ecc.sqrt_fp((x ** 3 + 1) % q, q) is not None:
        x += 1
    xo = 7
    while True:
        yo = ecc.sqrt_fp((xo ** 3 + 1) % q, q)
        if yo is not None and not ecc.E1_377.in_subgroup((xo, yo)):
            break
        xo += 1
    enc = [ecc.ser_point(ecc.E1_377, None), q.to_bytes(48, "little"), x.to_bytes(48, "little"), ecc.ser_point(ecc.E1_377, (xo, yo)), g1[0]]
    xy, st = co.decompress("g1", b"".join(enc))
    assert st.tolist() == [1, 2, 2, 3, 0] and not xy[:4].any()
    xy, st = co.decompress("g1", b"".join(enc), check_subgroup=False)
    assert st.tolist() == [1, 2, 2, 0, 0] and co.from_mont(xy[3].reshape(2, 6), q) == [xo, yo]


# ---------------------------------------------------------------- frozen MSM results (tests/golden/msm_fixtures.json)
def _msm_fixture():
    import json, os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msm_fixtures.json")) as f:
        return json.load(f)


def _unhex(P, f2=False):
    if P is None:
        return None
    if f2:
        return ((int(P[0][0], 16), int(P[0][1], 16)), (int(P[1][0], 16), int(P[1][1], 16)))
    return (int(P[0], 16), int(P[1], 16))


def test_oracle_pippenger_reproduces_the_frozen_msm_fixtures():
    """the C++ restatement of arkworks' Pippenger (the full-size checker) against results frozen from the big-int definition
    (tests/golden/make_msm_fixtures.py): the reference itself holds no MSM vector."""
    from tests import helpers as H
    from oracle import cpu_oracle as co
    fx = _msm_fixture()
    for n, want in fx["g1"].items():
        n = int(n)
        pts = H.seeded_points(ecc.E1_377, ecc.G1_377, n, 100 + n)
        sc = H.seeded_scalars(n, 200 + n, ecc.R377)
        xy, inf = co.pack_g1_377(pts)
        assert co.jac_to_affine(co.msm("bls12_377_g1", xy, inf, H.scalars_np(sc, 4), threads=2), "g1_377") == _unhex(want), n
    for n, want in fx["g2"].items():
        n = int(n)
        pts = H.seeded_points(ecc.E2_377, ecc.G2_377, n, 100 + n)
        sc = H.seeded_scalars(n, 200 + n, ecc.R377)
        xy, inf = co.pack_g2_377(pts)
        assert co.jac_to_affine(co.msm("bls12_377_g2", xy, inf, H.scalars_np(sc, 4), threads=2), "g2_377") == _unhex(want, True), n
