"""GPU: epoch blocks to bytes, public inputs and verdicts on the device (csrc/unit_epoch.hip) against the oracle (oracle/py/epoch.py) on the
case list of tests/epoch_cases.py.  Expected bytes are computed once per distinct block; the batches repeat a small pool of blocks.

NOT covered here: more than one device; keys off the curve under keys_form = 1 (rows are trusted: the host twins take such rows through the
encoder, tests/test_epoch_host.py, but nothing sums them); the 2^24 / 65 536 limits beyond their refusal (tests/test_epoch_abi.py)."""
import ctypes as C
import threading
import numpy as np
import pytest
import torch  # noqa: F401  (before the library: torch brings its own HIP runtime; loaded after the library's, it finds no device)
import epoch_cases as EC
import groth16_verify_cases as gc
from oracle.py import ecc
from oracle.py import epoch as ep
from oracle.py import hashing as hs
from oracle import cpu_oracle as co

pytestmark = pytest.mark.gpu
KEY8 = np.arange(11, 19, dtype=np.uint32)
UNDECODABLE = bytes([1]) + bytes(95)          # x = 1: x^3 + B' is no square in Fq2
OUTSIDE_G2 = bytes([2]) + bytes(95)           # x = 2: on the twist, not in the subgroup of order r


def blocks(gpu, cases, **kw):
    return gpu.EpochBlocks(**EC.arrays(cases, **kw))


def test_the_two_spoiled_keys_are_what_they_claim():
    with pytest.raises(ValueError):
        ecc.deser_point(ecc.E2_377, UNDECODABLE)
    assert not ecc.E2_377.in_subgroup(ecc.deser_point(ecc.E2_377, OUTSIDE_G2))


def test_pool_keys_from_the_device(gpu):
    """the key pool, made on the device: (k + 2) G2 by the fixed-base ladder, compressed by the encoder - equal to the oracle's pool, so the
    oracle's expected bytes are about the keys the other tests feed"""
    n = 150
    gen = co.pack_g2_377([ecc.G2_377])[0][0]
    rows, inf = gpu.fixed_base_mul("bls12_377_g2", gen, co.ints_to_limbs([k + 2 for k in range(n)], 4))
    enc, st = gpu.encode_points("g2", rows, inf)
    assert not inf.any() and not st.any()
    assert enc.tobytes() == b"".join(EC.pool_bytes(k) for k in range(n))
    assert np.array_equal(rows, co.pack_g2_377([EC.pool_key(k) for k in range(n)])[0])


@pytest.mark.parametrize("keys_form", [0, 1])
def test_whole_outputs_byte_for_byte_in_all_four_kinds(gpu, keys_form):
    cases = EC.small_cases() + [c for k in EC.BORDER_K for c in EC.border_cases(k)]
    b = blocks(gpu, cases, keys_form=keys_form)
    for kind in EC.KINDS:
        data, extras, status, _ = gpu.epoch_encode_blocks(b, kind)
        assert not status.any(), kind
        for i, c in enumerate(cases):
            want, wextra = EC.expected(c, kind)
            assert data[i] == want, (kind, i, c.ident())
            assert extras is None or extras[i].tobytes() == wextra, (kind, i)
    nulls = EC.null_entropy_cases()
    bn = blocks(gpu, nulls, keys_form=keys_form, null_entropy=True)
    for kind in EC.KINDS:
        data, extras, status, _ = gpu.epoch_encode_blocks(bn, kind)
        assert [d for d in data] == [EC.expected(c, kind)[0] for c in nulls] and not status.any(), kind


def test_inner_form_at_its_border_lengths_and_a_full_set(gpu):
    cases = EC.border_cases("inner") + [EC.full_case(150), EC.full_case(110).with_(maxv=150)]
    data, extras, status, _ = gpu.epoch_encode_blocks(blocks(gpu, cases), "inner")
    assert [len(d) for d in data][:3] == list(EC.BORDER_LEN["inner"]) and not status.any()
    for i, c in enumerate(cases):
        assert (data[i], extras[i].tobytes()) == EC.expected(c, "inner"), i
    for kind in ("first", "last", "legacy"):
        data, _, status, _ = gpu.epoch_encode_blocks(blocks(gpu, cases[3:]), kind)
        assert data == [EC.expected(c, kind)[0] for c in cases[3:]] and not status.any(), kind


def test_a_spoiled_key_zero_fills_its_block_only(gpu):
    cases = [EC.Case(1, 1, EC.entropy(1), EC.entropy(2), 1, 5, [0, 1, 2]), EC.Case(2, 2, None, EC.entropy(3), 2, 0, [3, 4]), EC.Case(3, 3, EC.entropy(4), None, 3, 3, [5, 6, 7])]
    for raw in (UNDECODABLE, OUTSIDE_G2):
        for pos in ((0, 0), (1, 1), (2, 2)):
            b = blocks(gpu, cases, spoil={pos: raw})
            for kind in EC.KINDS:
                data, extras, status, _ = gpu.epoch_encode_blocks(b, kind)
                assert status.tolist() == [1 if i == pos[0] else 0 for i in range(3)], (pos, kind)
                for i, c in enumerate(cases):
                    want = EC.expected(c, kind)[0]
                    assert data[i] == (bytes(len(want)) if i == pos[0] else want), (pos, kind, i)


def test_blocks_without_any_key(gpu):
    """no key in the whole call: headers, padding and (last form) the identity as the aggregated key"""
    cases = [EC.small_cases()[13], EC.small_cases()[14], EC.Case(7, 7, EC.entropy(8), EC.entropy(9), 7, 2, [])]
    for keys_form in (0, 1):
        b = blocks(gpu, cases, keys_form=keys_form)
        for kind in EC.KINDS:
            data, extras, status, _ = gpu.epoch_encode_blocks(b, kind)
            assert data == [EC.expected(c, kind)[0] for c in cases] and not status.any(), (keys_form, kind)
        got, st = gpu.epoch_public_inputs(b, b)
        assert not st.any() and np.array_equal(got, EC.inputs_limbs([(c, c) for c in cases]))


def test_dev_form_equals_the_host_form(gpu):
    cases = EC.small_cases()
    for keys_form in (0, 1):
        a = EC.arrays(cases, keys_form=keys_form)
        host = gpu.EpochBlocks(**a)
        dev = gpu.EpochBlocks(**a)
        keep = {}
        for name, arr in (("keys", host.keys), ("keys_inf", host.inf), ("epoch_entropy", host.ee), ("parent_entropy", host.pe)):
            if arr is not None:
                keep[name] = torch.from_numpy(arr.copy()).cuda()
                setattr(dev.c, name, keep[name].data_ptr())
        for kind in range(4):
            data, extras, status, (flat, off) = gpu.epoch_encode_blocks(host, kind)
            d_out = torch.full((int(off[-1]) + 16,), 0x5A, dtype=torch.uint8, device="cuda")
            d_extras = torch.full((len(cases), 7), 0x5A, dtype=torch.uint8, device="cuda")
            d_status = torch.full((len(cases),), 9, dtype=torch.uint8, device="cuda")
            rc = gpu.epoch_encode_blocks_dev(dev.c, len(cases), kind, off, d_out.data_ptr(), d_extras.data_ptr(), d_status.data_ptr(), torch.cuda.current_stream().cuda_stream)
            assert rc == 0
            torch.cuda.synchronize()
            got = d_out.cpu().numpy()
            assert np.array_equal(got[:int(off[-1])], flat[:int(off[-1])]) and (got[int(off[-1]):] == 0x5A).all(), (keys_form, kind)
            assert np.array_equal(d_status.cpu().numpy(), status)
            assert np.array_equal(d_extras.cpu().numpy(), extras) if kind == 2 else (d_extras.cpu().numpy() == 0x5A).all()
        first, last = host, host
        want, wst = gpu.epoch_public_inputs(first, last)
        d_in = torch.zeros((len(cases), 12), dtype=torch.int64, device="cuda")
        d_st = torch.full((len(cases),), 9, dtype=torch.uint8, device="cuda")
        assert gpu.epoch_public_inputs_dev(dev.c, dev.c, len(cases), d_in.data_ptr(), d_st.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        assert np.array_equal(d_in.cpu().numpy().view(np.uint64).reshape(-1, 2, 6), want) and np.array_equal(d_st.cpu().numpy(), wst)


def pair_pool():
    """(first, last) block pairs: 0 .. 5 keys and a full set of 150, every Blake2s border length of both forms, the empty first block"""
    small = EC.small_cases()
    pairs = [(small[i], small[(i + 3) % 10]) for i in range(6)]
    pairs += list(zip(EC.border_cases("first"), EC.border_cases("last")))
    pairs += [(small[13], small[10]), (small[11], small[12]), (EC.full_case(150), EC.full_case(150).with_(index=4243, ee=EC.entropy(23)))]
    return pairs


def test_blake2s_borders_through_the_inputs(gpu):
    pairs = pair_pool()
    assert [len(EC.expected(f, "first")[0]) for f, _ in pairs[6:9]] == list(EC.BORDER_LEN["first"]) and len(EC.expected(pairs[9][0], "first")[0]) == 22
    assert [len(EC.expected(l, "last")[0]) for _, l in pairs[6:9]] == list(EC.BORDER_LEN["last"])
    got, st = gpu.epoch_public_inputs(blocks(gpu, [f for f, _ in pairs]), blocks(gpu, [l for _, l in pairs]))
    assert not st.any() and np.array_equal(got, EC.inputs_limbs(pairs))


@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 256, 257])
def test_inputs_against_the_oracle_with_spoiled_keys(gpu, m):
    pool = pair_pool()[:9]
    pairs = [pool[i % len(pool)] for i in range(m)]
    firsts, lasts = [f for f, _ in pairs], [l for _, l in pairs]
    got, st = gpu.epoch_public_inputs(blocks(gpu, firsts), blocks(gpu, lasts))
    want = EC.inputs_limbs(pool)[[i % len(pool) for i in range(m)]]
    assert not st.any() and np.array_equal(got, want)
    # one bad key at the first, a middle and the last position of a first or a last block: only that proof's status may change
    spots = sorted({0, m // 2, m - 1})
    for n, i in enumerate(spots):
        side, raw = n % 2, (UNDECODABLE, OUTSIDE_G2)[(n + m) % 2]
        if not any(c.keys for c in (firsts, lasts)[side]):
            side ^= 1
        cases = (firsts, lasts)[side]
        j = next(k for k in range(i, i + m) if cases[k % m].keys) % m          # the nearest proof whose block has a key to spoil
        nk = len(cases[j].keys)
        for kpos in sorted({0, nk // 2, nk - 1}):
            bf = blocks(gpu, firsts, spoil={(j, kpos): raw} if side == 0 else None)
            bl = blocks(gpu, lasts, spoil={(j, kpos): raw} if side == 1 else None)
            got, st = gpu.epoch_public_inputs(bf, bl)
            assert st.tolist() == [(1 + side) if k == j else 0 for k in range(m)], (m, j, side, kpos)
            clean = np.arange(m) != j
            assert np.array_equal(got[clean], want[clean])


# ---- verdicts
@pytest.fixture(scope="module")
def key2():
    return gc.Key(2, 0xE90C)


@pytest.fixture(scope="module")
def vk2(gpu, key2):
    vk = gpu.VerifyingKey(key2.alpha, key2.beta, key2.gamma, key2.delta, key2.abc)
    yield vk
    vk.release()


@pytest.fixture(scope="module")
def proof_pool(key2):
    """one valid proof per block pair (blocks of 0 .. 5 and 150 keys), serialized: a batch repeats them"""
    pairs = pair_pool()[:6] + [pair_pool()[-1]]
    rng = ecc.SplitMix64(0xE90C2)
    batch = gc.Batch(key2, [gc.valid_proof(key2, rng, x=EC.expected_inputs(f, l)) for f, l in pairs])
    ser = batch.serialize()
    return pairs, [ser[288 * i:288 * i + 288] for i in range(len(pairs))], batch


def _status_batch(pool, m, rotation):
    """m proofs; position p is of status class (p + rotation) % 5: 0 clean, 1 a spoiled first block, 2 a spoiled last block, 3 a proof point
    that is no encoding, 4 another pair's proof.  Returns (firsts, lasts, spoil_first, spoil_last, proof bytes, classes)."""
    pairs, sers, _ = pool
    usable = [i for i, (f, l) in enumerate(pairs) if f.keys and l.keys]
    firsts, lasts, sf, sl, proofs, classes = [], [], {}, {}, [], []
    for p in range(m):
        cls = (p + rotation) % 5
        i = usable[p % len(usable)]
        f, l = pairs[i]
        raw = sers[i]
        if cls == 1:
            sf[(p, len(f.keys) - 1)] = (UNDECODABLE, OUTSIDE_G2)[p % 2]
        elif cls == 2:
            sl[(p, 0)] = (OUTSIDE_G2, UNDECODABLE)[p % 2]
        elif cls == 3:
            raw = raw[:95] + bytes([raw[95] | 0xC0]) + raw[96:]             # A with both flags set: no encoding at all
        elif cls == 4:
            raw = sers[usable[(p + 1) % len(usable)]]
        firsts.append(f); lasts.append(l); proofs.append(raw); classes.append(cls)
    return firsts, lasts, sf, sl, b"".join(proofs), classes


def test_every_status_class_at_every_position_in_both_modes(gpu, vk2, proof_pool):
    m = 65
    for rotation in range(5):
        firsts, lasts, sf, sl, proofs, classes = _status_batch(proof_pool, m, rotation)
        bf, bl = blocks(gpu, firsts, spoil=sf), blocks(gpu, lasts, spoil=sl)
        for mode in (0, 1):
            ok, st = gpu.verify_epoch_proofs(vk2, proofs, bf, bl, mode=mode, key=KEY8)
            assert st.tolist() == classes, (rotation, mode)
            assert ok.tolist() == [1 if c == 0 else 0 for c in classes], (rotation, mode)
            assert gpu.groth16_verify_last()[0] == ("each", "combined then each")[mode]
    # all clean: the combination holds
    pairs, sers, _ = proof_pool
    idx = [i % len(pairs) for i in range(m)]
    bf, bl = blocks(gpu, [pairs[i][0] for i in idx]), blocks(gpu, [pairs[i][1] for i in idx])
    for mode, path in ((0, "each"), (1, "combined accepted")):
        ok, st = gpu.verify_epoch_proofs(vk2, b"".join(sers[i] for i in idx), bf, bl, mode=mode, key=(KEY8, None)[mode])
        assert ok.tolist() == [1] * m and not st.any() and gpu.groth16_verify_last()[0] == path
    ms = gpu.epoch_last()
    assert ms["wall"] > 0 and ms["decode"] > 0 and ms["verify"] > 0 and ms["hash"] > 0


def test_agrees_with_the_serialized_batch_verifier_fed_the_oracles_inputs(gpu, vk2, proof_pool):
    firsts, lasts, sf, sl, proofs, classes = _status_batch(proof_pool, 33, 2)
    x = EC.inputs_limbs(list(zip(firsts, lasts)))
    for mode in (0, 1):
        want = vk2.verify_serialized(proofs, x, mode=mode, key=KEY8)            # (it knows nothing of the blocks: classes 1 and 2 pass there)
        ok, st = gpu.verify_epoch_proofs(vk2, proofs, blocks(gpu, firsts, spoil=sf), blocks(gpu, lasts, spoil=sl), mode=mode, key=KEY8)
        assert want.tolist() == [1 if c in (0, 1, 2) else 0 for c in classes]
        assert ok.tolist() == [int(w) if c not in (1, 2) else 0 for w, c in zip(want, classes)]


def _reference(gpu, golden):
    g = golden["groth16_bw6_761"]
    return gpu.VerifyingKey.from_serialized(bytes.fromhex(g["vk"])), bytes.fromhex(g["proof"]), EC.reference_cases(golden)


def _flips(first, last):
    """(label, first fields, last fields): one byte flipped in an entropy, a key, index or maximum_non_signers"""
    flip = lambda b, i: b[:i] + bytes([b[i] ^ 1]) + b[i + 1:]
    # a key with one byte flipped need not decode: swap two keys instead where the block must stay decodable, and flip a byte for the status
    swap = lambda raw: raw[96:192] + raw[:96] + raw[192:]
    return [("untouched", {}, {}), ("first parent entropy", dict(pe=flip(first["pe"], 0)), {}), ("last epoch entropy", {}, dict(ee=flip(last["ee"], 15))),
            ("first index", dict(index=first["index"] ^ 1), {}), ("last index", {}, dict(index=last["index"] ^ 0x100)),
            ("first maximum_non_signers", dict(mns=first["mns"] ^ 1), {}), ("last maximum_non_signers", {}, dict(mns=last["mns"] ^ (1 << 24))),
            ("first keys swapped", dict(raw=swap(first["raw"])), {}), ("last key byte", {}, dict(raw=flip(last["raw"], 3)))]


def test_the_references_own_vector_accepts_and_every_flip_rejects(gpu, golden):
    vk, proof, (first, last) = _reference(gpu, golden)
    try:
        for label, cf, cl in _flips(first, last):
            bf, bl = gpu.EpochBlocks(**EC.reference_arrays(first, **cf)), gpu.EpochBlocks(**EC.reference_arrays(last, **cl))
            for mode in (0, 1):
                ok, st = gpu.verify_epoch_proofs(vk, proof, bf, bl, mode=mode, key=KEY8)
                if label == "untouched":
                    assert (ok.tolist(), st.tolist()) == ([1], [0]), mode
                elif label == "last key byte":
                    assert ok.tolist() == [0] and st.tolist()[0] in (2, 4), (label, mode)       # the flipped x decodes, or it does not
                else:
                    assert (ok.tolist(), st.tolist()) == ([0], [4]), (label, mode)
        # a last block without the aggregated key's owner: the untouched first block with the last block's fields is another statement
        ok, st = gpu.verify_epoch_proofs(vk, proof, gpu.EpochBlocks(**EC.reference_arrays(last)), gpu.EpochBlocks(**EC.reference_arrays(first)))
        assert (ok.tolist(), st.tolist()) == ([0], [4])
    finally:
        vk.release()


def test_a_handful_of_cases_against_seam_a_verify(gpu, golden):
    """the host-only `verify` of the reference's C ABI (csrc/seam_epoch.hip) on the same blocks: the same verdicts"""
    from celo_bls_snark_rs_amd import ffi

    class EpochBlockFFI(C.Structure):
        _fields_ = [("index", C.c_uint16), ("round", C.c_uint8), ("epoch_entropy", C.c_char_p), ("parent_entropy", C.c_char_p), ("pubkeys", C.c_char_p),
                    ("pubkeys_num", C.c_size_t), ("maximum_non_signers", C.c_uint32), ("maximum_validators", C.c_size_t)]
    lib = C.CDLL(ffi.LIB_PATH)
    lib.verify.restype = C.c_bool
    lib.verify.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, EpochBlockFFI, EpochBlockFFI]
    g = golden["groth16_bw6_761"]
    vk_bytes = bytes.fromhex(g["vk"])
    vk, proof, (first, last) = _reference(gpu, golden)
    seam = lambda s: EpochBlockFFI(s["index"], s["round"], s["ee"], s["pe"], s["raw"], len(s["raw"]) // 96, s["mns"], s["maxv"])
    ident = ecc.ser_point(ecc.E2_377, None)
    try:
        flips = _flips(first, last)
        handful = [flips[0], flips[2], flips[3], flips[7], ("an identity key in the last block", {}, dict(raw=ident + last["raw"][96:])),
                   ("an undecodable key in the first block", dict(raw=UNDECODABLE + first["raw"][96:]), {})]
        for label, cf, cl in handful:
            f, l = dict(first, **cf), dict(last, **cl)
            want = bool(lib.verify(vk_bytes, len(vk_bytes), proof, len(proof), seam(f), seam(l)))
            ok, st = gpu.verify_epoch_proofs(vk, proof, gpu.EpochBlocks(**EC.reference_arrays(f)), gpu.EpochBlocks(**EC.reference_arrays(l)))
            assert bool(ok[0]) == want == (label == "untouched"), label
        assert st.tolist() == [1]
    finally:
        vk.release()


def test_two_threads(gpu, vk2, proof_pool):
    firsts, lasts, sf, sl, proofs, classes = _status_batch(proof_pool, 20, 1)
    out, errs = {}, []

    def work(t):
        try:
            gpu.use_device(0)
            for _ in range(2):
                ok, st = gpu.verify_epoch_proofs(vk2, proofs, blocks(gpu, firsts, spoil=sf), blocks(gpu, lasts, spoil=sl), mode=t, key=KEY8)
                x, xs = gpu.epoch_public_inputs(blocks(gpu, firsts), blocks(gpu, lasts))
                out[t] = (ok.tolist(), st.tolist(), x, xs.tolist())
        except Exception as e:      # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=work, args=(t,)) for t in (0, 1)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    want_x = EC.inputs_limbs(list(zip(firsts, lasts)))
    for t in (0, 1):
        assert out[t][0] == [1 if c == 0 else 0 for c in classes] and out[t][1] == classes
        assert np.array_equal(out[t][2], want_x) and not any(out[t][3])


def test_kind_2_chained_into_the_composite_cip22_hash(gpu):
    """the inner form's msgs / extras, as the encoder lays them out, are what hash_to_g1_composite(cip22) reads: the message validators sign"""
    cases = [EC.Case(7, 3, EC.entropy(1), EC.entropy(2), 5, 1, [0]), EC.Case(EC.U16, EC.U8, None, EC.entropy(9), EC.U32, 0, [1, 2])]
    data, extras, status, _ = gpu.epoch_encode_blocks(blocks(gpu, cases), "inner")
    assert not status.any()
    xy, att = gpu.hash_to_g1_composite(b"ULforxof", data, [e.tobytes() for e in extras], cip22=True)
    want = [hs.hash_to_g1(b"ULforxof", *ep.encode_inner_to_bytes_cip22(c.block()), composite=True, cip22=True) for c in cases]
    assert np.array_equal(xy, co.pack_g1_377([P for P, _ in want])[0]) and att.tolist() == [c for _, c in want]
