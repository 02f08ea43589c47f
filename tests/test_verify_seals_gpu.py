"""GPU: verify_aggregated_seals_bls12_377 (csrc/unit_seals.hip: masked key sums -> signatures decoded on the device -> message hashes -> pairs
packed into the pairing engine -> products) on the cases of tests/seal_cases.py, whose verdicts tests/test_seal_cases.py proves on the CPU.
Seals are built with fixed_base_mul_bls12_377_g2 (the keys) and sign_batch_bls12_377 under the summed key; verdicts and statuses are checked
whole, in both modes.  NOT covered: keys outside G2 (a precondition), counter exhaustion (no findable input), more than one device."""
import ctypes as C
import functools
import numpy as np
import pytest
import torch  # before the library: both must share one HIP runtime
from oracle.py import ecc
from oracle import cpu_oracle as co
import seal_cases as sc

pytestmark = pytest.mark.gpu
NEG_G2 = co.pack_g2_377([ecc.E2_377.neg(ecc.G2_377)])[0][0]
KEY = np.arange(1, 9, dtype=np.uint32) * 0x9E3779B1


@functools.lru_cache(None)
def _batch(m, rotation, tag, per_seal_sets=False, classes=sc.CLASSES):
    return sc.Batch(m, 9, rotation, 100 * m + rotation, tag, per_seal_sets=per_seal_sets, classes=classes)


def _material(gpu, b, hash_mode=0):
    """(key rows, signatures) of a batch: built once and kept on the batch"""
    _MATERIAL = b.__dict__.setdefault("material", {})
    k = hash_mode
    if k not in _MATERIAL:
        pk, pinf = gpu.fixed_base_mul("bls12_377_g2", co.pack_g2_377([ecc.G2_377])[0][0], co.ints_to_limbs(b.sks, 4))
        assert not pinf.any()
        sig, att = gpu.sign_batch(co.ints_to_limbs(b.sign_key, 4), gpu.SIG_DOMAIN, b.sign_msg, [sc.EXTRA] * b.m, hash_mode)
        assert (att != 255).all()
        _MATERIAL[k] = (pk[b.key_rows()].copy(), b.signatures(sig))
    return _MATERIAL[k]


def _verify(gpu, b, mode, hash_mode=0, key=KEY, sigs=None, thresholds=True):
    pk, honest = _material(gpu, b, hash_mode)
    mins = np.array(b.min_signers, dtype=np.uint32) if thresholds else None
    return gpu.verify_aggregated_seals(pk, None, b.offsets(), b.bits(), mins, gpu.SIG_DOMAIN, b.msg, [sc.EXTRA] * b.m, honest if sigs is None else sigs, NEG_G2,
                                       hash_mode=hash_mode, mode=mode, key=key)


def _check(b, ok, st, want=None):
    want = b.status if want is None else want
    bad = [(lab, int(g), w) for lab, g, w in zip(b.label, st, want) if g != w]
    assert not bad, bad[:6]
    assert ok.tolist() == [1 if w == 0 else 0 for w in want]


@pytest.mark.parametrize("mode", [0, 1], ids=["each", "combined"])
@pytest.mark.parametrize("rotation", range(len(sc.CLASSES)))
def test_every_class_at_every_position_of_65_seals(gpu, rotation, mode):
    """the nine rotations put every class at every position; a batch with a bad product makes the combined check fall back"""
    b = _batch(65, rotation, "gpu")
    ok, st = _verify(gpu, b, mode)
    _check(b, ok, st)
    assert gpu.seals_last()["path"] == (2 if mode else 0)


@pytest.mark.parametrize("per_seal_sets", [False, True], ids=["shared", "per_seal"])
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 257])
def test_sizes_without_a_bad_product_take_the_combined_path(gpu, m, per_seal_sets):
    """valid seals among seals that never reach a product: accepted by one combined product under a fixed key, under OS randomness, and one by one"""
    b = _batch(m, 0, "sizes", per_seal_sets, sc.NO_BAD_PRODUCT)
    for mode, key, path in ((1, KEY, 1), (1, None, 1), (0, None, 0)):
        ok, st = _verify(gpu, b, mode, key=key)
        _check(b, ok, st)
        assert gpu.seals_last()["path"] == path
    rec = gpu.seals_last()
    assert rec["lanes"] in gpu.AGGREGATE_LANES and rec["ms"]["sums"] > 0 and rec["ms"]["count"] > 0 and rec["ms"]["wall"] > 0


def test_all_classes_with_per_seal_sets_and_without_thresholds(gpu):
    b = _batch(65, 3, "gpu", True)
    for mode in (0, 1):
        _check(b, *_verify(gpu, b, mode))
    # min_signers = NULL: the threshold classes are valid seals; zero signers stays refused
    want = [0 if "signer short" in lab else w for lab, w in zip(b.label, b.status)]
    for mode in (0, 1):
        _check(b, *_verify(gpu, b, mode, thresholds=False), want=want)


def test_a_fixed_key_reproduces_and_a_rejected_combination_reports_path_2(gpu):
    b = _batch(65, 0, "sizes", False, sc.NO_BAD_PRODUCT)
    first = _verify(gpu, b, 1)
    again = _verify(gpu, b, 1)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]) and gpu.seals_last()["path"] == 1


def test_cancelling_pair_is_rejected_by_the_combined_mode(gpu):
    """sig_1 + D and sig_2 - D: the two errors cancel in an unrandomised sum of the signatures; with random exponents the combined check
    fails, the call falls back and both are refused - and only they"""
    b = _batch(9, 0, "sizes", False, ("valid",))
    pk, honest = _material(gpu, b)
    pts = [ecc.deser_point(ecc.E1_377, honest[i].tobytes()) for i in range(3)]
    D = pts[2]
    E = ecc.E1_377
    sigs = honest.copy()
    sigs[0] = np.frombuffer(ecc.ser_point(E, E.add(pts[0], D)), dtype=np.uint8)
    sigs[1] = np.frombuffer(ecc.ser_point(E, E.add(pts[1], E.neg(D))), dtype=np.uint8)
    # the unrandomised sum passes: one product over all pairs with the tampered signatures
    hxy, _ = gpu.hash_to_g1_direct(gpu.SIG_DOMAIN, b.msg, [sc.EXTRA] * b.m)
    apk, ainf, _ = gpu.aggregate_by_bitmap("bls12_377_g2", pk, None, b.offsets(), b.bits())
    sxy, sst = gpu.decompress("g1", sigs.tobytes())
    assert not sst.any() and not ainf.any()
    g1 = np.concatenate([np.stack([sxy[i], hxy[i]]) for i in range(b.m)])
    g2 = np.concatenate([np.stack([NEG_G2, apk[i]]) for i in range(b.m)])
    assert gpu.pairing_product_is_one_batch(g1, None, g2, None, np.array([0, 2 * b.m], dtype=np.uint32)).tolist() == [1]
    want = [4, 4] + [0] * 7
    for mode in (1, 0):
        _check(b, *_verify(gpu, b, mode, sigs=sigs), want=want)
        assert gpu.seals_last()["path"] == (2 if mode else 0)
    ok, st = _verify(gpu, b, 1, sigs=sigs, key=None)
    _check(b, ok, st, want=want)


@pytest.mark.parametrize("hash_mode", [0, 2, 3])
def test_hash_modes(gpu, hash_mode):
    b = _batch(9, 2, "modes")
    for mode in (0, 1):
        _check(b, *_verify(gpu, b, mode, hash_mode=hash_mode))
    good = _batch(9, 0, "modes", False, sc.NO_BAD_PRODUCT)
    _check(good, *_verify(gpu, good, 1, hash_mode=hash_mode))
    assert gpu.seals_last()["path"] == 1
    if hash_mode:                                   # a signature made under another hasher is a bad product
        _, direct = _material(gpu, good, 0)
        want = [4 if w == 0 else w for w in good.status]
        _check(good, *_verify(gpu, good, 0, hash_mode=hash_mode, sigs=direct), want=want)


def test_an_identity_key_sum_follows_the_pairing_engine(gpu):
    """keys P and -P, both signing: apk is the identity with count 2, that pair contributes 1, so the product is e(sig, -g2) - one only for
    the identity signature"""
    g2 = co.pack_g2_377([ecc.G2_377])[0][0]
    k = 12345
    pk, _ = gpu.fixed_base_mul("bls12_377_g2", g2, co.ints_to_limbs([k, ecc.R377 - k], 4))
    sig, att = gpu.sign_batch(co.ints_to_limbs([0, 7], 4), gpu.SIG_DOMAIN, [b"m0", b"m1"], None, 0)
    ok, st = gpu.verify_aggregated_seals(pk, None, [0, 2], np.ones((2, 2), dtype=np.uint8), np.array([2, 2], dtype=np.uint32), gpu.SIG_DOMAIN, [b"m0", b"m1"], None, sig,
                                         NEG_G2, mode=0)
    assert st.tolist() == [0, 4] and ok.tolist() == [1, 0]


def test_a_handful_against_seam_a(gpu):
    """the independent path: Seam A aggregate_public_keys + verify_signature, one seal at a time on handles"""
    from celo_bls_snark_rs_amd import ffi
    lib = C.CDLL(ffi.LIB_PATH)
    for name in ("deserialize_public_key", "deserialize_signature", "aggregate_public_keys", "verify_signature", "destroy_public_key", "destroy_signature"):
        getattr(lib, name).restype = C.c_bool
    b = _batch(65, 5, "gpu")
    _, sigs = _material(gpu, b)
    ok, st = _verify(gpu, b, 0)
    handles = []
    for k in b.sks:
        h = C.c_void_p()
        enc = ecc.ser_point(ecc.E2_377, ecc.E2_377.mul(ecc.G2_377, k))
        assert lib.deserialize_public_key(enc, C.c_int(96), C.byref(h))
        handles.append(h)
    seen = set()
    for i in range(b.m):
        if st[i] not in (0, 4) or (int(st[i]), b.label[i].split(": ")[1]) in seen:
            continue                                 # one seal of each class that reaches a product
        seen.add((int(st[i]), b.label[i].split(": ")[1]))
        chosen = [handles[j] for j, x in enumerate(b.bitmap[i]) if x]
        arr = (C.c_void_p * len(chosen))(*[h.value for h in chosen])
        apk, s, verdict = C.c_void_p(), C.c_void_p(), C.c_bool(False)
        assert lib.aggregate_public_keys(arr, C.c_int(len(chosen)), C.byref(apk))
        assert lib.deserialize_signature(sigs[i].tobytes(), C.c_int(48), C.byref(s))
        assert lib.verify_signature(apk, b.msg[i], C.c_int(len(b.msg[i])), sc.EXTRA, C.c_int(len(sc.EXTRA)), s, C.c_bool(False), C.c_bool(False), C.byref(verdict))
        assert bool(verdict.value) == bool(ok[i]), b.label[i]
        assert lib.destroy_public_key(apk) and lib.destroy_signature(s)
    assert len(seen) >= 5
    for h in handles:
        assert lib.destroy_public_key(h)


def test_bls_helper(gpu):
    from celo_bls_snark_rs_amd import bls
    b = _batch(9, 1, "modes")
    _, sigs = _material(gpu, b)
    pks = [ecc.E2_377.mul(ecc.G2_377, k) for k in b.sks]
    ok, st = bls.verify_seals(pks, b.bitmap, b.msg, [sigs[i].tobytes() for i in range(b.m)], extras=[sc.EXTRA] * b.m, min_signers=b.min_signers, combined=True)
    assert st == b.status and ok == [w == 0 for w in b.status]


def test_refused_arguments_leave_the_outputs_untouched(gpu):
    b = _batch(9, 0, "modes")
    pk, sigs = _material(gpu, b)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    data = np.frombuffer(b"".join(b.msg), dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum([len(x) for x in b.msg])]).astype(np.uint64)
    dom = np.frombuffer(gpu.SIG_DOMAIN, dtype=np.uint8)
    base = dict(pk=pk, offsets=b.offsets(), n_sets=1, bits=b.bits(), dom=dom, msgs=data, moff=off, hash_mode=0, sig=sigs, ng2=NEG_G2, m=b.m, mode=0, out=True)
    cases = [("pk NULL", dict(pk=None)), ("offsets NULL", dict(offsets=None)), ("bits NULL", dict(bits=None)), ("domain NULL", dict(dom=None)), ("msgs NULL", dict(msgs=None)),
             ("msg_off NULL", dict(moff=None)), ("sig NULL", dict(sig=None)), ("neg_g2 NULL", dict(ng2=None)), ("out_ok NULL", dict(out=False)),
             ("hash mode 1", dict(hash_mode=1)), ("hash mode 4", dict(hash_mode=4)), ("mode 2", dict(mode=2)), ("mode -1", dict(mode=-1)), ("two sets", dict(n_sets=2)),
             ("decreasing offsets", dict(offsets=np.array([9, 0], dtype=np.uint32))), ("m above 2^24", dict(m=(1 << 24) + 1))]
    for label, change in cases:
        a = dict(base, **change)
        ok = np.full(b.m, 9, dtype=np.uint8)
        st = np.full(b.m, 9, dtype=np.uint8)
        rc = gpu.lib().verify_aggregated_seals_bls12_377(p(a["pk"]), None, p(a["offsets"]), C.c_size_t(a["n_sets"]), p(a["bits"]), None, p(a["dom"]), p(a["msgs"]), p(a["moff"]),
                                                         None, None, C.c_int(a["hash_mode"]), p(a["sig"]), p(a["ng2"]), C.c_size_t(a["m"]), C.c_int(a["mode"]), None,
                                                         p(ok) if a["out"] else None, p(st))
        assert rc == 2, label
        assert (ok == 9).all() and (st == 9).all(), label
