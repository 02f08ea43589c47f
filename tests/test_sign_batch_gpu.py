"""GPU: sign_batch_bls12_377 (csrc/unit_varbase.hip: hash to G1 -> [sk] H on the subgroup path -> compressed signatures) byte for byte against
Seam A's sign_message / sign_pop, which hash and multiply one message at a time on the host - an independent path - and end to end through
fixed_base_mul_bls12_377_g2 (the keys) and batch_verify_bls12_377."""
import ctypes as C
import random
import numpy as np
import pytest
import torch  # before the library: both must share one HIP runtime
from oracle.py import ecc
from oracle import cpu_oracle as co

pytestmark = pytest.mark.gpu
LENGTHS = (0, 1, 32, 200)


@pytest.fixture(scope="module")
def sys_lib():
    from celo_bls_snark_rs_amd import ffi
    lib = C.CDLL(ffi.LIB_PATH)
    for name in ("deserialize_private_key", "serialize_signature", "sign_message", "sign_pop", "free_vec", "destroy_signature", "destroy_private_key"):
        getattr(lib, name).restype = C.c_bool
    return lib


def _keys(n, seed):
    rng = random.Random(seed)
    ks = [rng.randrange(1, ecc.R377) for _ in range(n)]
    if n >= 3:
        ks[1], ks[2] = 1, ecc.R377 - 1
    return ks


def _messages(n, seed):
    rng = random.Random(seed)
    msgs = [rng.randbytes(LENGTHS[i % 4]) for i in range(n)]
    extras = [rng.randbytes((0, 1, 7, 40)[(i // 4) % 4]) for i in range(n)]
    return msgs, extras


def _seam_a(sys_lib, keys, msgs, extras, mode, pop):
    """one sign_message / sign_pop per message; keys: one for all, or one per message"""
    out = []
    handles = []
    for k in keys:
        h = C.c_void_p()
        assert sys_lib.deserialize_private_key(k.to_bytes(32, "little"), C.c_int(32), C.byref(h))
        handles.append(h)
    for i, m in enumerate(msgs):
        h, s = handles[0 if len(keys) == 1 else i], C.c_void_p()
        if pop:
            assert sys_lib.sign_pop(h, m, C.c_int(len(m)), C.byref(s))
        else:
            e = extras[i] if extras is not None else b""
            assert sys_lib.sign_message(h, m, C.c_int(len(m)), e, C.c_int(len(e)), C.c_bool(mode != 0), C.c_bool(mode == 3), C.byref(s))
        ptr, n = C.c_void_p(), C.c_int()
        assert sys_lib.serialize_signature(s, C.byref(ptr), C.byref(n)) and n.value == 48
        out.append(bytes(C.cast(ptr, C.POINTER(C.c_ubyte * 48)).contents))
        assert sys_lib.free_vec(ptr, n) and sys_lib.destroy_signature(s)
    for h in handles:
        assert sys_lib.destroy_private_key(h)
    return out


# mode 2 hashes ~25 ms per message on the host side of the comparison: its batches stop at 65
@pytest.mark.parametrize("mode,n", [(0, 1), (0, 65), (0, 257), (2, 1), (2, 65), (3, 1), (3, 65), (3, 257)])
@pytest.mark.parametrize("one_key", [True, False], ids=["one_key", "n_keys"])
def test_signatures_match_seam_a_byte_for_byte(gpu, sys_lib, mode, n, one_key):
    keys = _keys(1 if one_key else n, 10 * n + mode)
    msgs, extras = _messages(n, n + mode)
    sk = co.ints_to_limbs(keys, 4)
    for ex in (extras, None):
        sig, att = gpu.sign_batch(sk, gpu.SIG_DOMAIN, msgs, ex, mode)
        assert (att != 255).all()
        assert [sig[i].tobytes() for i in range(n)] == _seam_a(sys_lib, keys, msgs, ex, mode, False)
    if mode == 0:                                                    # sign_pop: POP_DOMAIN, the direct hasher, no extra data
        sig, att = gpu.sign_batch(sk, gpu.POP_DOMAIN, msgs, None, 0)
        assert [sig[i].tobytes() for i in range(n)] == _seam_a(sys_lib, keys, msgs, None, 0, True)


def test_pop_domain_with_extra_data_against_the_python_oracle(gpu):
    """sign_pop takes no extra data, so Seam A has no counterpart for this combination: three messages against oracle/py"""
    from oracle.py import hashing as hs
    keys = _keys(3, 77)
    msgs, extras = [b"", b"a", b"proof of possession"], [b"x", b"", b"extra"]
    sig, att = gpu.sign_batch(co.ints_to_limbs(keys, 4), gpu.POP_DOMAIN, msgs, extras, 0)
    for i in range(3):
        H, c = hs.hash_to_g1_direct(b"ULforpop", msgs[i], extras[i])
        assert att[i] == c and sig[i].tobytes() == ecc.ser_point(ecc.E1_377, ecc.E1_377.mul(H, keys[i]))


def test_bls_helper_and_zero_key(gpu, sys_lib):
    from celo_bls_snark_rs_amd import bls
    msgs, extras = _messages(9, 3)
    k = _keys(1, 5)[0]
    assert bls.sign_batch(k, msgs, extras) == _seam_a(sys_lib, [k], msgs, extras, 0, False)
    assert bls.sign_batch([k] * 9, msgs, pop=True) == _seam_a(sys_lib, [k], msgs, None, 0, True)
    assert bls.sign_batch(k, msgs, extras, composite=True, cip22=True) == _seam_a(sys_lib, [k], msgs, extras, 3, False)
    # the zero key is canonical: every signature is the identity, as serialize_signature writes it
    ident = ecc.ser_point(ecc.E1_377, None)
    assert bls.sign_batch(0, msgs) == [ident] * 9


def test_refused_arguments_leave_the_outputs_untouched(gpu):
    lib = gpu.lib()
    msgs = [b"a", b"bc", b""]
    data = np.frombuffer(b"abc", dtype=np.uint8)
    off = np.array([0, 1, 3, 3], dtype=np.uint64)
    dom = np.frombuffer(gpu.SIG_DOMAIN, dtype=np.uint8)
    sk = co.ints_to_limbs(_keys(3, 1), 4)
    at_r = co.ints_to_limbs([ecc.R377], 4)
    bad_last = sk.copy()
    bad_last[2] = at_r[0]
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    cases = [("sk NULL", None, 3, dom, data, off, 0, True, True), ("domain NULL", sk, 3, None, data, off, 0, True, True), ("msgs NULL", sk, 3, dom, None, off, 0, True, True),
             ("offsets NULL", sk, 3, dom, data, None, 0, True, True), ("sig NULL", sk, 3, dom, data, off, 0, False, True), ("attempts NULL", sk, 3, dom, data, off, 0, True, False),
             ("two keys for three", sk, 2, dom, data, off, 0, True, True), ("no key", sk, 0, dom, data, off, 0, True, True), ("key = r", bad_last, 3, dom, data, off, 0, True, True),
             ("one key = r", at_r, 1, dom, data, off, 0, True, True), ("mode 1", sk, 3, dom, data, off, 1, True, True), ("mode 4", sk, 3, dom, data, off, 4, True, True),
             ("mode -1", sk, 3, dom, data, off, -1, True, True)]
    for label, k, n_sk, d, m, o, mode, with_sig, with_att in cases:
        sig = np.full((3, 48), 0x5A, dtype=np.uint8)
        att = np.full(3, 9, dtype=np.uint8)
        rc = lib.sign_batch_bls12_377(p(k), C.c_size_t(n_sk), p(d), p(m), p(o), None, None, C.c_size_t(3), C.c_int(mode), p(sig) if with_sig else None,
                                      p(att) if with_att else None)
        assert rc == 2, label
        assert (sig == 0x5A).all() and (att == 9).all(), label
    assert lib.sign_batch_bls12_377(None, C.c_size_t(0), None, None, None, None, None, C.c_size_t(0), C.c_int(0), None, None) == 0
    sig, att = gpu.sign_batch(sk, gpu.SIG_DOMAIN, msgs)
    assert (att != 255).all() and sig.any()


def test_sign_then_verify_end_to_end(gpu):
    """sign_batch -> public keys by fixed_base_mul_bls12_377_g2 -> batch_verify_bls12_377 accepts every batch; with one signature swapped for
    its neighbour's in one batch, exactly that batch is rejected"""
    m, per = 5, 13
    keys = _keys(m * per, 99)
    msgs = [b"epoch %d" % j for j in range(m)]
    sk = co.ints_to_limbs(keys, 4)
    g2 = co.pack_g2_377([ecc.G2_377])[0][0]
    pk, pinf = gpu.fixed_base_mul("bls12_377_g2", g2, sk)
    assert not pinf.any()
    sig, att = gpu.sign_batch(sk, gpu.SIG_DOMAIN, [msgs[i // per] for i in range(m * per)], [b"\x01\x02"] * (m * per), 0)
    sxy, st = gpu.decompress("g1", sig.tobytes())
    assert not st.any()
    hxy, hatt = gpu.hash_to_g1_direct(gpu.SIG_DOMAIN, msgs, [b"\x01\x02"] * m)
    rng = random.Random(8)
    exps = co.ints_to_limbs([rng.getrandbits(128) | 1 for _ in range(m * per)], 4)
    offsets = np.arange(0, m * per + 1, per, dtype=np.uint32)
    neg_g2 = co.pack_g2_377([ecc.E2_377.neg(ecc.G2_377)])[0][0]
    assert gpu.batch_verify(pk, sxy, exps, offsets, hxy, neg_g2).tolist() == [1] * m
    bad = sig.copy()
    i = 2 * per + 4
    bad[i], bad[i + 1] = sig[i + 1], sig[i]                         # both still valid signatures - each under its neighbour's key
    bxy, st = gpu.decompress("g1", bad.tobytes())
    assert not st.any()
    assert gpu.batch_verify(pk, bxy, exps, offsets, hxy, neg_g2).tolist() == [1, 1, 0, 1, 1]


def test_cip22_signatures_are_the_three_steps_of_the_public_entries(gpu):
    """three messages in CIP22 mode: sign_batch == hash_to_g1_composite(cip22) -> scalar_mul_batch (subgroup entry) -> encode_points, byte for byte"""
    keys = _keys(3, 41)
    msgs, extras = _messages(3, 42)
    sk = co.ints_to_limbs(keys, 4)
    sig, att = gpu.sign_batch(sk, gpu.SIG_DOMAIN, msgs, extras, 3)
    hxy, hatt = gpu.hash_to_g1_composite(gpu.SIG_DOMAIN, msgs, extras, cip22=True)
    assert np.array_equal(att, hatt) and (hatt != 255).all()
    rows, inf = gpu.scalar_mul_batch("bls12_377_g1", hxy, None, sk, subgroup=True)
    enc, st = gpu.encode_points("g1", rows, inf, True)
    assert not st.any() and [sig[i].tobytes() for i in range(3)] == [enc[i].tobytes() for i in range(3)]
