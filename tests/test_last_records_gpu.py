"""GPU: what the celo_amd_*_last* getters report after a composed call (csrc/last_call.h) - the path and lane tags,
every slot >= 0 and the unused ones exactly 0, every stage time within the call's own wall time, the sub-calls' times handed up as the
sub-calls' own records hold them, and a refused call (code 2) leaving the record as it was.  The case builders are those of
test_verify_seals_gpu.py, test_transitions_gpu.py, test_epoch_gpu.py and test_sign_batch_gpu.py at their smallest shapes: 3 seals over one
shared set of 4 keys, one chain of 3 blocks of 4 validators, 2 epoch proofs, 4 signatures.  One test runs seals beside hashing and decoding
from a second thread: it guards the results and the record's coherence.  The values are checked elsewhere; nothing here is about speed."""
import ctypes as C
import threading
import numpy as np
import pytest
import torch  # noqa: F401  (before the library: both must share one HIP runtime)
from oracle.py import ecc
from oracle import cpu_oracle as co
import groth16_verify_cases as gc
import epoch_cases as EC
import seal_cases as sc
import test_epoch_gpu as TE
import test_sign_batch_gpu as TB
import test_transitions_gpu as TT
import test_verify_seals_gpu as TS

pytestmark = pytest.mark.gpu


def _seals(tag="records"):
    return sc.Batch(3, 4, 0, 777, tag, classes=("valid",))


def _whole(ms, wall, unused=()):
    """ms: the 8 (or 4) slots in order; every one >= 0, none above the wall slot, the unused ones exactly 0"""
    assert all(v >= 0 for v in ms), ms
    assert ms[wall] > 0 and all(v <= ms[wall] for v in ms), ms
    assert all(ms[i] == 0 for i in unused), ms


def _seals_record_ok(gpu, rec, path):
    ms = list(rec["ms"].values())
    assert rec["path"] == path and rec["lanes"] in gpu.AGGREGATE_LANES, rec
    _whole(ms, 6, unused=(3,) if path == 0 else ())
    assert ms[0] > 0 and ms[1] > 0 and ms[2] > 0 and ms[4] > 0 and ms[7] <= ms[0], ms
    if path == 1:
        assert ms[3] > 0, ms


def test_seals_record(gpu):
    b = _seals()
    for mode in (0, 1):
        ok, st = TS._verify(gpu, b, mode)
        assert ok.tolist() == [1, 1, 1] and not st.any()
        rec = gpu.seals_last()
        _seals_record_ok(gpu, rec, mode)
        # the handed-up times are the sub-calls' own (the combined mode normalises one point after the signatures' decoding: the decoder's
        # record then holds that call)
        assert rec["ms"]["hash"] == gpu.hash_last_ms()
        if mode == 0:
            assert rec["ms"]["decode"] == gpu.decompress_last_ms()
    # a refused call leaves the record as it was
    with pytest.raises(ValueError):
        TS._verify(gpu, b, 2)
    assert gpu.seals_last() == rec
    # a bare sum: path -1, the sums, their count kernel and the wall alone
    pk, _ = TS._material(gpu, b)
    gpu.aggregate_by_bitmap("bls12_377_g2", pk, None, b.offsets(), b.bits())
    bare = gpu.seals_last()
    ms = list(bare["ms"].values())
    assert bare["path"] == -1 and bare["lanes"] in gpu.AGGREGATE_LANES
    _whole(ms, 6, unused=(1, 2, 3, 4, 5))
    assert 0 < ms[7] <= ms[0]
    out, oinf, down = np.zeros((3, 24), dtype=np.uint64), np.zeros(3, dtype=np.uint8), np.array([4, 0], dtype=np.uint32)
    rows, bits = np.ascontiguousarray(pk), np.ascontiguousarray(b.bits())
    assert gpu.lib().aggregate_by_bitmap_bls12_377_g2(co._p(rows), None, co._p(down), C.c_size_t(1), co._p(bits), C.c_size_t(3), co._p(out), co._p(oinf), None) == 2
    assert gpu.seals_last() == bare


def test_sign_batch_record(gpu):
    keys, (msgs, extras) = TB._keys(4, 5), TB._messages(4, 5)
    sig, att = gpu.sign_batch(co.ints_to_limbs(keys, 4), gpu.SIG_DOMAIN, msgs, extras, 0)
    assert (att != 255).all() and sig.shape == (4, 48)
    assert gpu.hash_last_ms() > 0
    rec = gpu.scalar_mul_last_ms()
    ms = list(rec.values())
    _whole(ms, 3)
    assert ms[0] > 0 and ms[1] > 0 and ms[2] > 0
    with pytest.raises(ValueError):
        gpu.sign_batch(co.ints_to_limbs(keys[:2], 4), gpu.SIG_DOMAIN, msgs, extras, 0)
    assert gpu.scalar_mul_last_ms() == rec


def test_transitions_record(gpu):
    b, blocks, sigs, _, _ = TT._world(gpu, ((2, "valid", 1),), 4242, n_keys=4)
    assert b.nb == 3
    for mode in (0, 1):
        TT._check(b, TT._run(gpu, b, blocks, sigs, mode), mode)
        rec = gpu.transitions_last()
        ms = list(rec["ms"].values())
        assert rec["path"] == mode
        _whole(ms, 6)
        assert ms[3] >= gpu.hash_last_ms() > 0                    # the CRH and the tail: the hash unit's record holds the tail
        assert ms[0] > 0 and ms[1] > 0 and ms[5] > 0 and ms[7] > 0, ms
        assert gpu.seals_last()["path"] == -1                     # the key sums ran through aggregate_by_bitmap: its record is theirs
    with pytest.raises(ValueError):
        TT._run(gpu, b, blocks, sigs, 2)
    assert gpu.transitions_last() == rec


@pytest.fixture(scope="module")
def two_proofs():
    """two valid proofs of the epoch circuit under one key, with their block pairs"""
    key = gc.Key(2, 0xE90C)
    pairs = TE.pair_pool()[:2]
    rng = ecc.SplitMix64(0xE90C3)
    batch = gc.Batch(key, [gc.valid_proof(key, rng, x=EC.expected_inputs(f, l)) for f, l in pairs])
    return key, pairs, batch.serialize()


def test_epoch_and_groth16_records(gpu, two_proofs):
    key, pairs, proofs = two_proofs
    vk = gpu.VerifyingKey(key.alpha, key.beta, key.gamma, key.delta, key.abc)
    try:
        bf, bl = TE.blocks(gpu, [f for f, _ in pairs]), TE.blocks(gpu, [l for _, l in pairs])
        for mode, path in ((0, "each"), (1, "combined accepted")):
            ok, st = gpu.verify_epoch_proofs(vk, proofs, bf, bl, mode=mode, key=TE.KEY8)
            assert ok.tolist() == [1, 1] and not st.any()
            ms = (C.c_float * 8)()
            assert gpu.lib().celo_amd_epoch_last(ms) == 0
            ms = list(ms)
            _whole(ms, 6, unused=(7,))
            assert ms[0] > 0 and ms[3] > 0 and ms[5] > 0, ms
            got_path, _, g = gpu.groth16_verify_last()
            assert got_path == path
            _whole(g, 5, unused=(7,))
            assert 0 < g[4] <= g[5] <= ms[5]                      # the products within the verifier's call, and that within the epoch call's slot
        with pytest.raises(ValueError):
            gpu.verify_epoch_proofs(vk, proofs, bf, bl, mode=2)
        after = (C.c_float * 8)()
        assert gpu.lib().celo_amd_epoch_last(after) == 0 and list(after) == ms
    finally:
        vk.release()


def test_seals_beside_hashing_and_decoding_from_another_thread(gpu):
    """thread A: 20 seal calls, modes alternating; thread B: 20 rounds of 2048 hashes and 2048 decoded points.  Every result is the
    single-threaded one, and every record A reads is a whole record of a seals call"""
    b = _seals()
    n = 2048
    msgs = [b"beside %d" % i for i in range(n)]
    sig, att = gpu.sign_batch(co.ints_to_limbs([0x5EA15], 4), gpu.SIG_DOMAIN, msgs, None, 0)      # 2048 points of G1, compressed
    assert (att != 255).all()
    points = sig.tobytes()
    want_hash = gpu.hash_to_g1_direct(gpu.SIG_DOMAIN, msgs)
    want_dec = gpu.decompress("g1", points)
    assert not want_dec[1].any()
    want_seals = {mode: TS._verify(gpu, b, mode) for mode in (0, 1)}
    errors = []

    def seals():
        try:
            for i in range(20):
                mode = i % 2
                ok, st = TS._verify(gpu, b, mode)
                assert np.array_equal(ok, want_seals[mode][0]) and np.array_equal(st, want_seals[mode][1]), i
                _seals_record_ok(gpu, gpu.seals_last(), mode)
        except BaseException as e:      # noqa: BLE001
            errors.append(e)

    def beside():
        try:
            for i in range(20):
                xy, at = gpu.hash_to_g1_direct(gpu.SIG_DOMAIN, msgs)
                assert np.array_equal(xy, want_hash[0]) and np.array_equal(at, want_hash[1]), i
                dxy, dst = gpu.decompress("g1", points)
                assert np.array_equal(dxy, want_dec[0]) and np.array_equal(dst, want_dec[1]), i
        except BaseException as e:      # noqa: BLE001
            errors.append(e)
    ts = [threading.Thread(target=seals), threading.Thread(target=beside)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errors, errors
