"""CPU (-m "not gpu"): the entry points of the epoch unit (include/celo_bls_amd.h: epoch_*, verify_epoch_proofs_bw6_761) are declared, exported
and wrapped; every refusal of the contract returns 2 before the device is looked for and leaves the outputs untouched; the size function is
host code; without a device the wrappers raise."""
import ctypes as C
import numpy as np
import pytest
import epoch_cases as EC
from test_abi_symbols import declared_symbols

NAMES = ["epoch_encoded_size", "epoch_encode_blocks_bls12_377", "epoch_encode_blocks_bls12_377_dev", "epoch_public_inputs_bw6_761", "epoch_public_inputs_bw6_761_dev",
         "verify_epoch_proofs_bw6_761", "celo_amd_epoch_last"]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_symbols_are_declared_exported_and_wrapped():
    from celo_bls_snark_rs_amd import ffi
    lib = C.CDLL(ffi.LIB_PATH)
    decl = declared_symbols()
    for name in NAMES:
        assert name in ffi.EXPORTS and name in decl and hasattr(lib, name), name
    for wrapper in ("EpochBlocks", "epoch_encoded_size", "epoch_encode_blocks", "epoch_encode_blocks_dev", "epoch_public_inputs", "epoch_public_inputs_dev",
                    "verify_epoch_proofs", "epoch_last"):
        assert callable(getattr(ffi, wrapper)), wrapper
    assert ffi.EPOCH_KINDS == {k: i for i, k in enumerate(EC.KINDS)} and ffi.EPOCH_MAX_KEYS == EC.MAX_KEYS
    assert C.sizeof(ffi.EpochBlocksC) == 10 * C.sizeof(C.c_void_p)


def test_size_function_is_the_formula_and_needs_no_device():
    from celo_bls_snark_rs_amd import ffi
    for kind in EC.KINDS:
        for n, v in ((0, 0), (1, 0), (0, 1), (9, 4), (4, 9), (150, 150), (110, 150), (EC.MAX_KEYS, 0), (0, EC.MAX_KEYS)):
            assert ffi.epoch_encoded_size(kind, n, v) == EC.encoded_size(kind, n, v), (kind, n, v)
    assert ffi.epoch_encoded_size("first", 0, 0) == 22 and ffi.epoch_encoded_size("inner", 1, 0) == 127
    out = C.c_uint64(77)
    for kind, n, v in ((-1, 0, 0), (4, 0, 0), (0, EC.MAX_KEYS + 1, 0), (0, 0, EC.MAX_KEYS + 1), (3, 0, EC.MAX_KEYS + 1), (1, 1 << 40, 0)):
        assert ffi.lib().epoch_encoded_size(C.c_int(kind), C.c_uint64(n), C.c_uint64(v), C.byref(out)) == 2 and out.value == 77
    assert ffi.lib().epoch_encoded_size(C.c_int(0), C.c_uint64(0), C.c_uint64(0), None) == 2


def _blocks(ffi, **change):
    """three blocks of 2, 0 and 3 keys; `change` replaces arrays (None = a NULL pointer)"""
    cases = [EC.Case(1, 2, None, None, 3, 4, [0, 1]), EC.Case(5, 6, None, None, 7, 0, []), EC.Case(9, 10, None, None, 11, 3, [2, 3, 4])]
    b = ffi.EpochBlocks(**EC.arrays(cases))
    for name, val in change.items():
        if name == "keys_form":
            b.c.keys_form = val
        else:
            keep = None if val is None else np.ascontiguousarray(val)
            setattr(b, "_keep_" + name, keep)
            setattr(b.c, name, None if keep is None else _p(keep).value)
    return b, cases


BLOCK_REFUSALS = [("index NULL", dict(index=None)), ("max_non_signers NULL", dict(max_non_signers=None)), ("max_validators NULL", dict(max_validators=None)),
                  ("key_off NULL", dict(key_off=None)), ("keys NULL", dict(keys=None)), ("keys_form 2", dict(keys_form=2)), ("keys_form -1", dict(keys_form=-1)),
                  ("decreasing key_off", dict(key_off=np.array([0, 2, 1, 5], dtype=np.uint32))),
                  ("a block of 65 537 keys", dict(key_off=np.array([0, 2, 2, 2 + EC.MAX_KEYS + 1], dtype=np.uint32))),
                  ("max_validators 65 537", dict(max_validators=np.array([4, EC.MAX_KEYS + 1, 3], dtype=np.uint32)))]


def test_encode_refusals_need_no_device_and_write_nothing():
    from celo_bls_snark_rs_amd import ffi
    nb = 3
    for dev in (False, True):
        fn = getattr(ffi.lib(), "epoch_encode_blocks_bls12_377" + ("_dev" if dev else ""))
        for kind in range(4):
            good, cases = _blocks(ffi)
            sizes = [EC.encoded_size(EC.KINDS[kind], len(c.keys), c.maxv) for c in cases]
            off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
            refused = [(label, _blocks(ffi, **ch)[0], nb, kind, off, True, True, True) for label, ch in BLOCK_REFUSALS]
            refused += [("blocks NULL", None, nb, kind, off, True, True, True), ("out_off NULL", good, nb, kind, None, True, True, True),
                        ("out NULL", good, nb, kind, off, False, True, True), ("status NULL", good, nb, kind, off, True, True, False),
                        ("kind 4", good, nb, 4, off, True, True, True), ("kind -1", good, nb, -1, off, True, True, True),
                        ("nb above 2^24", good, (1 << 24) + 1, kind, off, True, True, True),
                        ("out_off not from 0", good, nb, kind, off + np.uint64(1), True, True, True),
                        ("out_off one byte long", good, nb, kind, off + np.array([0, 0, 1, 1], dtype=np.uint64), True, True, True),
                        ("decreasing out_off", good, nb, kind, off[[0, 2, 1, 3]].copy(), True, True, True)]
            if kind == 2:
                refused += [("extras NULL", good, nb, kind, off, True, False, True), ("round NULL", _blocks(ffi, round=None)[0], nb, kind, off, True, True, True)]
            for label, b, n, k, o, with_out, with_extras, with_status in refused:
                out = np.full(int(off[-1]) + 8, 0x5A, dtype=np.uint8)
                extras = np.full((nb, 7), 0x5A, dtype=np.uint8)
                status = np.full(nb, 9, dtype=np.uint8)
                args = [C.byref(b.c) if b is not None else None, C.c_size_t(n), C.c_int(k), _p(o), _p(out) if with_out else None, _p(extras) if with_extras else None,
                        _p(status) if with_status else None]
                assert fn(*(args + ([None] if dev else []))) == 2, (label, kind, dev)
                assert (out == 0x5A).all() and (extras == 0x5A).all() and (status == 9).all(), (label, kind, dev)
        assert fn(*([None, C.c_size_t(0), C.c_int(0), None, None, None, None] + ([None] if dev else []))) == 0          # nb = 0: nothing to do


def test_input_and_verdict_refusals_need_no_device_and_write_nothing():
    from celo_bls_snark_rs_amd import ffi
    m = 3
    good = _blocks(ffi)[0]
    bad = [(label, _blocks(ffi, **ch)[0]) for label, ch in BLOCK_REFUSALS]
    pairs = [("first: " + label, b, good) for label, b in bad] + [("last: " + label, good, b) for label, b in bad] + [("first NULL", None, good), ("last NULL", good, None)]
    ref = lambda b: C.byref(b.c) if b is not None else None
    for dev in (False, True):
        fn = getattr(ffi.lib(), "epoch_public_inputs_bw6_761" + ("_dev" if dev else ""))
        cases = [(label, f, l, m, True, True) for label, f, l in pairs] + [("out_inputs NULL", good, good, m, False, True), ("out_status NULL", good, good, m, True, False),
                                                                           ("m above 2^24", good, good, (1 << 24) + 1, True, True)]
        for label, f, l, n, with_out, with_status in cases:
            out = np.full((m, 12), 0x5A5A, dtype=np.uint64)
            st = np.full(m, 9, dtype=np.uint8)
            args = [ref(f), ref(l), C.c_size_t(n), _p(out) if with_out else None, _p(st) if with_status else None]
            assert fn(*(args + ([None] if dev else []))) == 2, (label, dev)
            assert (out == 0x5A5A).all() and (st == 9).all(), (label, dev)
        assert fn(*([None, None, C.c_size_t(0), None, None] + ([None] if dev else []))) == 0
    # the verdict call: the same block refusals, and a key that is no live BW6-761 handle with two inputs - a NULL handle, a stale pointer
    proofs = np.zeros(m * 288, dtype=np.uint8)
    junk = np.zeros(64, dtype=np.uint64)
    vcases = [(label, C.c_void_p(_p(junk).value), f, l, m, 0, True, True) for label, f, l in pairs]
    vcases += [("vk NULL", None, good, good, m, 0, True, True), ("vk not a handle", C.c_void_p(_p(junk).value), good, good, m, 0, True, True),
               ("proofs NULL", C.c_void_p(_p(junk).value), good, good, m, 0, False, True), ("out_ok NULL", C.c_void_p(_p(junk).value), good, good, m, 0, True, False),
               ("mode 2", C.c_void_p(_p(junk).value), good, good, m, 2, True, True), ("mode -1", C.c_void_p(_p(junk).value), good, good, m, -1, True, True),
               ("m above 2^24", C.c_void_p(_p(junk).value), good, good, (1 << 24) + 1, 0, True, True)]
    for label, vk, f, l, n, mode, with_proofs, with_ok in vcases:
        ok = np.full(m, 9, dtype=np.uint8)
        st = np.full(m, 9, dtype=np.uint8)
        rc = ffi.lib().verify_epoch_proofs_bw6_761(vk, _p(proofs) if with_proofs else None, ref(f), ref(l), C.c_size_t(n), C.c_int(mode), None, _p(ok) if with_ok else None,
                                                   _p(st))
        assert rc == 2, label
        assert (ok == 9).all() and (st == 9).all(), label
    assert ffi.lib().verify_epoch_proofs_bw6_761(None, None, None, None, C.c_size_t(0), C.c_int(0), None, None, None) == 0
    assert ffi.lib().celo_amd_epoch_last(None) == 2
    assert set(ffi.epoch_last()) == {"decode", "sums", "pack", "hash", "transfers", "verify", "wall"}


def test_wrappers_refuse_and_without_a_device_fail_loudly():
    """a bad argument is a ValueError with or without a GPU; without one a good call must refuse (code 100), not fall back to a CPU path"""
    import torch
    from celo_bls_snark_rs_amd import ffi
    good, cases = _blocks(ffi)
    with pytest.raises(ValueError):
        ffi.epoch_encode_blocks(good, 4)
    with pytest.raises(ValueError):
        ffi.epoch_encoded_size("first", EC.MAX_KEYS + 1, 0)
    with pytest.raises(ValueError):
        ffi.epoch_public_inputs(good, ffi.EpochBlocks(**EC.arrays(cases[:2])))
    with pytest.raises(ValueError):
        ffi.EpochBlocks(**dict(EC.arrays(cases), key_off=[0, 2]))
    if torch.cuda.is_available():
        data, extras, status, _ = ffi.epoch_encode_blocks(good, "first")
        assert data == [EC.expected(c, "first")[0] for c in cases] and extras is None and not status.any()
        return
    for kind in EC.KINDS:
        with pytest.raises(RuntimeError):
            ffi.epoch_encode_blocks(good, kind)
    with pytest.raises(RuntimeError):
        ffi.epoch_public_inputs(good, good)
    assert ffi.epoch_encode_blocks_dev(good.c, 3, 0, np.concatenate([[0], np.cumsum([EC.encoded_size("first", len(c.keys), c.maxv) for c in cases])]), 16, 0, 16) == 100
    assert ffi.epoch_public_inputs_dev(good.c, good.c, 3, 16, 16) == 100
