"""CPU (-m "not gpu"): verify_epoch_transitions_bls12_377, celo_amd_transitions_last and the four device-resident hash entries are declared,
exported and wrapped; every refusal of the chain check returns 2 before the device is looked for and leaves the outputs untouched; nb = 0
returns 0; without a device a good call refuses loudly (code 100)."""
import ctypes as C
import numpy as np
import pytest
import epoch_cases as EC
from test_abi_symbols import declared_symbols
from test_epoch_abi import _blocks, _p, BLOCK_REFUSALS

NAMES = ["verify_epoch_transitions_bls12_377", "celo_amd_transitions_last", "composite_crh_bls12_377_dev", "hash_to_g1_direct_bls12_377_dev",
         "hash_to_g1_cip22_tail_bls12_377_dev", "hash_to_g1_composite_bls12_377_dev"]
NB = 3


def test_symbols_are_declared_exported_and_wrapped():
    from celo_bls_snark_rs_amd import ffi
    lib = C.CDLL(ffi.LIB_PATH)
    decl = declared_symbols()
    for name in NAMES:
        assert name in ffi.EXPORTS and name in decl and hasattr(lib, name), name
    for wrapper in ("verify_epoch_transitions", "transitions_last", "composite_crh_dev", "hash_to_g1_dev"):
        assert callable(getattr(ffi, wrapper)), wrapper
    assert len(ffi.TRANSITION_STATUS) == 11


def _call(ffi, b, nb=NB, chain_off=(0, 3), n_chains=None, bits=True, sig=True, dom=True, ng2=True, mode=0, ok=True):
    """-> (code, whether every output is untouched)"""
    co = None if chain_off is None else np.array(chain_off, dtype=np.uint32)
    n_chains = (len(chain_off) - 1 if chain_off is not None else 1) if n_chains is None else n_chains
    bt = np.ones(8, dtype=np.uint8)
    sg = np.zeros((NB, 48), dtype=np.uint8)
    d = np.frombuffer(b"ULforxof", dtype=np.uint8)
    g = np.ones(24, dtype=np.uint64)
    o_ok, o_st, o_cok, o_att, o_ainf = (np.full(NB, 9, dtype=np.uint8) for _ in range(5))
    o_crh = np.full((NB, 48), 9, dtype=np.uint8)
    o_axy = np.full((NB, 12), 9, dtype=np.uint64)
    rc = ffi.lib().verify_epoch_transitions_bls12_377(C.byref(b.c) if b is not None else None, C.c_size_t(nb), _p(co), C.c_size_t(n_chains), _p(bt) if bits else None,
                                                      _p(sg) if sig else None, _p(d) if dom else None, _p(g) if ng2 else None, C.c_int(mode), _p(o_ok) if ok else None,
                                                      _p(o_st), _p(o_cok), _p(o_crh), _p(o_att), _p(o_axy), _p(o_ainf))
    return rc, all((a == 9).all() for a in (o_ok, o_st, o_cok, o_att, o_ainf, o_crh, o_axy))


def test_refusals_need_no_device_and_write_nothing():
    from celo_bls_snark_rs_amd import ffi
    good = _blocks(ffi)[0]
    cases = [(label, dict(b=_blocks(ffi, **ch)[0])) for label, ch in BLOCK_REFUSALS]
    cases += [("round NULL", dict(b=_blocks(ffi, round=None)[0])), ("blocks NULL", dict(b=None)), ("chain_off NULL", dict(chain_off=None)), ("bits NULL", dict(bits=False)),
              ("sig48 NULL", dict(sig=False)), ("domain NULL", dict(dom=False)), ("neg_g2 NULL", dict(ng2=False)), ("out_ok NULL", dict(ok=False)),
              ("mode 2", dict(mode=2)), ("mode -1", dict(mode=-1)), ("no chain", dict(chain_off=(0,), n_chains=0)), ("chain_off not from 0", dict(chain_off=(1, 3))),
              ("chain_off not to nb", dict(chain_off=(0, 2))), ("chain_off past nb", dict(chain_off=(0, 4))), ("an empty chain", dict(chain_off=(0, 2, 2, 3))),
              ("an empty first chain", dict(chain_off=(0, 0, 3))), ("decreasing chain_off", dict(chain_off=(0, 2, 1, 3))), ("more chains than blocks", dict(chain_off=(0, 1, 2, 3, 3))),
              ("nb above 2^24", dict(nb=(1 << 24) + 1, chain_off=(0, (1 << 24) + 1)))]
    # the Pedersen table: K = max(n_keys, max_validators) = 206 fits, 207 does not (the reference panics there)
    cases += [("max_validators 207", dict(b=_blocks(ffi, max_validators=np.array([4, 207, 3], dtype=np.uint32))[0])),
              ("a block of 207 keys", dict(b=_blocks(ffi, key_off=np.array([0, 2, 2, 209], dtype=np.uint32), keys=np.zeros((209, 96), dtype=np.uint8))[0]))]
    for label, change in cases:
        rc, untouched = _call(ffi, **dict(dict(b=good), **change))
        assert rc == 2, label
        assert untouched, label
    assert ffi.lib().verify_epoch_transitions_bls12_377(None, C.c_size_t(0), None, C.c_size_t(0), None, None, None, None, C.c_int(0), None, None, None, None, None, None, None) == 0
    path, ms = C.c_int(0), (C.c_float * 8)()
    assert ffi.lib().celo_amd_transitions_last(None, ms) == 2 and ffi.lib().celo_amd_transitions_last(C.byref(path), None) == 2
    rec = ffi.transitions_last()
    assert set(rec["ms"]) == {"decode", "sums", "pack", "hash", "transfers", "products", "wall", "signatures"} and rec["path"] in (-1, 0, 1, 2)


def test_what_fits_the_pedersen_table_passes_the_refusals():
    """206 key slots is no refusal: the call goes on to look for a device (0 with one, 100 without)"""
    import torch
    from celo_bls_snark_rs_amd import ffi
    b = _blocks(ffi, max_validators=np.array([4, 206, 3], dtype=np.uint32))[0]
    rc, _ = _call(ffi, b)
    assert rc == (0 if torch.cuda.is_available() else 100)


def test_wrapper_refuses_and_without_a_device_fails_loudly():
    import torch
    from celo_bls_snark_rs_amd import ffi
    good, cases = _blocks(ffi)
    ng2 = np.ones(24, dtype=np.uint64)
    with pytest.raises(ValueError):
        ffi.verify_epoch_transitions(good, [0, 3], np.ones(4, dtype=np.uint8), np.zeros((3, 48), dtype=np.uint8), b"ULforxof", ng2)      # 5 keys, 4 bytes
    with pytest.raises(ValueError):
        ffi.verify_epoch_transitions(good, [0, 3], np.ones(5, dtype=np.uint8), np.zeros((2, 48), dtype=np.uint8), b"ULforxof", ng2)      # 3 blocks, 2 signatures
    with pytest.raises(ValueError):
        ffi.verify_epoch_transitions(good, [0, 2], np.ones(5, dtype=np.uint8), np.zeros((3, 48), dtype=np.uint8), b"ULforxof", ng2)      # code 2
    if torch.cuda.is_available():
        return
    with pytest.raises(RuntimeError):
        ffi.verify_epoch_transitions(good, [0, 3], np.ones(5, dtype=np.uint8), np.zeros((3, 48), dtype=np.uint8), b"ULforxof", ng2)
    off = np.array([0, 4], dtype=np.uint64)
    assert ffi.composite_crh_dev(16, off, 1, 16) == 100
    for mode in range(4):
        assert ffi.hash_to_g1_dev(b"ULforxof", 16, off, 0, None, 1, 16, 16, mode=mode) == 100
