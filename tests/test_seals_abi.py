"""CPU (-m "not gpu"): the entry points of the masked segmented point sums (include/celo_bls_amd.h: aggregate_by_bitmap_*) are declared,
exported and wrapped; every refusal of the contract returns 2 before the device is looked for and leaves the outputs untouched; without a
device the wrappers raise."""
import ctypes as C
import numpy as np
import pytest
from test_abi_symbols import declared_symbols

NAMES = ["aggregate_by_bitmap_bls12_377_g1", "aggregate_by_bitmap_bls12_377_g2", "aggregate_by_bitmap_bls12_377_g1_dev", "aggregate_by_bitmap_bls12_377_g2_dev",
         "verify_aggregated_seals_bls12_377", "celo_amd_aggregate_set_lanes", "celo_amd_aggregate_set_complement", "celo_amd_seals_last"]
SENTINEL = 0x5A5A5A5A5A5A5A5A


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_symbols_are_declared_exported_and_wrapped():
    from celo_bls_snark_rs_amd import ffi
    lib = C.CDLL(ffi.LIB_PATH)
    decl = declared_symbols()
    for name in NAMES:
        assert name in ffi.EXPORTS and name in decl and hasattr(lib, name), name
    for wrapper in ("aggregate_by_bitmap", "aggregate_by_bitmap_dev", "set_aggregate_lanes", "set_aggregate_complement", "seals_last", "verify_aggregated_seals"):
        assert callable(getattr(ffi, wrapper)), wrapper
    assert ffi.AGGREGATE_LANES == (1, 2, 4, 8, 16, 32, 64)


@pytest.mark.parametrize("group,aw", [("bls12_377_g1", 12), ("bls12_377_g2", 24)])
def test_refused_arguments_need_no_device_and_write_nothing(group, aw):
    from celo_bls_snark_rs_amd import ffi
    m, n = 3, 4
    xy = np.zeros((m * n, aw), dtype=np.uint64)
    bits = np.ones(m * n, dtype=np.uint8)
    per_seal = np.array([0, 4, 8, 12], dtype=np.uint32)
    shared = np.array([0, 4], dtype=np.uint32)
    refused = [("pk_xy NULL", None, per_seal, m, bits, m, True, True), ("offsets NULL", xy, None, m, bits, m, True, True),
               ("bits NULL", xy, per_seal, m, None, m, True, True), ("out_xy NULL", xy, per_seal, m, bits, m, False, True),
               ("out_inf NULL", xy, per_seal, m, bits, m, True, False), ("two sets for three seals", xy, per_seal, 2, bits, m, True, True),
               ("no set", xy, per_seal, 0, bits, m, True, True), ("decreasing offsets", xy, np.array([0, 8, 4, 12], dtype=np.uint32), m, bits, m, True, True),
               ("decreasing shared offsets", xy, np.array([4, 0], dtype=np.uint32), 1, bits, m, True, True),
               ("m above 2^24", xy, shared, 1, bits, (1 << 24) + 1, True, True)]
    for dev in (False, True):
        fn = getattr(ffi.lib(), "aggregate_by_bitmap_" + group + ("_dev" if dev else ""))
        for label, pk, off, n_sets, b, seals, with_out, with_inf in refused:
            out = np.full((m, aw), SENTINEL, dtype=np.uint64)
            oinf = np.full(m, 9, dtype=np.uint8)
            cnt = np.full(m, 0x5A5A5A5A, dtype=np.uint32)
            args = [_p(pk), None, _p(off), C.c_size_t(n_sets), _p(b), C.c_size_t(seals), _p(out) if with_out else None, _p(oinf) if with_inf else None, _p(cnt)]
            assert fn(*(args + ([None] if dev else []))) == 2, (label, dev)
            assert (out == SENTINEL).all() and (oinf == 9).all() and (cnt == 0x5A5A5A5A).all(), (label, dev)
        # m = 0: nothing to do, whatever the pointers
        assert fn(*([None, None, None, C.c_size_t(0), None, C.c_size_t(0), None, None, None] + ([None] if dev else []))) == 0


def test_verdict_call_refusals_need_no_device_and_write_nothing():
    from celo_bls_snark_rs_amd import ffi
    m, n = 3, 4
    base = dict(pk=np.zeros((n, 24), dtype=np.uint64), offsets=np.array([0, n], dtype=np.uint32), n_sets=1, bits=np.ones(m * n, dtype=np.uint8),
                dom=np.frombuffer(b"ULforxof", dtype=np.uint8), msgs=np.frombuffer(b"abc", dtype=np.uint8), moff=np.array([0, 1, 2, 3], dtype=np.uint64), hash_mode=0,
                sig=np.zeros((m, 48), dtype=np.uint8), ng2=np.zeros(24, dtype=np.uint64), m=m, mode=0, out=True)
    cases = [("pk NULL", dict(pk=None)), ("offsets NULL", dict(offsets=None)), ("bits NULL", dict(bits=None)), ("domain NULL", dict(dom=None)), ("msgs NULL", dict(msgs=None)),
             ("msg_off NULL", dict(moff=None)), ("sig NULL", dict(sig=None)), ("neg_g2 NULL", dict(ng2=None)), ("out_ok NULL", dict(out=False)),
             ("hash mode 1", dict(hash_mode=1)), ("hash mode 4", dict(hash_mode=4)), ("mode 2", dict(mode=2)), ("mode -1", dict(mode=-1)), ("two sets", dict(n_sets=2)),
             ("decreasing offsets", dict(offsets=np.array([4, 0], dtype=np.uint32))), ("m above 2^24", dict(m=(1 << 24) + 1))]
    for label, change in cases:
        a = dict(base, **change)
        ok = np.full(m, 9, dtype=np.uint8)
        st = np.full(m, 9, dtype=np.uint8)
        rc = ffi.lib().verify_aggregated_seals_bls12_377(_p(a["pk"]), None, _p(a["offsets"]), C.c_size_t(a["n_sets"]), _p(a["bits"]), None, _p(a["dom"]), _p(a["msgs"]),
                                                         _p(a["moff"]), None, None, C.c_int(a["hash_mode"]), _p(a["sig"]), _p(a["ng2"]), C.c_size_t(a["m"]), C.c_int(a["mode"]),
                                                         None, _p(ok) if a["out"] else None, _p(st))
        assert rc == 2, label
        assert (ok == 9).all() and (st == 9).all(), label
    assert ffi.lib().verify_aggregated_seals_bls12_377(*([None] * 3 + [C.c_size_t(0)] + [None] * 7 + [C.c_int(0), None, None, C.c_size_t(0), C.c_int(0), None, None, None])) == 0


def test_hooks_refuse_values_outside_their_range():
    from celo_bls_snark_rs_amd import ffi
    lib = ffi.lib()
    try:
        for lanes in (-1, 3, 5, 6, 48, 65, 128):
            assert lib.celo_amd_aggregate_set_lanes(C.c_int(lanes)) == 2, lanes
            with pytest.raises(ValueError):
                ffi.set_aggregate_lanes(lanes)
        for lanes in (0,) + ffi.AGGREGATE_LANES:
            assert lib.celo_amd_aggregate_set_lanes(C.c_int(lanes)) == 0, lanes
        for mode in (-2, 2, 7):
            assert lib.celo_amd_aggregate_set_complement(C.c_int(mode)) == 2, mode
            with pytest.raises(ValueError):
                ffi.set_aggregate_complement(mode)
        for mode in (-1, 0, 1):
            assert lib.celo_amd_aggregate_set_complement(C.c_int(mode)) == 0, mode
        assert lib.celo_amd_seals_last(None, None, None) == 2
        assert set(ffi.seals_last()) == {"path", "lanes", "ms"}
    finally:
        ffi.set_aggregate_lanes(0)
        ffi.set_aggregate_complement(-1)


def test_no_device_fails_loudly():
    """Without a GPU the sums must refuse, not fall back to a CPU path; a bad argument is a ValueError either way."""
    import torch
    from celo_bls_snark_rs_amd import ffi
    xy = np.zeros((2, 24), dtype=np.uint64)
    with pytest.raises(ValueError):
        ffi.aggregate_by_bitmap("bls12_377_g2", xy, None, [2, 0], np.ones((1, 2), dtype=np.uint8))
    with pytest.raises(ValueError):
        ffi.aggregate_by_bitmap("bw6_761_g1", xy, None, [0, 2], np.ones((1, 2), dtype=np.uint8))
    if torch.cuda.is_available():
        out, inf, cnt = ffi.aggregate_by_bitmap("bls12_377_g2", xy, None, [0, 2], np.zeros((1, 2), dtype=np.uint8))
        assert inf.tolist() == [1] and cnt.tolist() == [0] and not out.any()
        return
    for group in ("bls12_377_g1", "bls12_377_g2"):
        with pytest.raises(RuntimeError):
            ffi.aggregate_by_bitmap(group, np.zeros((2, 24 if group.endswith("g2") else 12), dtype=np.uint64), None, [0, 2], np.ones((1, 2), dtype=np.uint8))
    assert ffi.aggregate_by_bitmap_dev("bls12_377_g2", 16, 0, [0, 2], 16, 1, 16, 16) == 100
    with pytest.raises(RuntimeError):
        ffi.verify_aggregated_seals(xy, None, [0, 2], np.ones((1, 2), dtype=np.uint8), None, b"ULforxof", [b"m"], None, np.zeros((1, 48), dtype=np.uint8),
                                    np.zeros(24, dtype=np.uint64))
