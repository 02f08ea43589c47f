"""CPU (-m "not gpu"): celo_amd_crh_set_lanes and celo_amd_crh_last_lanes are declared, exported and wrapped, and answer without a device:
0 for the rule and for each of the nine widths, 2 for anything else and for a NULL result.  That a refused value leaves the width as it was
is seen where a kernel runs (tests/test_crh_lanes_gpu.py): the library has no reader of the setting."""
import ctypes as C

import pytest
from test_abi_symbols import declared_symbols

NAMES = ["celo_amd_crh_set_lanes", "celo_amd_crh_last_lanes"]


@pytest.fixture()
def ffi():
    from celo_bls_snark_rs_amd import ffi as f
    try:
        yield f
    finally:
        assert f.lib().celo_amd_crh_set_lanes(C.c_int(0)) == 0


def test_symbols_are_declared_exported_and_wrapped(ffi):
    lib = C.CDLL(ffi.LIB_PATH)
    decl = declared_symbols()
    for name in NAMES:
        assert name in ffi.EXPORTS and name in decl and hasattr(lib, name), name
    assert callable(ffi.crh_set_lanes) and callable(ffi.crh_last_lanes)
    assert ffi.CRH_LANES == (1, 2, 4, 8, 16, 32, 64, 128, 256)


def test_the_setter_takes_the_rule_and_the_nine_widths_and_refuses_the_rest(ffi):
    lib = ffi.lib()
    for lanes in (0,) + ffi.CRH_LANES:
        assert lib.celo_amd_crh_set_lanes(C.c_int(lanes)) == 0, lanes
        for bad in (-1, 3, 257, 512):
            assert lib.celo_amd_crh_set_lanes(C.c_int(bad)) == 2, (lanes, bad)
    for bad in (-256, -2, 5, 6, 7, 12, 96, 255, 1024, 2**30):
        assert lib.celo_amd_crh_set_lanes(C.c_int(bad)) == 2, bad
        with pytest.raises(ValueError):
            ffi.crh_set_lanes(bad)
    for lanes in ffi.CRH_LANES + (0,):
        ffi.crh_set_lanes(lanes)


def test_the_reader_refuses_null_and_needs_no_device(ffi):
    lib = ffi.lib()
    assert lib.celo_amd_crh_last_lanes(None) == 2
    lanes = C.c_int(-7)
    assert lib.celo_amd_crh_last_lanes(C.byref(lanes)) == 0
    assert lanes.value in (0,) + ffi.CRH_LANES and ffi.crh_last_lanes() == lanes.value
