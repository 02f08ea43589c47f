"""CPU: the many-lane form of the composite hasher's Pedersen CRH (csrc/pedersen.h: pedersen_crh_lane_sum, the fold of k_pedersen_crh_lanes,
crh_pick_lanes) through host_test.cpp under bounds tracking, on the three-window generator table of tests/test_hash_host.py.  The hash is the x
of a sum in a group, so every width must give the 48 bytes of the one-lane form and of oracle/py/composite.py."""
import ctypes as C

import numpy as np
import pytest

from oracle.py import composite as comp
from tests import helpers as H
from test_hash_host import small_table, TABLE_CHUNKS, TABLE_BYTES      # noqa: F401  (small_table: a fixture)

WIDTHS = (1, 2, 4, 8, 16, 32, 64, 128, 256)
MAX_LANES = 256
BLOCK = 256                      # lanes of a workgroup of the lanes kernel (pedersen.h CRH_BLOCK)
GRID_LANES = (2**31 - 1) * BLOCK  # the lanes a 31-bit grid of workgroups holds


@pytest.fixture(scope="module")
def ht():
    lib = C.CDLL(H.build_hosttest())
    lib.ht_crh_pick_lanes.restype = C.c_uint32
    lib.ht_crh_pick_lanes.argtypes = [C.c_uint32, C.c_size_t, C.c_size_t]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def messages():
    """random bytes and the all-ones string (every chunk: 4g, negated) of every length the table covers, with their oracle hashes"""
    rng = np.random.default_rng(0x1A9E5)
    msgs = [m for l in range(TABLE_BYTES + 1) for m in (bytes(rng.integers(0, 256, size=l, dtype=np.uint8)), b"\xff" * l)]
    return [(m, comp.composite_crh(m)) for m in msgs]


@pytest.mark.parametrize("L", WIDTHS)
def test_lanes_equal_one_lane_and_the_oracle_at_every_length(ht, small_table, messages, L):
    """lengths 0 ... 104 bytes are chunk counts 0 ... 278: 0, 1, L - 1, L, L + 1, 2 L - 1, 2 L + 1 for every L up to 128, all three bit
    alignments of the last chunk, and for L = 256 lanes without a chunk at every length"""
    for msg, want in messages:
        one, got = np.zeros(48, dtype=np.uint8), np.zeros(48, dtype=np.uint8)
        assert ht.ht_pedersen_crh(_p(small_table), C.c_size_t(TABLE_CHUNKS), msg, C.c_size_t(len(msg)), _p(one)) == 0
        assert ht.ht_pedersen_crh_lanes(_p(small_table), C.c_size_t(TABLE_CHUNKS), msg, C.c_size_t(len(msg)), C.c_int(L), _p(got)) == 0
        assert got.tobytes() == one.tobytes() == want, (L, len(msg))


def test_refused_widths_and_lengths(ht, small_table):
    out = np.zeros(48, dtype=np.uint8)
    for L in (0, -1, 3, 257, 512):
        assert ht.ht_pedersen_crh_lanes(_p(small_table), C.c_size_t(TABLE_CHUNKS), b"abc", C.c_size_t(3), C.c_int(L), _p(out)) == -2
    assert ht.ht_pedersen_crh_lanes(_p(small_table), C.c_size_t(TABLE_CHUNKS), bytes(TABLE_BYTES + 1), C.c_size_t(TABLE_BYTES + 1), C.c_int(4), _p(out)) == -2
    assert not out.any()


CHUNKS = sorted({0, 1, 2, 3, 5, 31, 32, 33, 34, 63, 64, 65, 100, 127, 128, 129, 255, 256, 257, 339, 511, 512, 513, 1000, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096,
                 4097, 8191, 8192, 8193, 16384, 16385, 27734, 37867, 52080})
COUNTS = sorted({1, 2, 3, 63, 64, 65, 127, 128, 129, 143, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 8191, 8192, 8193, 16384, 32767, 32768,
                 32769, 65535, 65536, 65537, 131072, 2**20, 2**31 - 1})


def test_the_rule_gives_a_power_of_two_monotone_in_the_work_and_against_the_count(ht):
    table = {(c, n): ht.ht_crh_pick_lanes(0, c, n) for c in CHUNKS for n in COUNTS}
    for (c, n), L in table.items():
        assert 1 <= L <= MAX_LANES and L & (L - 1) == 0, (c, n, L)
    for n in COUNTS:
        col = [table[c, n] for c in CHUNKS]
        assert col == sorted(col), n                               # more chunks: never fewer lanes
        assert table[0, n] == 1
    for c in CHUNKS:
        row = [table[c, n] for n in COUNTS]
        assert row == sorted(row, reverse=True), c                 # more messages: never more lanes
    # the long single message and the few long messages get many lanes
    assert table[37867, 1] > 1 and table[27734, 64] > 1


def test_the_rule_is_one_lane_for_a_call_that_fills_the_device(ht):
    """CRH_FILL_LANES: the smallest power of two of messages from which the rule gives 1 whatever the length (half as many still get two
    lanes); the bulk short-message calls (65 536 x 127 B, 65 537 x 12 B) lie at or above it"""
    fill = next(n for n in (2**k for k in range(32)) if ht.ht_crh_pick_lanes(0, 52080, n) == 1)
    assert fill <= 65536
    assert ht.ht_crh_pick_lanes(0, 52080, fill // 2) == 2
    for n in (fill, fill + 1, 65536, 65537, 2**24, 2**31 - 1):
        for c in (0, 1, 32, 339, 52080):
            assert ht.ht_crh_pick_lanes(0, c, n) == 1, (c, n)
    assert ht.ht_crh_pick_lanes(0, (127 * 8 + 2) // 3, 65536) == 1 and ht.ht_crh_pick_lanes(0, (12 * 8 + 2) // 3, 65537) == 1


def test_a_request_is_returned_while_the_grid_holds_it_and_halved_beyond(ht):
    for L in WIDTHS:
        for c in (0, 1, 52080):
            for n in (1, 64, 65537, 2**31 - 1, GRID_LANES // L):
                assert ht.ht_crh_pick_lanes(L, c, n) == L, (L, c, n)
        if L > 1:
            assert ht.ht_crh_pick_lanes(L, 52080, GRID_LANES // L + 1) == L // 2
        for n in (2**40, 2**41 + 1, 2**45):                        # counts no call has: the clamp alone
            want = L
            while want > 1 and n * want > GRID_LANES:
                want //= 2
            assert ht.ht_crh_pick_lanes(L, 52080, n) == want, (L, n)
            assert ht.ht_crh_pick_lanes(0, 52080, n) == 1
