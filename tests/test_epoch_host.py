"""CPU (-m "not gpu"): the host twins of the epoch kernels - csrc/epoch.h built with the bounds-tracking field (host_test.cpp, -DCELO_FP_TRACK):
epoch_key_record, epoch_pack_word, epoch_blake2s and epoch_inputs are the templates k_epoch_key_record, k_epoch_pack, k_epoch_blake2s and
k_epoch_inputs run - against the oracle (oracle/py/epoch.py) on the case list of tests/epoch_cases.py."""
import ctypes as C
import hashlib
import numpy as np
import pytest
import epoch_cases as EC
from helpers import build_hosttest
from oracle.py import ecc
from oracle.py import epoch as ep
from oracle import cpu_oracle as co

Q = ecc.Q377
HALF = (Q - 1) // 2
KIND_ID = {k: i for i, k in enumerate(EC.KINDS)}


@pytest.fixture(scope="module")
def ht():
    lib = C.CDLL(build_hosttest())
    lib.ht_epoch_encode.restype = C.c_int64
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _encode(ht, kind, index, round_, mns, maxv, ee, pe, rows, inf, sum_row=None, sum_inf=0):
    n = rows.shape[0]
    cap = EC.encoded_size(kind, n, maxv)
    out = np.full(cap + 8, 0xA5, dtype=np.uint8)
    extra = np.full(7, 0xA5, dtype=np.uint8)
    rows = np.ascontiguousarray(rows if n else np.zeros((1, 24), dtype=np.uint64))
    got = ht.ht_epoch_encode(C.c_int(KIND_ID[kind]), C.c_uint32(index), C.c_uint32(round_), C.c_uint32(mns), C.c_uint32(maxv), ee, pe, _p(rows), _p(inf), C.c_uint32(n),
                             _p(sum_row), C.c_int(sum_inf), _p(out), C.c_uint64(cap), _p(extra))
    assert got == cap, (kind, got, cap)
    assert (out[cap:] == 0xA5).all()
    return out[:cap].tobytes(), (extra.tobytes() if kind == "inner" else None)


def _case_rows(case):
    if not case.keys:
        return np.zeros((0, 24), dtype=np.uint64), None
    return co.pack_g2_377([EC.pool_key(k) for k in case.keys])


def _sum_row(case):
    agg = None
    for k in case.keys:
        agg = ecc.E2_377.add(agg, EC.pool_key(k))
    xy, inf = co.pack_g2_377([agg])
    return np.ascontiguousarray(xy[0]), int(inf[0])


def test_whole_blocks_match_the_oracle_in_every_kind(ht):
    cases = EC.small_cases() + EC.null_entropy_cases() + [EC.border_cases(k)[i] for k, i in (("first", 0), ("last", 1), ("inner", 2))]
    for c in cases:
        rows, inf = _case_rows(c)
        for kind in EC.KINDS:
            s_row, s_inf = _sum_row(c) if kind == "last" else (None, 0)
            got = _encode(ht, kind, c.index, c.round, c.mns, c.maxv, c.ee, c.pe, rows, inf, s_row, s_inf)
            assert got == EC.expected(c, kind), (c.ident(), kind)


def test_golden_strings_through_the_twin(ht, golden):
    e = golden["epoch_encoding"]
    gen, _ = co.pack_g2_377([ecc.G2_377] * 10)
    f, g = bytes([255] * 16), bytes([254] * 16)
    assert _encode(ht, "first", 120, 5, 3, 10, f, g, gen, None)[0].hex() == e["EXPECTED_ENCODING_WITH_ENTROPY"]
    assert _encode(ht, "first", 120, 5, 3, 10, None, None, gen, None)[0].hex() == e["EXPECTED_ENCODING_WITHOUT_ENTROPY"]
    assert _encode(ht, "legacy", 120, 10, 3, 10, None, None, gen, None)[0].hex() == e["EXPECTED_ENCODING_BEFORE_DONUT"]
    assert _encode(ht, "first", 120, 5, 3, 11, f, g, gen, None)[0].hex() == e["EXPECTED_ENCODING_WITH_ENTROPY_PADDED"]


def _row(x0, x1, y0, y1):
    return co.to_mont([x0, x1, y0, y1], Q).reshape(1, 24)


SIGN_ROWS = [((0, 0), 0), ((0, HALF), 0), ((0, HALF + 1), 1), ((0, Q - 1), 1),            # y = (c0, c1): c1 decides unless it is zero
             ((HALF, 0), 0), ((HALF + 1, 0), 1), ((Q - 1, 0), 1), ((Q - 1, 1), 0), ((0, 1), 0), ((1, HALF + 1), 1)]
X_VALUES = [0, 1, 2, (1 << 64) - 1, 1 << 64, (1 << 64) + 1, (1 << 128) - 1, 1 << 128, (1 << 192) - 1, 1 << 192, (1 << 256) - 1, 1 << 256, (1 << 320) - 1,
            1 << 320, (1 << 376) - 1, 1 << 376, Q - 2, Q - 1]


@pytest.mark.parametrize("kind", ["first", "inner", "legacy"])
def test_sign_rule_and_x_borders_on_rows_off_the_curve(ht, kind):
    """keys_form 1 does not look at the curve: any (x, y) is a record.  Every sign-rule row yields its bit, x at the limb borders and at q - 1
    lands bit for bit.  (Not the last form: rows off the curve must not be summed.)"""
    for (y0, y1), bit in SIGN_ROWS:
        pk = ((5, 7), (y0, y1))
        assert ep.encode_public_key(pk)[-1] == bit
        blk = ep.EpochBlock(9, 1, None, bytes(range(16)), 4, 0, [pk])
        want = {"first": blk.encode_first_epoch_to_bytes_cip22, "legacy": blk.encode_to_bytes}.get(kind, lambda: ep.encode_inner_to_bytes_cip22(blk)[0])()
        assert _encode(ht, kind, 9, 1, 4, 0, None, bytes(range(16)), _row(5, 7, y0, y1), None)[0] == want, (y0, y1)
    pks = [((x, X_VALUES[-1 - i]), (1, 0)) for i, x in enumerate(X_VALUES)]
    blk = ep.EpochBlock(1, 2, bytes(16), None, 3, 0, pks)
    want = {"first": blk.encode_first_epoch_to_bytes_cip22, "legacy": blk.encode_to_bytes}.get(kind, lambda: ep.encode_inner_to_bytes_cip22(blk)[0])()
    rows = np.concatenate([_row(p[0][0], p[0][1], 1, 0) for p in pks])
    assert _encode(ht, kind, 1, 2, 3, 0, bytes(16), None, rows, None)[0] == want


def test_key_record_is_the_reversed_bit_string(ht):
    rng = ecc.SplitMix64(77)
    for _ in range(8):
        x0, x1, y0, y1 = (ecc.random_scalar(rng, Q) for _ in range(4))
        rec = np.zeros(24, dtype=np.uint32)
        ht.ht_epoch_key_record(_p(_row(x0, x1, y0, y1)), C.c_int(0), _p(rec))
        bits = ep.encode_public_key(((x0, x1), (y0, y1)))
        assert int.from_bytes(rec.tobytes(), "little") == int("".join(map(str, bits)), 2)
    rec = np.full(24, 9, dtype=np.uint32)
    ht.ht_epoch_key_record(_p(_row(1, 2, 3, 4)), C.c_int(1), _p(rec))
    assert not rec.any()


def test_identity_through_inf_and_as_a_compressed_key(ht):
    """arkworks' zero() = (0, 1): 755 zero bits, through the flag and through the decoder's status"""
    real, _ = co.pack_g2_377([EC.pool_key(0), EC.pool_key(1)])
    c = EC.Case(3, 4, EC.entropy(1), None, 2, 4, [0, EC.IDENTITY, 1])
    rows = np.stack([real[0], np.zeros(24, dtype=np.uint64), real[1]])
    enc = b"".join(EC.pool_bytes(k) for k in c.keys)
    dec = np.zeros((3, 24), dtype=np.uint64)
    st = np.zeros(3, dtype=np.uint8)
    ht.ht_wire_decode(C.c_int(1), enc, C.c_size_t(3), C.c_int(1), _p(dec), _p(st))
    assert st.tolist() == [0, 1, 0]
    for kind in EC.KINDS:
        s_row, s_inf = _sum_row(c) if kind == "last" else (None, 0)
        want = EC.expected(c, kind)
        assert _encode(ht, kind, c.index, c.round, c.mns, c.maxv, c.ee, c.pe, rows, np.array([0, 1, 0], dtype=np.uint8), s_row, s_inf) == want, kind
        assert _encode(ht, kind, c.index, c.round, c.mns, c.maxv, c.ee, c.pe, dec, (st == 1).astype(np.uint8), s_row, s_inf) == want, kind


def test_blake2s_at_every_final_block_border(ht):
    rng = np.random.default_rng(5)
    for n in (0, 1, 22, 55, 63, 64, 65, 127, 128, 129, 1344, 3137, 5119, 14273):
        msg = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        out = np.zeros(32, dtype=np.uint8)
        ht.ht_epoch_blake2s(msg, C.c_uint64(n), _p(out))
        assert out.tobytes() == hashlib.blake2s(msg, digest_size=32, person=ep.OUT_DOMAIN).digest(), n


def test_inputs_pack_376_and_136_bits(ht):
    rng = np.random.default_rng(6)
    pairs = [(bytes(32), bytes(32)), (b"\xff" * 32, b"\xff" * 32), (b"\x01" + bytes(31), bytes(31) + b"\x80"), (bytes(31) + b"\x80", b"\x01" + bytes(31))]
    pairs += [(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), rng.integers(0, 256, 32, dtype=np.uint8).tobytes()) for _ in range(16)]
    for h1, h2 in pairs:
        want = ep.pack(ep.bytes_le_to_bits_le(h1, 256) + ep.bytes_le_to_bits_le(h2, 256))
        out = np.zeros(12, dtype=np.uint64)
        ht.ht_epoch_inputs(h1, h2, _p(out))
        assert co.limbs_to_ints(out.reshape(2, 6), 6) == want
        assert want[0] < 1 << 376 and want[1] < 1 << 136 < ecc.R761
