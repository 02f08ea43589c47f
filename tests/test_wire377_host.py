"""CPU (-m "not gpu"): uncompressed BLS12-377 point decoding (csrc/wire.h) and the layout walk and size function of a serialized
ProvingKey<Bls12_377>.

- The new entry points are in the header, in the library and in ffi.EXPORTS.
- groth16_key_layout_bls12_377 (a host walk, no device call) on a key with distinct section lengths: counts and offsets in all three forms, and
  its rejections (truncation at every section border, trailing bytes, a length of 2^61, a length that points past the end, a form out of range).
- groth16_serialized_key_size_bls12_377 against the Python serializer's lengths.
- ht_wire377_decode_uncompressed, the decoding templates under bounds tracking (the kernels run the same functions), against the status rules
  restated in tests/bls377_serial.py on the shared case list, both groups, checked and unchecked."""
import ctypes as C
import os
import numpy as np
import pytest
import bls377_serial as bs
from helpers import build_hosttest

NEW_SYMBOLS = ["decode_uncompressed_bls12_377_g1", "decode_uncompressed_bls12_377_g2", "decode_uncompressed_bls12_377_g1_dev",
               "decode_uncompressed_bls12_377_g2_dev", "groth16_key_layout_bls12_377", "groth16_load_key_bls12_377_serialized",
               "groth16_serialized_key_size_bls12_377", "groth16_serialize_key_bls12_377"]
VECTORS = ("a_query", "b_g1_query", "b_g2_query", "h_query", "l_query")


@pytest.fixture(scope="module")
def ht():
    lib = C.CDLL(build_hosttest())
    lib.ht_wire377_decode_uncompressed.restype = None
    return lib


def test_new_symbols_declared_and_exported():
    from celo_bls_snark_rs_amd import ffi
    lib = C.CDLL(ffi.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "celo_bls_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert name in ffi.EXPORTS and hasattr(lib, name) and ("int %s(" % name) in header, name


COUNTS = {"gamma_abc_g1": 3, "a_query": 5, "b_g1_query": 4, "b_g2_query": 6, "h_query": 7, "l_query": 2}


def _layout_key(form):
    """a key of identities with distinct section lengths (point bytes are opaque to the layout walk), and where its sections begin, worked out
    here from the point sizes: G1 P bytes, G2 2 P"""
    key = {n: ([None] * COUNTS[n] if n in COUNTS else None) for n in bs.SECTIONS}
    P = 48 if form == 0 else 96
    offs, pos = {}, 7 * P
    for name in ("gamma_abc_g1",) + VECTORS:
        if name == "a_query":
            offs["beta_g1"] = pos
            pos += 2 * P
        offs[name] = pos + 8
        pos += 8 + COUNTS[name] * (2 * P if name == "b_g2_query" else P)
    data = bs.ser_key(key, form)
    assert pos == len(data)
    return data, offs, P


@pytest.mark.parametrize("form", [0, 1, 2])
def test_key_layout_counts_and_offsets(form):
    from celo_bls_snark_rs_amd import ffi
    data, offs, P = _layout_key(form)
    rc, out = ffi.groth16_key_layout(data, form, curve="bls12_377")
    assert rc == 0
    S = ffi.KEY_LAYOUT_SLOTS
    assert int(out[S["point_bytes"]]) == P and int(out[S["len"]]) == len(data)
    for name in COUNTS:
        assert (int(out[S[name]]), int(out[S[name] + 1])) == (COUNTS[name], offs[name]), name
    assert int(out[14]) == offs["beta_g1"] and int(out[15]) == 4 + 2 + sum(COUNTS.values())
    # a compressed VerifyingKey with k gamma_abc entries is 7 * 48 + 8 + 48 k bytes
    if form == 0:
        assert offs["beta_g1"] == 7 * 48 + 8 + 48 * COUNTS["gamma_abc_g1"]
    # the same bytes are no key of the other point size, and no BW6-761 key
    assert ffi.groth16_key_layout(data, 0 if form else 1, curve="bls12_377")[0] != 0
    assert ffi.groth16_key_layout(data, form, curve="bw6_761")[0] != 0
    for bad_form in (-1, 3):
        assert ffi.groth16_key_layout(data, bad_form, curve="bls12_377")[0] == 2


@pytest.mark.parametrize("form", [0, 1])
def test_key_layout_rejections(form):
    from celo_bls_snark_rs_amd import ffi

    def layout(d):
        return ffi.groth16_key_layout(d, form, curve="bls12_377")[0]
    data, offs, P = _layout_key(form)
    # every section border: the end of each fixed point, each length field and each vector
    bounds = {P, 3 * P, 5 * P, 7 * P, offs["beta_g1"], offs["beta_g1"] + P, offs["beta_g1"] + 2 * P}
    for name in COUNTS:
        bounds |= {offs[name] - 8, offs[name], offs[name] + COUNTS[name] * (2 * P if name == "b_g2_query" else P)}
    bounds.discard(len(data))
    for b in sorted(bounds):
        for cut in (b, b - 1, b + 1):
            if 0 <= cut < len(data):
                assert layout(data[:cut]) == ffi.KEY_ERR_TRUNCATED, cut
    assert layout(b"") == ffi.KEY_ERR_TRUNCATED
    assert layout(data + b"\x00") == ffi.KEY_ERR_TRAILING
    for name in ("a_query", "b_g2_query"):
        at = offs[name] - 8
        size = 2 * P if name == "b_g2_query" else P

        def with_len(n):
            return data[:at] + n.to_bytes(8, "little") + data[at + 8:]
        assert layout(with_len(1 << 61)) == ffi.KEY_ERR_LENGTH, name           # count * size does not fit 64 bits
        assert layout(with_len((1 << 64) - 1)) == ffi.KEY_ERR_LENGTH, name
        past = (len(data) - offs[name]) // size + 1                              # one point more than the bytes left
        assert layout(with_len(past)) == ffi.KEY_ERR_TRUNCATED, name
        assert layout(with_len(COUNTS[name])) == 0


def test_serialized_key_size_matches_the_serializer():
    from celo_bls_snark_rs_amd import ffi
    for n_inputs, n_vars, n_h in ((1, 1, 0), (2, 5, 7), (3, 70, 63)):
        key = {n: None for n in bs.SECTIONS}
        key.update(gamma_abc_g1=[None] * n_inputs, a_query=[None] * n_vars, b_g1_query=[None] * n_vars, b_g2_query=[None] * n_vars,
                   h_query=[None] * n_h, l_query=[None] * (n_vars - n_inputs))
        for form in (0, 1):
            assert ffi.groth16_serialized_key_size(n_inputs, n_vars, n_h, form, curve="bls12_377") == len(bs.ser_key(key, form))
            assert ffi.groth16_serialized_key_size(n_inputs, n_vars, n_h, form, vk_only=True, curve="bls12_377") == len(bs.ser_key(key, form, bs.SECTIONS[:5]))
    assert ffi.groth16_serialized_key_size(2, 0, 0, 0, vk_only=True, curve="bls12_377") == 7 * 48 + 8 + 48 * 2
    for args in ((0, 4, 4, 0), (5, 4, 4, 0), (2, 4, 4, 2)):                     # no inputs, more inputs than variables, no such form to write
        with pytest.raises(ffi.KeySerializeError) as e:
            ffi.groth16_serialized_key_size(*args, curve="bls12_377")
        assert e.value.code == 2


def decode(ht, g2, data, check):
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    n = buf.size // (192 if g2 else 96)
    out = np.full((n, 24 if g2 else 12), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)      # every row is written, rejected ones with zeros
    st = np.full(n, 0xEE, dtype=np.uint8)
    ht.ht_wire377_decode_uncompressed(C.c_int(g2), C.c_int(check), buf.ctypes.data_as(C.c_void_p), C.c_size_t(n), out.ctypes.data_as(C.c_void_p),
                                      st.ctypes.data_as(C.c_void_p))
    return out, st


@pytest.mark.parametrize("check", [1, 0], ids=["checked", "unchecked"])
@pytest.mark.parametrize("g2", [0, 1], ids=["g1", "g2"])
def test_decode_uncompressed_against_the_rules(ht, g2, check):
    cases = bs.uncompressed_cases(g2)
    want_st, want_rows = bs.uncompressed_expected(g2, check)
    for (name, _, want), st in zip(cases, want_st):
        assert st == want[0 if check else 1], name                                # the restated rules give what the construction says
    out, st = decode(ht, g2, b"".join(data for _, data, _ in cases), check)
    for i, (name, _, _) in enumerate(cases):
        assert st[i] == want_st[i] and np.array_equal(out[i], want_rows[i]), (name, st[i], want_st[i])
    assert set(want_st.tolist()) == ({0, 1, 2, 3} if check else {0, 1, 2})
    # an unchecked off-curve pair comes back as written; a row is all zero unless its status is 0
    assert not out[st != 0].any() and out[st == 0].any(axis=1).all()
