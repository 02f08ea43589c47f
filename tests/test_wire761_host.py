"""CPU (-m "not gpu"): BW6-761 point decoding (csrc/wire761.h) and the layout walk of a serialized ProvingKey<BW6_761>.

- The new entry points are exported by the library.
- groth16_key_layout_bw6_761 (a host walk, no device call) on the reference's VK bytes embedded in a synthetic key: counts and offsets, and
  its rejections (truncation at every section boundary, trailing bytes, a length of 2^61, a length that points past the end).
- ht_wire761_decode, the decoding template under bounds tracking (the kernels run the same functions), against oracle/py/ecc.deser_point on
  the reference's VK and proof points, random on-curve points outside the subgroup and the malformed encodings, in all three forms."""
import ctypes as C
import numpy as np
import pytest
from oracle.py import ecc
from oracle import cpu_oracle as co
import bw6_serial as bs
from helpers import build_hosttest

NEW_SYMBOLS = ["decompress_bw6_761_g1", "decompress_bw6_761_g2", "decompress_bw6_761_g1_dev", "decompress_bw6_761_g2_dev",
               "decode_uncompressed_bw6_761_g1", "decode_uncompressed_bw6_761_g2", "groth16_key_layout_bw6_761",
               "groth16_load_key_bw6_761_serialized", "celo_amd_wire761_last_timings"]


@pytest.fixture(scope="module")
def ht():
    lib = C.CDLL(build_hosttest())
    lib.ht_wire761_decode.restype = None
    return lib


def decode(ht, curve, data, form):
    """form 0 compressed checked, 1 uncompressed checked, 2 uncompressed unchecked -> (rows (n, 24), status (n,))"""
    size = 96 if form == 0 else 192
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    n = buf.size // size
    out = np.zeros((n, 24), dtype=np.uint64)
    st = np.zeros(n, dtype=np.uint8)
    ht.ht_wire761_decode(C.c_int(1 if curve is ecc.E2_761 else 0), C.c_int(1 if form == 0 else 0), C.c_int(1 if form != 2 else 0),
                         buf.ctypes.data_as(C.c_void_p), C.c_size_t(n), out.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p))
    return out, st


def expect(curve, data, form):
    """the oracle's verdict as (status, row)"""
    st, P = bs.oracle_status(curve, data, form == 0, form != 2)
    return st, (co.pack_761([P])[0][0] if st == 0 else np.zeros(24, dtype=np.uint64))


def test_new_symbols_exported():
    from celo_bls_snark_rs_amd import ffi
    lib = C.CDLL(ffi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in ffi.EXPORTS and hasattr(lib, name), name


def _layout_key():
    """the reference VK (compressed bytes) + synthetic sections of distinct lengths; point bytes are opaque to the layout walk"""
    vk = bs.reference_vk()
    counts = {"a_query": 5, "b_g1_query": 3, "b_g2_query": 4, "h_query": 7, "l_query": 2}
    body, offs, pos = [], {}, len(vk) + 2 * 96
    for i, name in enumerate(("a_query", "b_g1_query", "b_g2_query", "h_query", "l_query")):
        n = counts[name]
        body.append(n.to_bytes(8, "little") + bytes([i + 1]) * (96 * n))
        offs[name] = pos + 8
        pos += 8 + 96 * n
    key = vk + bytes(2 * 96) + b"".join(body)
    return vk, key, counts, offs


def test_key_layout_counts_and_offsets():
    from celo_bls_snark_rs_amd import ffi
    vk, key, counts, offs = _layout_key()
    n_abc = int.from_bytes(vk[384:392], "little")
    rc, out = ffi.groth16_key_layout(key, 0)
    assert rc == 0
    S = ffi.KEY_LAYOUT_SLOTS
    assert int(out[S["point_bytes"]]) == 96 and int(out[S["len"]]) == len(key)
    assert (int(out[S["gamma_abc_g1"]]), int(out[S["gamma_abc_g1"] + 1])) == (n_abc, 392)
    for name in counts:
        assert (int(out[S[name]]), int(out[S[name] + 1])) == (counts[name], offs[name]), name
    assert int(out[14]) == len(vk) and int(out[15]) == 4 + n_abc + 2 + sum(counts.values())
    # uncompressed forms: the same walk with 192 B points
    key2 = bs.ser_key({n: ([None] * 3 if n in ("gamma_abc_g1", "a_query", "b_g1_query", "b_g2_query", "h_query", "l_query") else None)
                       for n in bs.SECTIONS}, 1)
    for form in (1, 2):
        rc, out = ffi.groth16_key_layout(key2, form)
        assert rc == 0 and int(out[0]) == 192 and int(out[15]) == 4 + 3 + 2 + 15
    assert ffi.groth16_key_layout(key2, 0)[0] != 0          # the same bytes are no compressed key
    assert ffi.groth16_key_layout(key, 3)[0] == 2            # no such form


def test_key_layout_rejections():
    from celo_bls_snark_rs_amd import ffi
    vk, key, counts, offs = _layout_key()
    # every section boundary: the end of each fixed point group, each length field and each vector
    bounds = {96, 4 * 96, 392, len(vk), len(vk) + 192}
    for name in counts:
        bounds |= {offs[name] - 8, offs[name], offs[name] + 96 * counts[name]}
    bounds.discard(len(key))
    for b in sorted(bounds):
        for cut in (b, b - 1, b + 1):
            if 0 <= cut < len(key):
                assert ffi.groth16_key_layout(key[:cut], 0)[0] == ffi.KEY_ERR_TRUNCATED, cut
    assert ffi.groth16_key_layout(b"", 0)[0] == ffi.KEY_ERR_TRUNCATED
    assert ffi.groth16_key_layout(key + b"\x00", 0)[0] == ffi.KEY_ERR_TRAILING
    a_len = offs["a_query"] - 8

    def with_len(n):
        return key[:a_len] + n.to_bytes(8, "little") + key[a_len + 8:]
    assert ffi.groth16_key_layout(with_len(1 << 61), 0)[0] == ffi.KEY_ERR_LENGTH
    assert ffi.groth16_key_layout(with_len((1 << 64) - 1), 0)[0] == ffi.KEY_ERR_LENGTH
    past = (len(key) - offs["a_query"]) // 96 + 1                          # one point more than the bytes left
    assert ffi.groth16_key_layout(with_len(past), 0)[0] == ffi.KEY_ERR_TRUNCATED
    assert ffi.groth16_key_layout(with_len(counts["a_query"]), 0)[0] == 0


def test_decode_reference_points(ht):
    for curve, data in bs.reference_points():
        out, st = decode(ht, curve, data, 0)
        want_st, want = expect(curve, data, 0)
        assert want_st == 0 and st[0] == 0 and np.array_equal(out[0], want)
        P = bs.rows_to_points(out)[0]
        for form in (1, 2):
            out2, st2 = decode(ht, curve, bs.ser(curve, P, form), form)
            assert st2[0] == 0 and np.array_equal(out2[0], want)


@pytest.mark.parametrize("curve", [ecc.E1_761, ecc.E2_761], ids=["g1", "g2"])
def test_decode_random_curve_points_all_forms(ht, curve):
    pts = bs.random_curve_points(curve, 64, 761 + (curve is ecc.E2_761))
    enc = {form: b"".join(bs.ser(curve, P, form) for P in pts) for form in (0, 1, 2)}
    got = {form: decode(ht, curve, enc[form], form) for form in (0, 1, 2)}
    rows = co.pack_761(pts)[0]
    for i, P in enumerate(pts):
        assert not curve.in_subgroup(P)                                   # the oracle confirms: outside the prime-order subgroup
        for form in (0, 1):
            assert got[form][1][i] == 3 and not got[form][0][i].any()
        assert got[2][1][i] == 0 and np.array_equal(got[2][0][i], rows[i])   # unchecked: the coordinates as they are
    # ... and the same points decoded without the subgroup test (compressed): the root and the sign flag
    unchecked = np.zeros((len(pts), 24), dtype=np.uint64)
    st = np.zeros(len(pts), dtype=np.uint8)
    ht.ht_wire761_decode(C.c_int(1 if curve is ecc.E2_761 else 0), C.c_int(1), C.c_int(0), enc[0], C.c_size_t(len(pts)),
                         unchecked.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p))
    assert (st == 0).all() and np.array_equal(unchecked, rows)


@pytest.mark.parametrize("curve", [ecc.E1_761, ecc.E2_761], ids=["g1", "g2"])
def test_decode_subgroup_points(ht, curve):
    gen = bs.reference_points()[0 if curve is ecc.E1_761 else 1]
    G = ecc.deser_point(curve, gen[1])
    pts = [curve.mul(G, k) for k in (2, 3, 0x1234567, ecc.R761 - 1)]
    for form in (0, 1, 2):
        out, st = decode(ht, curve, b"".join(bs.ser(curve, P, form) for P in pts), form)
        assert (st == 0).all() and np.array_equal(out, co.pack_761(pts)[0])


@pytest.mark.parametrize("curve", [ecc.E1_761, ecc.E2_761], ids=["g1", "g2"])
def test_decode_malformed(ht, curve):
    P = bs.random_curve_points(curve, 1, 99)[0]
    cases = []
    for form in (0, 1, 2):
        inf = bs.ser(curve, None, form)
        cases.append((form, inf, 1))
        both = bytearray(bs.ser(curve, P, form)); both[-1] |= 0xC0
        cases.append((form, bytes(both), 2))
        inf_c0 = bytearray(inf); inf_c0[-1] |= 0x80
        cases.append((form, bytes(inf_c0), 2))
        # infinity before any range check: x bytes that are no field element, with the infinity flag
        junk = bytearray(b"\xff" * (96 if form == 0 else 192)); junk[-1] = 0x40
        cases.append((form, bytes(junk), 1))
        for big in (ecc.Q761, ecc.Q761 + 12345, (1 << 760) + (1 << 759)):   # x >= q (below 2^766: the flag bits stay clear)
            enc = bytearray(bs.ser(curve, P, form)); enc[0:96] = big.to_bytes(96, "little")
            if form == 0:
                enc[95] |= bs.ser(curve, P, 0)[95] & 0x80
            cases.append((form, bytes(enc), 2))
    x = bs.non_residue_x(curve, 7)
    cases.append((0, x.to_bytes(96, "little"), 2))                           # no y for this x
    off = (P[0], (P[1] + 1) % ecc.Q761)                                      # off the curve
    for form, want in ((1, 2), (2, 0)):
        cases.append((form, off[0].to_bytes(96, "little") + off[1].to_bytes(96, "little"), want))
        cases.append((form, P[0].to_bytes(96, "little") + (P[1] + ecc.Q761).to_bytes(96, "little"), 2))   # y >= q
    for form, data, want in cases:
        out, st = decode(ht, curve, data, form)
        assert st[0] == want, (form, data.hex(), st[0], want)
        if want:
            assert not out[0].any()
        else:
            assert np.array_equal(out[0], co.pack_761([(int.from_bytes(data[:96], "little"), int.from_bytes(data[96:], "little"))])[0][0])
        # the oracle agrees wherever it has the same rule: it checks the curve equation in every form (deserialize_unchecked does not) and
        # does not range-check y in the uncompressed form
        y_big = form != 0 and int.from_bytes(data[96:191] + bytes([data[191] & 0x3F]), "little") >= ecc.Q761 and want == 2 and \
            int.from_bytes(data[:96], "little") < ecc.Q761 and data[191] & 0xC0 == 0
        if not (form == 2 and want == 0) and not y_big:
            assert bs.oracle_status(curve, data, form == 0, form != 2)[0] == want, (form, data.hex())
