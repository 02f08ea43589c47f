"""Test-side arkworks 0.1 serialization of BLS12-377 points and of a Groth16 ProvingKey<Bls12_377> (ark-groth16 0.1 derive order), shared by
tests/test_wire377_host.py, tests/test_wire377_uncompressed_gpu.py and tests/test_groth16_key377_gpu.py.  The twin of tests/bw6_serial.py; what
differs is that the two groups have different point sizes (G1 over Fq: 48 / 96 B, G2 over Fq2: 96 / 192 B).

The reference ships no serialized ProvingKey<Bls12_377>: the layout restates ark-groth16 0.1's field order, as the loader does."""
import json
import os
import numpy as np
from oracle.py import ecc
from oracle import cpu_oracle as co

Q = ecc.Q377
E1, E2 = ecc.E1_377, ecc.E2_377
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_vectors.json")


def reference_points():
    """The reference's hash-to-curve outputs of tests/golden: [(curve, compressed bytes)], the ten G1 points (compat) and the ten G2 points"""
    h = json.load(open(GOLDEN))["hash_to_curve"]
    return [(E1, bytes.fromhex(x)) for x in h["g1_compat"]["points"]] + [(E2, bytes.fromhex(x)) for x in h["g2_noncompat"]["points"]]


def ser(curve, P, form):
    """form 0: compressed (48 / 96 B); 1 / 2: uncompressed (96 / 192 B)"""
    return ecc.ser_point(curve, P, compressed=(form == 0))


def ser_vec(curve, pts, form):
    return len(pts).to_bytes(8, "little") + b"".join(ser(curve, P, form) for P in pts)


SECTIONS = ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "gamma_abc_g1", "beta_g1", "delta_g1",
            "a_query", "b_g1_query", "b_g2_query", "h_query", "l_query")
G2_FIELDS = ("beta_g2", "gamma_g2", "delta_g2", "b_g2_query")


def ser_key(key, form, only=SECTIONS):
    """key: {section: point or list of points (python affine tuples, None = infinity)} -> bytes of ProvingKey<Bls12_377>; only: the sections
    written (SECTIONS[:5] is the VerifyingKey)"""
    out = []
    for name in only:
        c = E2 if name in G2_FIELDS else E1
        v = key[name]
        out.append(ser_vec(c, v, form) if isinstance(v, list) else ser(c, v, form))
    return b"".join(out)


def key_point_order(key):
    """[(section, index)] in serialization order: the index space of first_bad_point"""
    order = []
    for name in SECTIONS:
        v = key[name]
        order += [(name, i) for i in range(len(v))] if isinstance(v, list) else [(name, 0)]
    return order


def pack(curve, pts):
    """python affine points -> (n, 12 | 24) uint64 arkworks Montgomery rows (None -> a zero row)"""
    return (co.pack_g2_377 if curve is E2 else co.pack_g1_377)(pts)[0]


def rows_to_points(curve, rows, ark_zero=False):
    """(n, 12 | 24) uint64 arkworks Montgomery rows -> python affine points; zero rows -> None, and with ark_zero arkworks' (0, 1) too"""
    k = 2 if curve is E2 else 1
    v = co.from_mont(np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, 6), Q)
    out = []
    for i in range(0, len(v), 2 * k):
        c = v[i:i + 2 * k]
        if not any(c) or (ark_zero and c == ([0, 1] if k == 1 else [0, 0, 1, 0])):
            out.append(None)
        else:
            out.append((c[0], c[1]) if k == 1 else ((c[0], c[1]), (c[2], c[3])))
    return out


def oracle_status(curve, data, compressed, check):
    """The status rules of decompress_* / decode_uncompressed_* restated on oracle/py/ecc, in their order: (status, point).
    flags 0xC0 -> 2; the infinity flag -> 1; a component >= q -> 2 (only the last component is read without the flag bits); compressed: no
    root -> 2; uncompressed, checked: off the curve -> 2; checked: outside the subgroup -> 3; else 0."""
    k = 2 if curve.f2 else 1
    ncomp = k if compressed else 2 * k
    data = bytes(data)
    assert len(data) == 48 * ncomp
    flags = data[-1] & 0xC0
    if flags == 0xC0:
        return 2, None
    if flags & 0x40:
        return 1, None
    comps = [int.from_bytes(data[48 * i:48 * (i + 1)], "little") for i in range(ncomp)]
    comps[-1] &= (1 << 382) - 1
    if any(c >= Q for c in comps):
        return 2, None
    x = comps[0] if k == 1 else (comps[0], comps[1])
    if compressed:
        rhs = curve._add(curve._mul(curve._mul(x, x), x), curve.b)
        y = curve.f2.sqrt(rhs) if curve.f2 else ecc.sqrt_fp(rhs, Q)
        if y is None:
            return 2, None
        if ecc._y_is_positive(curve, y) != bool(flags & 0x80):
            y = curve.f2.neg(y) if curve.f2 else -y % Q
    else:
        y = comps[1] if k == 1 else (comps[2], comps[3])
        if check and not curve.on_curve((x, y)):
            return 2, None
    if check and curve.mul((x, y), curve.n) is not None:
        return 3, None
    return 0, (x, y)


def _fq_bytes(v):
    return int(v).to_bytes(48, "little")


def raw_uncompressed(curve, x, y):
    """x || y as they are (no reduction): components that are no field elements stay so"""
    return b"".join(_fq_bytes(c) for c in ((x, y) if not curve.f2 else (*x, *y)))


_CASES = {}


def uncompressed_cases(g2):
    """The case list of the uncompressed decoders for one group, made once: [(name, 96 | 192 bytes, want)] with want = (status checked,
    status unchecked) as the construction of the case fixes it by the status rules (never taken from the library)."""
    if g2 in _CASES:
        return _CASES[g2]
    from groth16_verify377_cases import off_subgroup_point
    curve, G = (E2, ecc.G2_377) if g2 else (E1, ecc.G1_377)
    nb = 192 if g2 else 96
    cases = []
    for k in (1, 2, 3, 0x1234567, ecc.R377 - 1):                                   # the generator and multiples of it
        cases.append(("gen*%x" % k, ser(curve, curve.mul(G, k), 1), (0, 0)))
    for i, (c, data) in enumerate(p for p in reference_points() if p[0] is curve):      # the reference's hash-to-curve outputs, re-encoded
        cases.append(("golden%d" % i, ser(curve, ecc.deser_point(curve, data), 1), (0, 0)))
    P = curve.mul(G, 0xC0FFEE)
    good = ser(curve, P, 1)
    cases.append(("identity", ser(curve, None, 1), (1, 1)))
    junk = bytearray(b"\xff" * nb); junk[-1] = 0x40
    cases.append(("identity over junk", bytes(junk), (1, 1)))                      # the infinity flag comes before any range check
    both = bytearray(good); both[-1] |= 0xC0
    cases.append(("both flags", bytes(both), (2, 2)))
    sign = bytearray(good); sign[-1] |= 0x80
    cases.append(("0x80 set", bytes(sign), (0, 0)))                                # ignored: the y read is the one written
    hi = bytearray(good); hi[47] |= 0x80
    cases.append(("high bit in x", bytes(hi), (2, 2)))                             # not the flag byte: the integer is >= q
    x, y = P
    if g2:
        cases += [("x.c0 = q", raw_uncompressed(curve, (Q, x[1]), y), (2, 2)), ("x.c1 = q", raw_uncompressed(curve, (x[0], Q), y), (2, 2)),
                  ("y.c0 = q", raw_uncompressed(curve, x, (Q, y[1])), (2, 2)), ("y.c1 = q", raw_uncompressed(curve, x, (y[0], Q)), (2, 2)),
                  ("y.c1 > q", raw_uncompressed(curve, x, (y[0], Q + 12345)), (2, 2)),
                  ("off curve", raw_uncompressed(curve, x, ((y[0] + 1) % Q, y[1])), (2, 0))]
    else:
        cases += [("x = q", raw_uncompressed(curve, Q, y), (2, 2)), ("y = q", raw_uncompressed(curve, x, Q), (2, 2)),
                  ("y > q", raw_uncompressed(curve, x, Q + 12345), (2, 2)), ("off curve", raw_uncompressed(curve, x, (y + 1) % Q), (2, 0))]
    for seed in (5, 6, 7):                                                         # on the curve, outside the prime-order subgroup
        cases.append(("off subgroup %d" % seed, ser(curve, off_subgroup_point(bool(g2), seed), 1), (3, 0)))
    _CASES[g2] = cases
    return cases


_EXPECTED = {}


def uncompressed_expected(g2, check):
    """(status (n,) uint8, rows (n, 12 | 24) uint64) of the case list by oracle_status, made once per (group, check)"""
    key = (g2, bool(check))
    if key not in _EXPECTED:
        curve = E2 if g2 else E1
        res = [oracle_status(curve, data, False, check) for _, data, _ in uncompressed_cases(g2)]
        st = np.array([r[0] for r in res], dtype=np.uint8)
        rows = pack(curve, [r[1] for r in res])
        st.setflags(write=False); rows.setflags(write=False)
        _EXPECTED[key] = (st, rows)
    return _EXPECTED[key]
