"""Shared by tests/test_wire_encode_host.py and tests/test_wire_encode_gpu.py: the four groups the encoders serve and the edge table of
coordinate values, with the expected bytes from oracle/py/ecc.ser_point (ark-serialize 0.1 serialize / serialize_uncompressed restated).

Rows need not be curve points: neither the encoder nor ser_point looks at the curve equation."""
import numpy as np
from oracle.py import ecc
from oracle import cpu_oracle as co


class Group:
    def __init__(self, name, ffi_group, code, curve, words, pack, gen):
        self.name, self.ffi_group, self.code, self.curve, self.words, self.pack, self.gen = name, ffi_group, code, curve, words, pack, gen
        self.q = curve.p
        self.f2 = bool(curve.f2)
        self.size = {True: (96 if words == 24 else 48), False: (192 if words == 24 else 96)}     # bytes per point by `compressed`

    def ser(self, P, compressed):
        return ecc.ser_point(self.curve, P, compressed=compressed)


def _gen761(curve, idx):
    import bw6_serial as bs
    return ecc.deser_point(curve, bs.reference_points()[idx][1])


GROUPS = {
    "g1_377": Group("g1_377", "g1", 0, ecc.E1_377, 12, co.pack_g1_377, lambda: ecc.G1_377),
    "g2_377": Group("g2_377", "g2", 1, ecc.E2_377, 24, co.pack_g2_377, lambda: ecc.G2_377),
    "g1_761": Group("g1_761", "bw6_761", 2, ecc.E1_761, 24, co.pack_761, lambda: _gen761(ecc.E1_761, 0)),
    "g2_761": Group("g2_761", "bw6_761", 2, ecc.E2_761, 24, co.pack_761, lambda: _gen761(ecc.E2_761, 1)),
}
GROUP_IDS = list(GROUPS)


def edge_points(g):
    """the edge table as python (x, y) pairs of integers below q (Fq2: pairs of pairs)"""
    q = g.q
    lo, hi = (q - 1) // 2, (q + 1) // 2
    xs = [0, 1, (1 << 28) - 1, 1 << 28, (1 << 64) - 1, 1 << 64, q - 1]
    pts = []
    if not g.f2:
        for x in xs:
            for y in (0, 1, lo, hi, q - 1):
                if (x, y) != (0, 0):
                    pts.append((x, y))
        return pts
    # y.c1 = 0: c0 decides, on either side of (q - 1) / 2; y.c1 != 0: c1 decides, with c0 on the opposite side
    ys = [(0, 0), (1, 0), (lo, 0), (hi, 0), (q - 1, 0), (q - 1, 1), (hi, lo), (lo, hi), (1, q - 1)]
    for i, x in enumerate(xs):
        for y in ys:
            for xx in ((x, 0), (0, x), (x, xs[(i + 3) % len(xs)])):
                if (xx, y) != ((0, 0), (0, 0)):
                    pts.append((xx, y))
    return pts


def flag_must_be_clear(g, P):
    """y = 0 and y = (q - 1) / 2 are not the larger of (y, -y) (Fq2: by c1 when it is not zero, else by c0)"""
    lo = (g.q - 1) // 2
    y = P[1]
    if not g.f2:
        return y in (0, lo)
    return (y[1] == 0 and y[0] in (0, lo)) or y[1] == lo


def edge_table(g):
    """-> (rows (m, words) uint64, inf (m,) uint8, points [python point or None], status (m,) uint8).  The expected bytes of entry i are
    g.ser(points[i], compressed) for status 0 / 1 and zeros for status 2."""
    pts = edge_points(g)
    rows, _ = g.pack(pts)
    rows = [r for r in rows]
    points, inf, status = list(pts), [0] * len(pts), [0] * len(pts)

    def add(row, i, P, st):
        rows.append(np.asarray(row, dtype=np.uint64)); inf.append(i); points.append(P); status.append(st)

    one = (1, 0) if g.f2 else 1
    zero = (0, 0) if g.f2 else 0
    add(g.pack([(zero, one)])[0][0], 0, (zero, one), 0)                    # (0, 1): a pair of field elements like any other
    nw = 6 if g.q == ecc.Q377 else 12
    qrow = np.tile(co.ints_to_limbs([g.q], nw)[0], g.words // nw)
    add(qrow, 0, None, 2)                                                  # every component's limbs equal q exactly
    last = g.pack([g.gen()])[0][0].copy()
    last[-nw:] = qrow[:nw]
    add(last, 0, None, 2)                                                  # ... the last component alone
    first = g.pack([g.gen()])[0][0].copy()
    first[:nw] = qrow[:nw]
    add(first, 0, None, 2)                                                 # ... the first alone
    add(np.full(g.words, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64), 0, None, 2)  # all ones
    add(g.pack([g.gen()])[0][0], 1, None, 1)                               # the identity through inf (the row's content does not matter)
    add(np.full(g.words, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64), 1, None, 1)  # ... even a row that is no field element
    add(np.zeros(g.words, dtype=np.uint64), 0, None, 1)                    # the identity through a zero row
    return np.stack(rows), np.array(inf, dtype=np.uint8), points, np.array(status, dtype=np.uint8)


def expected_bytes(g, points, status, compressed):
    """(m, size) uint8: ser_point of every entry (zeros where status is 2)"""
    size = g.size[compressed]
    out = np.zeros((len(points), size), dtype=np.uint8)
    for i, (P, st) in enumerate(zip(points, status)):
        if st != 2:
            out[i] = np.frombuffer(g.ser(P, compressed), dtype=np.uint8)
    return out
