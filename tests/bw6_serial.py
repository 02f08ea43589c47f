"""Test-side arkworks 0.1 serialization of BW6-761 points and of a Groth16 ProvingKey<BW6_761> (ark-groth16 0.1 derive order), shared by
tests/test_wire761_host.py, tests/test_wire761_gpu.py and tests/test_groth16_key_load_gpu.py.

The reference ships no serialized ProvingKey: past the VerifyingKey prefix (which seam_epoch.hip verify and oracle/py/epoch.parse_vk parse from the
reference's own vector) the layout below restates ark-groth16 0.1's field order, as the loader does."""
import json
import os
import numpy as np
from oracle.py import ecc
from oracle import cpu_oracle as co

Q = ecc.Q761
E1, E2 = ecc.E1_761, ecc.E2_761
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_vectors.json")


def reference_points():
    """The ten VK and proof points of the reference's Groth16 vector: [(curve, compressed bytes)]."""
    d = json.load(open(GOLDEN))["groth16_bw6_761"]
    vk, pr = bytes.fromhex(d["vk"]), bytes.fromhex(d["proof"])
    pts = [(E1, vk[0:96]), (E2, vk[96:192]), (E2, vk[192:288]), (E2, vk[288:384])]
    n = int.from_bytes(vk[384:392], "little")
    pts += [(E1, vk[392 + 96 * i:392 + 96 * (i + 1)]) for i in range(n)]
    pts += [(E1, pr[0:96]), (E2, pr[96:192]), (E1, pr[192:288])]
    return pts


def reference_vk():
    return bytes.fromhex(json.load(open(GOLDEN))["groth16_bw6_761"]["vk"])


def ser(curve, P, form):
    """form 0: compressed (96 B); 1 / 2: uncompressed (192 B)"""
    return ecc.ser_point(curve, P, compressed=(form == 0))


def ser_vec(curve, pts, form):
    return len(pts).to_bytes(8, "little") + b"".join(ser(curve, P, form) for P in pts)


SECTIONS = ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "gamma_abc_g1", "beta_g1", "delta_g1",
            "a_query", "b_g1_query", "b_g2_query", "h_query", "l_query")
G2_FIELDS = ("beta_g2", "gamma_g2", "delta_g2", "b_g2_query")


def ser_key(key, form):
    """key: {section: point or list of points (python affine tuples, None = infinity)} -> bytes of ProvingKey<BW6_761>"""
    out = []
    for name in SECTIONS:
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


def rows_to_points(rows):
    """(n, 24) uint64 arkworks Montgomery rows -> python affine points (zero rows -> None)"""
    rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, 24)
    ints = co.limbs_to_ints(rows.reshape(-1, 12), 12)
    rinv = pow(1 << 768, -1, Q)
    out = []
    for i in range(rows.shape[0]):
        x, y = ints[2 * i], ints[2 * i + 1]
        out.append(None if x == 0 and y == 0 else (x * rinv % Q, y * rinv % Q))
    return out


def oracle_status(curve, data, compressed, check):
    """oracle/py/ecc.deser_point mapped to the library's status codes: (status, point).  The oracle raises where the library returns a
    status: an AssertionError (flags 0xC0, a coordinate >= q) is 2, "not in subgroup" 3, any other ValueError (no root, off the curve) 2."""
    try:
        P = ecc.deser_point(curve, data, compressed=compressed, check_subgroup=check)
    except AssertionError:
        return 2, None
    except ValueError as e:
        return (3 if "subgroup" in str(e) else 2), None
    return (1, None) if P is None else (0, P)


def random_curve_points(curve, n, seed):
    """n random points of the curve (random x until x^3 + b is a square, random sign): almost surely outside the prime-order subgroup"""
    rng = ecc.SplitMix64(seed)
    out = []
    while len(out) < n:
        x = ecc.random_scalar(rng, Q)
        y = ecc.sqrt_fp((x * x * x + curve.b) % Q, Q)
        if y is None:
            continue
        out.append((x, y if rng.next() & 1 else (-y) % Q))
    return out


def non_residue_x(curve, seed):
    """an x < q for which x^3 + b has no square root (no point of the curve has it)"""
    rng = ecc.SplitMix64(seed)
    while True:
        x = ecc.random_scalar(rng, Q)
        if ecc.sqrt_fp((x * x * x + curve.b) % Q, Q) is None:
            return x
