"""Epoch blocks for the tests of the epoch encoder (csrc/epoch.h, csrc/unit_epoch.hip): a pool of keys, the case list, the oracle's bytes,
digests and public inputs for every case (oracle/py/epoch.py) and the arrays the library takes.  No GPU import at module level.

A case is (index, round, epoch_entropy, parent_entropy, maximum_non_signers, maximum_validators, key ids).  A key id k >= 0 is the pool key
(k + 2) G2; IDENTITY is the point at infinity, which the reference encodes as arkworks' zero() = (0, 1).  Expected bytes are computed once per
distinct (case, kind) and cached: large batches repeat a small pool of blocks."""
import hashlib
import numpy as np
from oracle.py import ecc
from oracle.py import epoch as ep
from oracle import cpu_oracle as co

IDENTITY = -1
KINDS = ("first", "last", "inner", "legacy")
HEADER_BITS = {"first": 176, "last": 176, "inner": 256, "legacy": 48}
U16, U8, U32 = 0xFFFF, 0xFF, 0xFFFFFFFF
MAX_KEYS = 1 << 16

_POOL = [None]          # _POOL[k] = (k + 2) G2, grown by additions
_SER = {}


def pool_key(k):
    if k == IDENTITY:
        return None
    if _POOL[0] is None:
        _POOL[0] = ecc.E2_377.add(ecc.G2_377, ecc.G2_377)
    while len(_POOL) <= k:
        _POOL.append(ecc.E2_377.add(_POOL[-1], ecc.G2_377))
    return _POOL[k]


def pool_bytes(k):
    if k not in _SER:
        _SER[k] = ecc.ser_point(ecc.E2_377, pool_key(k))
    return _SER[k]


def entropy(seed):
    """16 bytes from a seed; None stays None (an absent entropy)"""
    return None if seed is None else hashlib.sha256(b"entropy %d" % seed).digest()[:16] if seed else bytes(16)


class Case:
    def __init__(self, index, round_, ee, pe, mns, maxv, keys):
        self.index, self.round, self.ee, self.pe, self.mns, self.maxv, self.keys = index, round_, ee, pe, mns, maxv, tuple(keys)

    def ident(self):
        return (self.index, self.round, self.ee, self.pe, self.mns, self.maxv, self.keys)

    def block(self):
        return ep.EpochBlock(self.index, self.round, self.ee, self.pe, self.mns, self.maxv, [pool_key(k) for k in self.keys])

    def with_(self, **kw):
        d = dict(index=self.index, round_=self.round, ee=self.ee, pe=self.pe, mns=self.mns, maxv=self.maxv, keys=self.keys)
        d.update(kw)
        return Case(**d)


def encoded_size(kind, n_keys, maxv):
    """the size formula of include/celo_bls_amd.h, restated"""
    k = n_keys if kind == "legacy" else max(n_keys, maxv)
    bits = HEADER_BITS[kind] + 755 * (k + (1 if kind == "last" else 0))
    return (bits + 7) // 8


_EXPECT = {}


def expected(case, kind):
    """(bytes, extra or None) of the oracle for one case in one kind"""
    key = (case.ident(), kind)
    if key not in _EXPECT:
        b = case.block()
        if kind == "first":
            out = (b.encode_first_epoch_to_bytes_cip22(), None)
        elif kind == "last":
            out = (b.encode_last_epoch_to_bytes_with_aggregated_pk_cip22(), None)
        elif kind == "inner":
            out = ep.encode_inner_to_bytes_cip22(b)
        else:
            out = (b.encode_to_bytes(), None)
        _EXPECT[key] = out
    return _EXPECT[key]


def digest(data):
    return hashlib.blake2s(data, digest_size=32, person=ep.OUT_DOMAIN).digest()


def expected_inputs(first, last):
    """the two public inputs of one proof: pack(hash_first_last_epoch_block)"""
    bits = ep.hash_to_bits(expected(first, "first")[0]) + ep.hash_to_bits(expected(last, "last")[0])
    return ep.pack(bits)


def inputs_limbs(pairs):
    """(m, 2, 6) uint64 canonical limbs of the oracle's inputs for (first, last) pairs"""
    return co.ints_to_limbs([v for f, l in pairs for v in expected_inputs(f, l)], 6).reshape(len(pairs), 2, 6)


# ---- the arrays of celo_epoch_blocks
def arrays(cases, keys_form=0, null_entropy=False, spoil=None):
    """dict of the arrays for ffi.EpochBlocks.  keys_form 0: compressed keys; 1: affine rows + flags.  null_entropy: both entropy arrays None
    (every case must have none).  spoil: {(case position, key position): 96 bytes} replaces a compressed key."""
    z = bytes(16)
    key_off = np.zeros(len(cases) + 1, dtype=np.uint32)
    key_off[1:] = np.cumsum([len(c.keys) for c in cases])
    ids = [k for c in cases for k in c.keys]
    if keys_form == 0:
        enc = [pool_bytes(k) for k in ids]
        for (ci, ki), raw in (spoil or {}).items():
            enc[int(key_off[ci]) + ki] = raw
        keys = np.frombuffer(b"".join(enc), dtype=np.uint8).reshape(-1, 96) if ids else np.zeros((0, 96), dtype=np.uint8)
        inf = None
    else:
        keys, inf = co.pack_g2_377([pool_key(k) for k in ids]) if ids else (np.zeros((0, 24), dtype=np.uint64), np.zeros(0, dtype=np.uint8))
    if null_entropy:
        assert all(c.ee is None and c.pe is None for c in cases)
    return dict(index=[c.index for c in cases], round_=[c.round for c in cases], max_non_signers=[c.mns for c in cases], max_validators=[c.maxv for c in cases],
                epoch_entropy=None if null_entropy else np.frombuffer(b"".join(c.ee or z for c in cases), dtype=np.uint8).reshape(-1, 16),
                parent_entropy=None if null_entropy else np.frombuffer(b"".join(c.pe or z for c in cases), dtype=np.uint8).reshape(-1, 16),
                keys=keys, key_off=key_off, keys_form=keys_form, keys_inf=inf)


# ---- the case list
def small_cases():
    """n_keys 0 .. 9 (755 = 3 mod 8: every bit alignment), maximum_validators below / equal / above / 0, entropies absent / zero / random, the
    integer fields at 0 and at their maxima, a duplicate key and an identity key"""
    out = []
    for n in range(10):
        keys = list(range(n))
        maxv = (0, n, n + 1, max(0, n - 1), n + 3)[n % 5]
        ee, pe = (None, 0, 7 + n)[n % 3], (11 + n, None, 0)[n % 3]
        out.append(Case((0, U16, 120 + n)[n % 3], (0, U8, 5)[(n + 1) % 3], entropy(ee), entropy(pe), (0, U32, 3)[(n + 2) % 3], maxv, keys))
    out.append(Case(U16, U8, entropy(3), entropy(4), U32, 0, [0, 0, 1]))                    # a duplicate: the sum's doubling branch
    out.append(Case(1, 2, entropy(5), None, 1, 4, [2, IDENTITY, 3]))                         # an identity key among others
    out.append(Case(1, 2, None, None, 1, 2, [IDENTITY]))                                     # ... alone: the sum is the identity
    out.append(Case(0, 0, None, None, 0, 0, []))                                             # 22 bytes in the first form
    out.append(Case(9, 9, None, None, 9, 3, []))                                             # only padding
    return out


def null_entropy_cases():
    return [Case(5 + n, n, None, None, n, n + 1, list(range(n))) for n in (0, 1, 4)]


# Blake2s final-block borders: total lengths = 0, 1, 63 mod 64 per kind (K = max(n_keys, maximum_validators))
BORDER_K = {"first": (14, 33, 54), "last": (13, 32, 53), "inner": (20, 39, 1)}
BORDER_LEN = {"first": (1344, 3137, 5119), "last": (1344, 3137, 5119), "inner": (1920, 3713, 127)}


def border_cases(kind):
    """for each K of BORDER_K[kind]: half the positions real keys, the rest padding"""
    return [Case(300 + k, 1, entropy(k), entropy(k + 1), 2, k, list(range(k // 2))) for k in BORDER_K[kind]]


def full_case(n=150):
    return Case(4242, 3, entropy(21), entropy(22), 49, n, list(range(n)))


def reference_cases(golden):
    """the first and last block of the reference's Groth16 vector (tests/golden/reference_vectors.json) as oracle EpochBlocks and as arrays"""
    g = golden["groth16_bw6_761"]
    out = []
    for side in ("first", "last"):
        raw = bytes.fromhex(g[side + "_pubkeys"])
        out.append(dict(index=g[side]["index"], round=g[side]["round"], ee=bytes.fromhex(g[side + "_epoch_entropy"]), pe=bytes.fromhex(g[side + "_parent_entropy"]),
                        mns=g[side]["maximum_non_signers"], maxv=g[side]["maximum_validators"], raw=raw))
    return out


def reference_arrays(side, **change):
    """arrays of one reference block (a dict of reference_cases), with fields replaced"""
    s = dict(side, **change)
    n = len(s["raw"]) // 96
    return dict(index=[s["index"]], round_=[s["round"]], max_non_signers=[s["mns"]], max_validators=[s["maxv"]],
                epoch_entropy=np.frombuffer(s["ee"], dtype=np.uint8).reshape(1, 16), parent_entropy=np.frombuffer(s["pe"], dtype=np.uint8).reshape(1, 16),
                keys=np.frombuffer(s["raw"], dtype=np.uint8).reshape(-1, 96), key_off=np.array([0, n], dtype=np.uint32), keys_form=0, keys_inf=None)
