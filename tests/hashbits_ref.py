"""Plain-Python restatement of the HashToBits circuit's contract (csrc/hashbits.h), independent of the library's code:
  - the statement: the instance vector from the 48-byte rows through the oracle's Blake2Xs (oracle.py.hashing.direct_xof) and pack
    (oracle.py.epoch.pack), as crates/epoch-snark/src/gadgets/hash_to_bits.rs:87-145 computes it on the verifier's side;
  - a sparse R1CS evaluator over Python ints mod r;
  - a single-variable perturbation check that keeps A z, B z, C z per row and updates only the rows that hold the variable."""
import numpy as np
from oracle.py import epoch as ep
from oracle.py import hashing as hs

R377 = 0x12ab655e9a2ca55660b44d1e5c37b00159aa76fed00000010a11800000000001      # the scalar field of BLS12-377
MONT = (1 << 256) % R377
MONT_INV = pow(MONT, -1, R377)
SIG_DOMAIN = b"ULforxof"
CAP = 252


def limbs_to_ints(a):
    """(k, 4) uint64 little-endian limbs -> list of Python ints"""
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
    return [int(r[0]) | int(r[1]) << 64 | int(r[2]) << 128 | int(r[3]) << 192 for r in a]


def from_mont(a):
    return [v * MONT_INV % R377 for v in limbs_to_ints(a)]


def ints_to_mont_limbs(vals):
    out = np.zeros((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        w = v * MONT % R377
        for j in range(4):
            out[i, j] = (w >> (64 * j)) & 0xFFFFFFFFFFFFFFFF
    return out


def message_bits(row, bit_order):
    """the 384 message bits of one 48-byte row: 0 = bytes_le_to_bits_le (hash_to_bits.rs:114), 1 = bytes_le_to_bits_be (prover.rs:101)"""
    row = bytes(row)
    assert len(row) == 48
    return ep.bytes_le_to_bits_le(row, 384) if bit_order == 0 else ep.bytes_le_to_bits_be(row, 384)


def xof_bits(bits):
    """hash_to_bits_fn of the reference's test (hash_to_bits.rs:87-93): bits -> bytes (bits_le_to_bytes_le) -> DirectHasher.xof(.., 64) -> bits"""
    msg = bytes(sum(b << k for k, b in enumerate(bits[i:i + 8])) for i in range(0, len(bits), 8))
    return ep.bytes_le_to_bits_le(hs.direct_xof(SIG_DOMAIN, msg, 64), 512)


def n_inputs(m):
    return 1 + (384 * m + CAP - 1) // CAP + (512 * m + CAP - 1) // CAP


def instance(rows, bit_order=0):
    """[1] ++ pack(all message bits) ++ pack(all xof bits) as canonical ints"""
    mb, xb = [], []
    for row in rows:
        b = message_bits(row, bit_order)
        mb += b
        xb += xof_bits(b)
    return [1] + ep.pack(mb, CAP) + ep.pack(xb, CAP)


def unique_rows(val):
    """the distinct rows of a (k, 4) uint64 array and the index of every row among them (rows compared as 32-byte strings)"""
    val = np.ascontiguousarray(val, dtype=np.uint64).reshape(-1, 4)
    if val.shape[0] == 0:
        return val, np.zeros(0, dtype=np.int64)
    uniq, inv = np.unique(val.view(np.dtype((np.void, 32))).reshape(-1), return_inverse=True)
    return uniq.view(np.uint64).reshape(-1, 4), inv.reshape(-1)


class Sparse:
    """one CSR matrix with its coefficients as canonical ints (object array); the distinct Montgomery values are converted once"""
    def __init__(self, row_ptr, col, val):
        self.rp = np.asarray(row_ptr, dtype=np.int64)
        self.col = np.asarray(col, dtype=np.int64)
        val = np.ascontiguousarray(val, dtype=np.uint64).reshape(-1, 4)
        uniq, inv = unique_rows(val)
        table = np.array(from_mont(uniq) + [0], dtype=object)[:-1]
        self.coef = table[inv.reshape(-1)] if len(val) else np.zeros(0, dtype=object)
        self.rows = len(self.rp) - 1

    def matvec(self, z):
        """z: object array of ints -> object array of row sums mod r"""
        out = np.zeros(self.rows, dtype=object)
        if len(self.col):
            prod = self.coef * z[self.col]
            ne = self.rp[:-1] < self.rp[1:]
            out[ne] = np.add.reduceat(prod, self.rp[:-1][ne])
        return out % R377

    def columns(self, n_vars):
        """per variable: (rows, coefficients) holding it"""
        order = np.argsort(self.col, kind="stable")
        row_of = np.repeat(np.arange(self.rows, dtype=np.int64), np.diff(self.rp))
        cnt = np.bincount(self.col, minlength=n_vars)
        ptr = np.concatenate([[0], np.cumsum(cnt)])
        return ptr, row_of[order], self.coef[order]


class System:
    def __init__(self, n_vars, mats):
        self.n_vars = n_vars
        self.m = [Sparse(*t) for t in mats]
        self.rows = self.m[0].rows

    def products(self, z):
        zz = np.array(list(z), dtype=object)
        return [M.matvec(zz) for M in self.m]

    def unsatisfied(self, z):
        """indices of the rows with (A z)(B z) != C z"""
        a, b, c = self.products(z)
        return np.nonzero((a * b - c) % R377)[0]

    def perturbation_misses(self, z, variables, values):
        """For every variable v of `variables` and every replacement f(z[v]) of `values` (skipped where it equals z[v]): is some row left
        unsatisfied?  Returns the (v, new value) pairs after which EVERY row still holds - the list a sound system leaves empty.
        A z, B z, C z are kept per row; only the rows that hold v are updated and looked at (no other row can change)."""
        a, b, c = (list(x) for x in self.products(z))
        assert not any((x * y - w) % R377 for x, y, w in zip(a, b, c)), "the starting assignment does not satisfy the system"
        cols = [M.columns(self.n_vars) for M in self.m]
        abc = (a, b, c)
        misses = []
        for v in variables:
            touched = []
            for k in range(3):
                ptr, rows, coef = cols[k]
                touched.append((rows[ptr[v]:ptr[v + 1]], coef[ptr[v]:ptr[v + 1]]))
            rowset = set(int(r) for rows, _ in touched for r in rows)
            for f in values:
                nv = f(z[v]) % R377
                d = nv - z[v]
                if d == 0:
                    continue
                delta = {r: [0, 0, 0] for r in rowset}
                for k in range(3):
                    for r, cf in zip(*touched[k]):
                        delta[int(r)][k] += cf * d
                if not any(((a[r] + dl[0]) * (b[r] + dl[1]) - (c[r] + dl[2])) % R377 for r, dl in delta.items()):
                    misses.append((v, nv))
        return misses
