"""Circuits as data for the R1CS tests: generators, CSR packing (the layout of groth16_r1cs_load_*) and the adapter that lets the Python
restatement in tests/groth16_setup_ref.py (witness_rows, qap_at - imported, not edited) read a CSR matrix.

A case keeps a matrix as (row_ptr, col, kind) numpy arrays plus a small table of coefficients (python ints): entry e has the coefficient
table[kind[e]].  That is what makes cases of 2^22 constraints affordable; the Montgomery limbs are one fancy index of the table's."""
import random
import numpy as np
from oracle import cpu_oracle as co
import groth16_setup_ref as gs

N64 = {"bw6_761": 6, "bls12_377": 4}
CURVE_ID = {"bw6_761": 0, "bls12_377": 1}


class _Row:
    """one constraint of one matrix for groth16_setup_ref: items() yields (variable, coefficient) - a repeated variable appears twice"""
    __slots__ = ("cols", "ks")

    def __init__(self, cols, ks):
        self.cols, self.ks = cols, ks

    def items(self):
        return zip(self.cols, self.ks)


class CsrMatrix:
    """a sequence of rows over CSR arrays, made as they are read"""
    def __init__(self, row_ptr, col, kind, table):
        self.row_ptr, self.col, self.kind, self.table = row_ptr, col, kind, table

    def __len__(self):
        return len(self.row_ptr) - 1

    def row(self, j):
        lo, hi = int(self.row_ptr[j]), int(self.row_ptr[j + 1])
        t = self.table
        return _Row(self.col[lo:hi].tolist(), [t[i] for i in self.kind[lo:hi].tolist()])

    def __iter__(self):
        for j in range(len(self)):
            yield self.row(j)

    def limbs(self, p):
        """(row_ptr uint64, col uint32, val (nnz, N64) uint64 Montgomery limbs)"""
        tm = co.to_mont(self.table, p)
        return (np.ascontiguousarray(self.row_ptr, dtype=np.uint64), np.ascontiguousarray(self.col, dtype=np.uint32),
                np.ascontiguousarray(tm[self.kind]))


class Case:
    def __init__(self, curve, mats, n_vars, n_inputs, name):
        self.curve, self.p, self.mats, self.n_vars, self.n_inputs, self.name = curve, gs.FIELDS[curve], mats, n_vars, n_inputs, name
        self.m = len(mats[0])

    def csr(self):
        return [M.limbs(self.p) for M in self.mats]

    def log_n(self):
        return gs.domain_log(self.m, self.n_inputs)


def from_dicts(curve, circuit, name):
    """a circuit of groth16_setup_ref ({variable: coefficient} per row) -> Case"""
    A, B, C, n_vars, n_inputs = circuit
    p = gs.FIELDS[curve]
    mats = []
    for M in (A, B, C):
        table, where, row_ptr, col, kind = [], {}, [0], [], []
        for row in M:
            for v, k in row.items():
                k %= p
                if k not in where:
                    where[k] = len(table)
                    table.append(k)
                col.append(v)
                kind.append(where[k])
            row_ptr.append(len(col))
        mats.append(CsrMatrix(np.array(row_ptr, dtype=np.uint64), np.array(col, dtype=np.uint32), np.array(kind, dtype=np.int64), table))
    return Case(curve, mats, n_vars, n_inputs, name)


def toy(curve):
    return from_dicts(curve, gs.toy_circuit(), "toy")


def chain(curve, m):
    return from_dicts(curve, gs.squaring_chain(m), "chain(%d)" % m)


ZERO_KIND = 4


def coefficient_table(p, seed):
    """the coefficients random_r1cs draws from and their weights: 1 (40 %), p - 1 (20 %), 2, 2^77 (4 % each), zero (placed, never drawn) and 59
    uniformly random field elements (32 % together)"""
    prng = random.Random(seed)
    table = [1, p - 1, 2, 1 << 77, 0] + [prng.randrange(p) for _ in range(59)]
    weights = np.array([40, 20, 4, 4, 0] + [32 / 59.0] * 59)
    return table, weights / weights.sum()


def random_r1cs(curve, m, n_vars, n_inputs, seed, chunk, long_threshold):
    """Three random matrices (no satisfying assignment is implied: these feed the two products, not a proof).  By construction, in every matrix:
    empty rows (every 17th); a repeated column within a row (every 29th); an explicit zero coefficient (every 31st); coefficients 1, p - 1, 2,
    2^77 and uniformly random ones; column 0 in more than half of all rows and two hub columns in about a tenth each (the long lists of the
    transposes); the variable n_vars - 2 in no constraint; about 4 terms per row.  Matrix a has one row of exactly 3 chunks + 37 terms, matrix b one
    of exactly long_threshold terms (the longest list one lane sums) and c one of long_threshold + 1 (the shortest that is cut)."""
    p = gs.FIELDS[curve]
    assert n_vars >= 8 and m >= 256 and 1 <= n_inputs < n_vars - 2
    table, weights = coefficient_table(p, seed)
    rng = np.random.default_rng(seed)
    unused, hubs = n_vars - 2, (n_inputs + 1, n_vars // 2)
    j = np.arange(m)
    mats = []
    for k in range(3):
        empty = (j % 17) == 5 + k
        base = rng.integers(1, 7, size=m)
        flags = [(rng.random(m) < 0.62) & ~empty, (rng.random(m) < 0.1) & ~empty, (rng.random(m) < 0.1) & ~empty,
                 ((j % 29) == 3) & ~empty, ((j % 31) == 7) & ~empty]
        special = next(x for x in range(m // 3 + 40 * k, m) if x % 17 < 5)
        base[special] = (3 * chunk + 37, long_threshold, long_threshold + 1)[k]
        for f in flags:
            f[special] = False
        cnt = np.where(empty, 0, base + sum(f.astype(np.int64) for f in flags))
        row_ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
        nnz = int(row_ptr[-1])
        col = rng.integers(0, n_vars - 1, size=nnz)
        col[col >= unused] += 1
        kind = rng.choice(len(table), size=nnz, p=weights)
        off = row_ptr[:-1].astype(np.int64) + base
        for f, c in zip(flags[:3], (0,) + hubs):
            col[off[f]] = c
            off = off + f
        f = flags[3]
        col[off[f]] = col[row_ptr[:-1].astype(np.int64)[f]]
        off = off + f
        kind[off[flags[4]]] = ZERO_KIND
        assert np.count_nonzero(col == unused) == 0
        rows0 = np.zeros(m, dtype=bool)
        rows0[np.repeat(j, cnt)[col == 0]] = True
        assert rows0.sum() * 2 >= m, "column 0 in at least half of all rows"
        mats.append(CsrMatrix(row_ptr, col.astype(np.uint32), kind.astype(np.int64), table))
    return Case(curve, mats, n_vars, n_inputs, "random(%d, %d, %d)" % (m, n_vars, n_inputs))


def random_assignment(case, seed):
    rng = random.Random(seed)
    return [1] + [rng.randrange(case.p) for _ in range(case.n_vars - 1)]


def mont(vals, p):
    return np.ascontiguousarray(co.to_mont(vals, p))
