"""The CPU side of the large NTT / witness-map tests, spread over worker processes.

At 2^20 points and above the reference work is seconds to minutes of single-threaded CPU time per case (the C++ oracle's transform,
Python big-int sums of tests/ntt_checks.py, the oracle's witness map), while the GPU side takes milliseconds.  The tests hand that work
to a small pool of freshly started Python processes (they never open the GPU) and collect the results after the GPU calls.  The sums of
ntt_checks split into ranges, so one check of a large array runs on all workers at once.  Nothing here decides what is compared: the
workers only evaluate the oracle and the identities."""
import atexit
import multiprocessing
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _d in (os.path.dirname(_HERE), _HERE):
    if _d not in sys.path:
        sys.path.insert(0, _d)

from oracle.py import ecc, ntt as ontt, groth16_prover as gp   # noqa: E402
from oracle import cpu_oracle as co                             # noqa: E402
import ntt_checks as nc                                         # noqa: E402


class Field:
    def __init__(self, name, p, limbs, top_bits, root, oracle_ntt):
        self.name, self.p, self.limbs, self.top_bits, self.root, self.oracle_ntt = name, p, limbs, top_bits, root, oracle_ntt
        self.radix = 1 << (64 * limbs)                   # arkworks' Montgomery radix
        g = 2
        while pow(g, (p - 1) // 2, p) != p - 1:
            g += 1
        self.coset = g                                   # a quadratic non-residue: outside every 2^k-torsion subgroup

    def mont1(self, v):
        return co.to_mont([v % self.p], self.p)[0]

    def ints(self, arr):
        return co.limbs_to_ints(arr, self.limbs)

    def random_limbs(self, seed, n):
        """n arbitrary Montgomery residues below 2^top_bits < p (the suite's usual input)"""
        x = np.random.default_rng(seed).integers(0, 1 << 62, size=(n, self.limbs), dtype=np.int64).astype(np.uint64)
        x[:, self.limbs - 1] &= np.uint64((1 << (self.top_bits - 64 * (self.limbs - 1))) - 1)
        return x


FIELDS = {
    "fr761": Field("fr761", ecc.Q377, 6, 376, ontt.root_of_unity, co.ntt_fq377),          # Fr(BW6-761) = Fq(BLS12-377)
    "fr377": Field("fr377", ecc.R377, 4, 252, ontt.root_of_unity_fr377, co.ntt_fr253),    # Fr(BLS12-377)
}


def kinds(F, log_n, w=None, g=None):
    """the four transforms of the witness map as keyword sets of the oracle's entry (canonical integers)"""
    n = 1 << log_n
    w = F.root(log_n) if w is None else w
    g = F.coset if g is None else g
    winv, ninv, ginv = pow(w, -1, F.p), pow(n, -1, F.p), pow(g, -1, F.p)
    return {"fft": dict(omega=w), "coset_fft": dict(omega=w, coset=g), "ifft": dict(omega=winv, scale=ninv),
            "coset_ifft": dict(omega=winv, coset=ginv, coset_after=True, scale=ninv)}


def oracle_ntt(fname, x, log_n, kw):
    F = FIELDS[fname]
    return F.oracle_ntt(x, log_n, kw["omega"], kw.get("coset"), kw.get("coset_after", False), kw.get("scale"))


def oracle_ntt_seeded(fname, seed, log_n, kw):
    F = FIELDS[fname]
    return oracle_ntt(fname, F.random_limbs(seed, 1 << log_n), log_n, kw)


# ---- the pool
_pool = None
CHUNK = 1 << 17


def workers():
    try:
        cpus = len(os.sched_getaffinity(0))
    except AttributeError:
        cpus = os.cpu_count() or 2
    return max(2, min(12, cpus))


def pool():
    global _pool
    if _pool is None:
        _pool = ProcessPoolExecutor(max_workers=workers(), mp_context=multiprocessing.get_context("spawn"))
        atexit.register(shutdown)
    return _pool


def shutdown():
    global _pool
    if _pool is not None:
        _pool.shutdown(wait=True, cancel_futures=True)
        _pool = None


# ---- random-evaluation identity of one transform, split into ranges
def _w_out_sum(fname, X, r, start):
    F = FIELDS[fname]
    return nc.output_sum(F.ints(X), r, F.p, start)


def _w_in_sum(fname, x, w, rho, pre, start):
    F = FIELDS[fname]
    return nc.input_sum(F.ints(x), w, rho, F.p, pre, start)


class Identity:
    """x, X: Montgomery limb arrays (the identity is linear, so the residues are used as they are); kw: a keyword set of kinds()."""
    def __init__(self, fname, x, X, log_n, kw, r):
        F = FIELDS[fname]
        self.F, self.n, self.r, self.kw = F, 1 << log_n, r, kw
        after = kw.get("coset_after", False)
        self.pre = kw.get("coset") if not after else None
        self.post = kw.get("coset") if after else None
        rho = nc.rho_of(r, F.p, self.post)
        assert x.shape == X.shape == (self.n, F.limbs)
        ex = pool()
        self.outs = [ex.submit(_w_out_sum, fname, X[s:s + CHUNK], r, s) for s in range(0, self.n, CHUNK)]
        self.ins = [ex.submit(_w_in_sum, fname, x[s:s + CHUNK], kw["omega"], rho, self.pre, s) for s in range(0, self.n, CHUNK)]

    def holds(self):
        p = self.F.p
        lhs = sum(f.result() for f in self.outs) % p
        rhs = nc.identity_rhs(sum(f.result() for f in self.ins) % p, self.n, self.r, p, self.post, self.kw.get("scale"))
        return lhs == rhs


# ---- the witness map: the oracle's h for a seeded instance, and the quotient identity split into ranges
def witness_inputs(fname, log_n, seed):
    F = FIELDS[fname]
    n = 1 << log_n
    return F.random_limbs(seed, n), F.random_limbs(seed + 1, n), F.random_limbs(seed + 2, n)


def witness_reference(fname, log_n, seed, satisfied):
    """(c, h as Montgomery limbs, h as canonical limbs) of gp.witness_map on witness_inputs(seed); satisfied: c = a o b instead of
    the seeded c."""
    F = FIELDS[fname]
    am, bm, cm = witness_inputs(fname, log_n, seed)
    a, b = co.from_mont(am, F.p), co.from_mont(bm, F.p)
    if satisfied:
        c = [u * v % F.p for u, v in zip(a, b)]
        cm = co.to_mont(c, F.p)
    else:
        c = co.from_mont(cm, F.p)
    h = gp.witness_map(a, b, c, log_n, F.root(log_n), F.coset, field=F.p)
    return cm, co.to_mont(h, F.p), co.ints_to_limbs(h, F.limbs)


def _w_bary(fname, a, b, c, w, tau, start):
    F = FIELDS[fname]
    return nc.bary_sums(F.ints(a), F.ints(b), F.ints(c), w, tau, F.p, start)


class Quotient:
    """a, b, c, h: Montgomery limb arrays of a satisfied instance and of the witness map's output for it"""
    def __init__(self, fname, a, b, c, h, log_n, tau):
        F = FIELDS[fname]
        self.F, self.n, self.tau = F, 1 << log_n, tau
        w = F.root(log_n)
        ex = pool()
        self.hs = [ex.submit(_w_out_sum, fname, h[s:s + CHUNK], tau, s) for s in range(0, self.n, CHUNK)]
        self.bs = [ex.submit(_w_bary, fname, a[s:s + CHUNK], b[s:s + CHUNK], c[s:s + CHUNK], w, tau, s) for s in range(0, self.n, CHUNK)]

    def holds(self):
        p = self.F.p
        h_at_tau = sum(f.result() for f in self.hs) % p
        parts = [f.result() for f in self.bs]
        sums = tuple(sum(t[k] for t in parts) % p for k in range(3))
        return nc.quotient_identity_from_sums(h_at_tau, sums, self.n, self.tau, p, mont_radix=self.F.radix)
