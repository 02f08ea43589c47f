"""CPU: pins tests/ntt_checks.py (the random-evaluation identity of a transform, the quotient identity of the witness map) on the O(n^2)
definition (oracle/py/ntt.py) at small sizes and on the C++ oracle at 2^16 - which also pins the C++ oracle beyond the sizes the O(n^2)
definition reaches - and shows that the checks reject what they have to reject: one output changed by 1, two outputs swapped, the output
scaled by a constant, a transform computed with w^3 instead of w, the coset factor applied on the wrong side, one coefficient of h
changed, a non-zero top coefficient of h.  The GPU tests (test_ntt_gpu.py, test_witness_map_gpu.py) rely on these checks above 2^19."""
import random

import numpy as np
import pytest
from oracle.py import ntt as ontt, groth16_prover as gp
from oracle import cpu_oracle as co
import ntt_checks as nc
import ntt_workers as nw

FIELD_NAMES = ["fr761", "fr377"]
KIND_NAMES = ["fft", "coset_fft", "ifft", "coset_ifft"]


def _definition(F, x, kw):
    """the four transforms by the O(n^2) definition: X_j = scale * post^j * sum_i x_i pre^i w^(i j)"""
    p, g, after = F.p, kw.get("coset"), kw.get("coset_after", False)
    v = list(x) if g is None or after else [u * pow(g, i, p) % p for i, u in enumerate(x)]
    X = ontt.dft_mod(v, kw["omega"], p)
    if g is not None and after:
        X = [u * pow(g, j, p) % p for j, u in enumerate(X)]
    s = kw.get("scale", 1)
    return [u * s % p for u in X]


def _holds(F, x, X, kw, r):
    after = kw.get("coset_after", False)
    return nc.ntt_identity_holds(x, X, kw["omega"], F.p, r, pre=None if after else kw.get("coset"), post=kw.get("coset") if after else None,
                                 scale=kw.get("scale"))


def test_batch_inverse():
    p = nw.FIELDS["fr377"].p
    rnd = random.Random(1)
    v = [rnd.randrange(1, p) for _ in range(33)] + [1, p - 1]
    assert [a * b % p for a, b in zip(v, nc.batch_inverse(v, p))] == [1] * len(v)
    assert nc.batch_inverse([], p) == []
    with pytest.raises(ZeroDivisionError):
        nc.batch_inverse([3, 0, 5], p)


@pytest.mark.parametrize("fname", FIELD_NAMES)
@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 6])
def test_identity_accepts_the_definition_and_rejects_its_neighbours(fname, log_n):
    F = nw.FIELDS[fname]
    n, p = 1 << log_n, F.p
    rnd = random.Random(10 * log_n + len(fname))
    x = [rnd.randrange(p) for _ in range(n)]
    for name, kw in nw.kinds(F, log_n).items():
        X = _definition(F, x, kw)
        r = rnd.randrange(2, p)
        assert _holds(F, x, X, kw, r), name
        for j in {0, n // 2, n - 1}:
            Y = list(X)
            Y[j] = (Y[j] + 1) % p
            assert not _holds(F, x, Y, kw, r), (name, j)
        if n >= 4:
            wrong_w = dict(kw, omega=pow(kw["omega"], 3, p))
            assert not _holds(F, x, _definition(F, x, wrong_w), kw, r), name


@pytest.mark.parametrize("fname", FIELD_NAMES)
def test_identity_accepts_the_cpp_oracle_at_two_to_16_and_rejects_wrong_outputs(fname):
    F = nw.FIELDS[fname]
    log_n, p = 16, F.p
    n = 1 << log_n
    rnd = random.Random(1600 + len(fname))
    xm = F.random_limbs(16, n)
    x = F.ints(xm)                                  # Montgomery residues used as the elements: the identity is linear
    K = nw.kinds(F, log_n)
    out = {}
    for name in KIND_NAMES:
        out[name] = F.ints(nw.oracle_ntt(fname, xm, log_n, K[name]))
        assert _holds(F, x, out[name], K[name], rnd.randrange(2, p)), name
    # ... and on the values themselves (from_mont on both sides)
    assert _holds(F, co.from_mont(xm, p), co.from_mont(nw.oracle_ntt(fname, xm, log_n, K["coset_ifft"]), p), K["coset_ifft"], rnd.randrange(2, p))
    r = rnd.randrange(2, p)
    for name in KIND_NAMES:
        X, kw = out[name], K[name]
        Y = list(X); Y[40000] = (Y[40000] + 1) % p                      # one output changed by 1
        assert not _holds(F, x, Y, kw, r), name
        Y = list(X); Y[5], Y[n - 7] = Y[n - 7], Y[5]                    # two outputs swapped
        assert not _holds(F, x, Y, kw, r), name
        assert not _holds(F, x, [3 * v % p for v in X], kw, r), name    # the whole output scaled by a constant
        wrong = F.ints(nw.oracle_ntt(fname, xm, log_n, dict(kw, omega=pow(kw["omega"], 3, p))))    # another generator of the same order
        assert not _holds(F, x, wrong, kw, r), name
    # coset on the wrong side: x_i g^i before the transform is not X_j g^j after it, in either direction
    g = K["coset_fft"]["coset"]
    after = F.ints(nw.oracle_ntt(fname, xm, log_n, dict(K["coset_fft"], coset_after=True)))
    assert not _holds(F, x, after, K["coset_fft"], r)
    assert _holds(F, x, after, dict(K["coset_fft"], coset_after=True), r)
    before = F.ints(nw.oracle_ntt(fname, xm, log_n, dict(K["coset_ifft"], coset_after=False)))
    assert not _holds(F, x, before, K["coset_ifft"], r)
    assert g != 1


@pytest.mark.parametrize("fname", FIELD_NAMES)
def test_sums_split_into_ranges(fname):
    F = nw.FIELDS[fname]
    p, n = F.p, 64
    rnd = random.Random(5)
    x = [rnd.randrange(p) for _ in range(n)]
    w, r, g = F.root(6), rnd.randrange(2, p), F.coset
    cuts = [0, 1, 17, 32, 64]
    assert sum(nc.output_sum(x[a:b], r, p, a) for a, b in zip(cuts, cuts[1:])) % p == nc.output_sum(x, r, p)
    for pre in (None, g):
        assert sum(nc.input_sum(x[a:b], w, r, p, pre, a) for a, b in zip(cuts, cuts[1:])) % p == nc.input_sum(x, w, r, p, pre)
    y, z = x[::-1], [v * 7 % p for v in x]
    parts = [nc.bary_sums(x[a:b], y[a:b], z[a:b], w, r, p, a) for a, b in zip(cuts, cuts[1:])]
    assert tuple(sum(t[k] for t in parts) % p for k in range(3)) == nc.bary_sums(x, y, z, w, r, p)


@pytest.mark.parametrize("fname", FIELD_NAMES)
@pytest.mark.parametrize("log_n", [1, 4, 16])
def test_quotient_identity_accepts_the_oracle_witness_map_and_rejects_a_changed_h(fname, log_n):
    F = nw.FIELDS[fname]
    p, n = F.p, 1 << log_n
    rnd = random.Random(77 + log_n)
    am, bm, _ = nw.witness_inputs(fname, log_n, 500 + log_n)
    a, b = co.from_mont(am, p), co.from_mont(bm, p)
    c = [u * v % p for u, v in zip(a, b)]
    w = F.root(log_n)
    h = gp.witness_map(a, b, c, log_n, w, F.coset, field=p)
    tau = rnd.randrange(2, p)
    assert h[n - 1] == 0
    assert nc.quotient_identity_holds(a, b, c, h, w, p, tau)
    # the same on Montgomery residues throughout
    assert nc.quotient_identity_holds(F.ints(am), F.ints(bm), F.ints(co.to_mont(c, p)), F.ints(co.to_mont(h, p)), w, p, tau, mont_radix=F.radix)
    for j in {0, n // 3, n - 2}:
        h2 = list(h); h2[j] = (h2[j] + 1) % p
        assert not nc.quotient_identity_holds(a, b, c, h2, w, p, tau), j
    h2 = list(h); h2[n - 1] = 1
    assert not nc.quotient_identity_holds(a, b, c, h2, w, p, tau)
    if n >= 4:
        h2 = list(h); h2[0], h2[1] = h2[1], h2[0]
        assert not nc.quotient_identity_holds(a, b, c, h2, w, p, tau)
        c2 = list(c); c2[n - 1] = (c2[n - 1] + 1) % p                   # not satisfied: a b - c is no multiple of x^n - 1
        assert not nc.quotient_identity_holds(a, b, c2, gp.witness_map(a, b, c2, log_n, w, F.coset, field=p), w, p, tau)


def test_worker_pool_gives_the_serial_answers():
    """the parallel forms used by the GPU tests (ranges summed over worker processes) against the serial functions"""
    fname, log_n = "fr377", 18
    F = nw.FIELDS[fname]
    n, p = 1 << log_n, F.p
    xm = F.random_limbs(3, n)
    K = nw.kinds(F, log_n)
    try:
        fut = nw.pool().submit(nw.oracle_ntt_seeded, fname, 3, log_n, K["coset_ifft"])
        X = nw.oracle_ntt(fname, xm, log_n, K["coset_ifft"])
        assert np.array_equal(fut.result(), X)
        r = random.Random(9).randrange(2, p)
        assert nw.Identity(fname, xm, X, log_n, K["coset_ifft"], r).holds()
        assert _holds(F, F.ints(xm), F.ints(X), K["coset_ifft"], r)
        Y = X.copy(); Y[n - 3, 0] ^= np.uint64(1)
        assert not nw.Identity(fname, xm, Y, log_n, K["coset_ifft"], r).holds()
        cm, hm, hc = nw.pool().submit(nw.witness_reference, fname, 10, 40, True).result()
        am, bm, _ = nw.witness_inputs(fname, 10, 40)
        assert co.from_mont(hm, p) == co.limbs_to_ints(hc, F.limbs)
        assert nw.Quotient(fname, am, bm, cm, hm, 10, r).holds()
        hm[5, 0] ^= np.uint64(1)
        assert not nw.Quotient(fname, am, bm, cm, hm, 10, r).holds()
    finally:
        nw.shutdown()
