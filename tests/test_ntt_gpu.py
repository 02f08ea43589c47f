"""GPU (-m gpu): NTT over Fr(BW6-761) through the C ABI (include/celo_bls_amd.h: ntt_bw6_761_fr[_dev]) vs the oracle.

What it replaces: ark-poly 0.1 Radix2EvaluationDomain::{fft, ifft, coset_fft, coset_ifft}_in_place inside
ark_groth16::create_proof_no_zk (called at crates/epoch-snark/src/api/prover.rs:78,112) - SURVEY.md section 8f row f3.
The reference holds no NTT vector (parity unpinned there); the oracle is the O(n^2) definition (oracle/py/ntt.py) at small
sizes and a textbook decimation-in-time restatement (oracle/cpu/capi.cpp: orc_ntt_fq377 / orc_ntt_fr253) at every size.

Coverage, for Fr(BW6-761) and Fr(BLS12-377) alike, every comparison exact and on the whole output:
  - every log_n from 0 to 22, all four transforms, host-pointer and device-pointer entry: equal to the oracle and to each other; at
    log_n 20, 21, 22 also the random-evaluation identity of tests/ntt_checks.py, which does not involve the oracle;
  - log_n 24 (fft and coset_fft, device-resident) by that identity alone: the size that needs more than two 1024-entry power tables
    twice over;
  - edge inputs at log_n 10, 16, 20: zeros, p - 1, constants, alternating signs, deltas, the top band of the field, limb boundaries;
  - the engine's state between calls (twiddle cache, grow-only buffers) and four threads on engines of their own;
  - log_n above the limit of include/celo_bls_amd.h is refused with code 2.
The older 2^20 property test (round trip, a delta, linearity at a few outputs) stays as it was.  The CPU side of the large cases (oracle
transforms, identities) runs in worker processes (tests/ntt_workers.py) while the GPU side runs here."""
import ctypes as C
import numpy as np
import pytest
import torch  # before the library: both must share one HIP runtime (torch's is loaded first everywhere else too)
from oracle.py import ecc, ntt as ontt
from oracle import cpu_oracle as co
import ntt_workers as nw

pytestmark = pytest.mark.gpu
Q = ecc.Q377


def _mont1(v):
    return co.to_mont([v % Q], Q)[0]


def _rand(rng, n):
    return [ecc.random_scalar(rng, Q) for _ in range(n)]


@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 4, 5, 7])
def test_matches_definition(gpu, log_n):
    rng = ecc.SplitMix64(100 + log_n)
    n = 1 << log_n
    w = ontt.root_of_unity(log_n)
    x = _rand(rng, n)
    X = co.from_mont(gpu.ntt(co.to_mont(x, Q), log_n, _mont1(w)), Q)
    assert X == ontt.dft(x, w)


@pytest.mark.parametrize("log_n", [6, 10, 11, 12, 13, 14, 15, 16])   # 10: 8+2, 12: 8+4, 14: 8+6, 15: 8+6+1, 16: 8+8 levels per launch
def test_all_four_transforms_match_oracle(gpu, log_n):
    """fft, ifft (omega^-1, scale n^-1), coset_fft (x_i *= g^i first), coset_ifft (x_i *= g^-i last, scale n^-1): bit-exact."""
    rng = ecc.SplitMix64(7 * log_n)
    n = 1 << log_n
    w = ontt.root_of_unity(log_n)
    winv, ninv, g = pow(w, -1, Q), pow(n, -1, Q), 15
    ginv = pow(g, -1, Q)
    x = np.random.default_rng(log_n).integers(0, 1 << 62, size=(n, 6), dtype=np.int64).astype(np.uint64)
    x[:, 5] &= np.uint64((1 << 56) - 1)                     # arbitrary Montgomery limbs below p
    for kw in (dict(), dict(coset=g), dict(omega=winv, scale=ninv), dict(omega=winv, coset=ginv, coset_after=True, scale=ninv)):
        om = kw.get("omega", w)
        got = gpu.ntt(x, log_n, _mont1(om), None if "coset" not in kw else _mont1(kw["coset"]), kw.get("coset_after", False),
                      None if "scale" not in kw else _mont1(kw["scale"]))
        want = co.ntt_fq377(x, log_n, om, kw.get("coset"), kw.get("coset_after", False), kw.get("scale"))
        assert np.array_equal(got, want), kw


def test_two_to_20_properties_device_resident(gpu):
    log_n = 20
    n = 1 << log_n
    w = ontt.root_of_unity(log_n)
    winv, ninv = pow(w, -1, Q), pow(n, -1, Q)
    rng = np.random.default_rng(20)
    x = rng.integers(0, 1 << 62, size=(n, 6), dtype=np.int64).astype(np.uint64)
    x[:, 5] &= np.uint64((1 << 56) - 1)
    d = torch.from_numpy(x.view(np.int64).copy()).cuda()
    gpu.ntt_dev(d.data_ptr(), log_n, _mont1(w))
    X = d.cpu().numpy().view(np.uint64)
    # spot-check 4 outputs against the definition restricted to them: X_j = sum_i x_i w^(ij) (host big-int arithmetic on a sparse input)
    gpu.ntt_dev(d.data_ptr(), log_n, _mont1(winv), None, False, _mont1(ninv))
    back = d.cpu().numpy().view(np.uint64)
    xc = co.from_mont(x[:64], Q)
    assert co.from_mont(back[:64], Q) == xc and co.from_mont(back[-64:], Q) == co.from_mont(x[-64:], Q)
    assert np.array_equal(back.reshape(n, 6)[1000:1100], co.to_mont(co.from_mont(x[1000:1100], Q), Q))
    # delta at position 3 -> X_j = w^(3j)
    delta = np.zeros((n, 6), dtype=np.uint64)
    delta[3] = _mont1(1)
    d2 = torch.from_numpy(delta.view(np.int64)).cuda()
    gpu.ntt_dev(d2.data_ptr(), log_n, _mont1(w))
    D = d2.cpu().numpy().view(np.uint64).reshape(n, 6)
    for j in (0, 1, 2, 12345, n - 1):
        assert co.from_mont(D[j:j + 1], Q) == [pow(w, 3 * j, Q)]
    # linearity on a slice: NTT(x + delta) - NTT(x) == NTT(delta)
    xs = co.from_mont(x[3:4], Q)[0]
    x2 = x.copy()
    x2[3] = _mont1(xs + 1)
    d3 = torch.from_numpy(x2.view(np.int64)).cuda()
    gpu.ntt_dev(d3.data_ptr(), log_n, _mont1(w))
    X2 = d3.cpu().numpy().view(np.uint64).reshape(n, 6)
    for j in (0, 5, 77777, n - 2):
        a = co.from_mont(X2[j:j + 1], Q)[0]
        b = co.from_mont(X.reshape(n, 6)[j:j + 1], Q)[0]
        assert (a - b) % Q == pow(w, 3 * j, Q)


# ------------------------------------------------------------------------------------------------ whole outputs at every size
FIELD_NAMES = ["fr761", "fr377"]
KIND_NAMES = ["fft", "coset_fft", "ifft", "coset_ifft"]
MAX_LOG_N = 28                                   # include/celo_bls_amd.h: log_n <= 28


def _entries(gpu, fname):
    return (gpu.ntt, gpu.ntt_dev) if fname == "fr761" else (gpu.ntt_fr377, gpu.ntt_fr377_dev)


def _args(F, kw):
    return (F.mont1(kw["omega"]), None if "coset" not in kw else F.mont1(kw["coset"]), kw.get("coset_after", False),
            None if "scale" not in kw else F.mont1(kw["scale"]))


def _run_host(gpu, fname, x, log_n, kw):
    return _entries(gpu, fname)[0](x, log_n, *_args(nw.FIELDS[fname], kw))


def _run_dev(gpu, fname, x, log_n, kw):
    d = torch.from_numpy(x.view(np.int64).copy()).cuda()
    _entries(gpu, fname)[1](d.data_ptr(), log_n, *_args(nw.FIELDS[fname], kw))
    torch.cuda.synchronize()
    return d.cpu().numpy().view(np.uint64)


def _seed(fname, log_n):
    return 9000 + 100 * FIELD_NAMES.index(fname) + log_n


@pytest.fixture(scope="module")
def oracle_outputs():
    """the oracle's transforms of the seeded inputs, computed ahead in worker processes from 2^17 points up (the largest first)"""
    jobs = {}
    for log_n in range(22, 16, -1):
        for fname in FIELD_NAMES:
            for kind, kw in nw.kinds(nw.FIELDS[fname], log_n).items():
                jobs[fname, log_n, kind] = nw.pool().submit(nw.oracle_ntt_seeded, fname, _seed(fname, log_n), log_n, kw)
    yield jobs
    nw.shutdown()


@pytest.mark.parametrize("log_n", list(range(23)))
@pytest.mark.parametrize("fname", FIELD_NAMES)
def test_whole_output_matches_oracle_at_every_size(gpu, oracle_outputs, fname, log_n):
    """All four transforms at every size from 1 to 2^22 points (register passes only: 3+3+2, 3+3+3 levels at 8, 9; tiles: 8+8+1 .. 8+8+6 at
    17 .. 22): the host-pointer and the device-pointer entry give the oracle's array, bit for bit.  From 2^20 up the device entry's output
    also passes the random-evaluation identity at a random r."""
    import random
    F = nw.FIELDS[fname]
    n = 1 << log_n
    x = F.random_limbs(_seed(fname, log_n), n)
    K = nw.kinds(F, log_n)
    rnd = random.Random(_seed(fname, log_n))
    got, ident = {}, {}
    for kind in KIND_NAMES:
        got[kind] = _run_dev(gpu, fname, x, log_n, K[kind])
        if log_n >= 20:
            ident[kind] = nw.Identity(fname, x, got[kind], log_n, K[kind], rnd.randrange(2, F.p))
        host = _run_host(gpu, fname, x, log_n, K[kind])
        assert np.array_equal(host, got[kind]), (kind, "host and device entry differ")
    for kind in KIND_NAMES:
        want = oracle_outputs.pop((fname, log_n, kind)).result() if log_n >= 17 else nw.oracle_ntt(fname, x, log_n, K[kind])
        assert got[kind].shape == want.shape and np.array_equal(got[kind], want), kind
    for kind, check in ident.items():
        assert check.holds(), kind


@pytest.mark.parametrize("fname", FIELD_NAMES)
def test_two_to_24_passes_the_random_evaluation_identity(gpu, fname):
    """2^24 points, device-resident, fft and coset_fft: 2^14 entries in the upper power table, 16 times the 1024 that two-level tables of
    1024 entries reach (a doubled table would still fail here).  Checked by the identity alone, on every output."""
    import random
    log_n = 24
    F = nw.FIELDS[fname]
    x = F.random_limbs(2424 + len(fname), 1 << log_n)
    K = nw.kinds(F, log_n)
    rnd = random.Random(24)
    try:
        checks = {}
        for kind in ("fft", "coset_fft"):
            X = _run_dev(gpu, fname, x, log_n, K[kind])
            assert X.shape == x.shape
            checks[kind] = nw.Identity(fname, x, X, log_n, K[kind], rnd.randrange(2, F.p))
        for kind, check in checks.items():
            assert check.holds(), kind
    finally:
        nw.shutdown()


# ------------------------------------------------------------------------------------------------ edge inputs
def _edge_inputs(F, log_n):
    """name -> (n, limbs) Montgomery limb array.  Built by tiling short patterns: no Python loop over n."""
    n, p, L = 1 << log_n, F.p, F.limbs
    rows = lambda vals: co.to_mont(vals, p)                       # values -> Montgomery limbs
    tile = lambda block: np.tile(block, (n // len(block) + 1, 1))[:n].copy()
    out = {}
    out["zeros"] = np.zeros((n, L), dtype=np.uint64)
    out["all_p_minus_1"] = tile(rows([p - 1]))
    out["constant"] = tile(rows([0x1234567 + (1 << 200)]))
    out["alternating"] = tile(rows([1, p - 1]))
    for name, pos in (("delta_0", 0), ("delta_mid", n // 2), ("delta_last", n - 1)):
        d = np.zeros((n, L), dtype=np.uint64)
        d[pos] = rows([1])[0]
        out[name] = d
    # the top band of the field, [2^376, q) resp. [2^252, r): as Montgomery residues (what the kernels load) and as values
    rng = np.random.default_rng(log_n)
    lo, width = 1 << F.top_bits, p - (1 << F.top_bits)
    band = [lo + int.from_bytes(rng.bytes(8 * L), "little") % width for _ in range(min(n, 1024))]
    assert all(lo <= v < p for v in band)
    out["top_band_residues"] = tile(co.ints_to_limbs(band, L))
    out["top_band_values"] = tile(rows(band))
    # 0, 1, p - 1, p - 2 and 2^k, 2^k - 1 at every 28-bit limb boundary of the device form (and the 64-bit ones of the caller's form)
    mix = [0, 1, p - 1, p - 2]
    for k in sorted(set(range(28, p.bit_length(), 28)) | set(range(64, p.bit_length(), 64))):
        mix += [1 << k, (1 << k) - 1]
    assert all(0 <= v < p for v in mix)
    out["limb_boundaries_residues"] = tile(co.ints_to_limbs(mix, L))
    out["limb_boundaries_values"] = tile(rows(mix))
    return out


@pytest.mark.parametrize("log_n", [10, 16, 20])
@pytest.mark.parametrize("fname", FIELD_NAMES)
def test_edge_inputs_match_oracle(gpu, fname, log_n):
    """fft and coset_ifft of the inputs a random vector never is: whole output against the oracle, and where the answer is known in closed
    form (constant input: n c at index 0; alternating +1, -1: n at index n / 2; both with canonical zero limbs everywhere else) against
    that too - the redundant difference of a butterfly has to leave to_ark as the canonical 0."""
    F = nw.FIELDS[fname]
    n, p = 1 << log_n, F.p
    K = nw.kinds(F, log_n)
    inputs = _edge_inputs(F, log_n)
    try:
        jobs = {}
        for name, x in inputs.items():
            for kind in ("fft", "coset_ifft"):
                jobs[name, kind] = nw.pool().submit(nw.oracle_ntt, fname, x, log_n, K[kind]) if log_n >= 16 else None
        for (name, kind), job in jobs.items():
            x = inputs[name]
            got = _run_dev(gpu, fname, x, log_n, K[kind])
            want = job.result() if job is not None else nw.oracle_ntt(fname, x, log_n, K[kind])
            assert np.array_equal(got, want), (name, kind)
            if kind != "fft":
                continue
            if name == "zeros":
                assert not got.any()
            if name in ("constant", "all_p_minus_1", "alternating"):
                at = n // 2 if name == "alternating" else 0
                c = 1 if name == "alternating" else co.from_mont(x[:1], p)[0]
                assert np.array_equal(got[at], F.mont1(n * c)), name
                rest = np.delete(got, at, axis=0)
                assert not rest.any(), name                       # canonical zero limbs, not p or another multiple of p
            if name == "delta_0":
                assert np.array_equal(got, np.tile(F.mont1(1), (n, 1)))
    finally:
        nw.shutdown()


# ------------------------------------------------------------------------------------------------ engine state, threads, the limit
def test_engine_state_survives_changes_of_size_and_generator(gpu):
    """One thread, one engine, no re-initialisation: the twiddle table is cached on (log_n, omega), the buffers only grow.  A stale table
    or a buffer sized for another call shows as a difference from the oracle in one of these steps."""
    fname = "fr761"
    F = nw.FIELDS[fname]
    p = F.p
    w20, w12 = F.root(20), F.root(12)
    steps = [(20, dict(omega=w20)), (4, dict(omega=F.root(4))), (20, dict(omega=pow(w20, -1, p))), (20, dict(omega=pow(w20, 3, p))),
             (12, dict(omega=w12, coset=F.coset)), (12, dict(omega=w12)), (21, dict(omega=F.root(21))), (10, dict(omega=F.root(10))),
             (20, dict(omega=w20))]
    try:
        jobs = [nw.pool().submit(nw.oracle_ntt_seeded, fname, 700 + i, log_n, kw) for i, (log_n, kw) in enumerate(steps)]
        for i, (log_n, kw) in enumerate(steps):
            x = F.random_limbs(700 + i, 1 << log_n)
            got = _run_host(gpu, fname, x, log_n, kw)
            assert np.array_equal(got, jobs[i].result()), (i, log_n)
    finally:
        nw.shutdown()


def test_four_threads_on_their_own_engines(gpu):
    """Four Python threads (the ctypes calls release the GIL), each looping over its own mix of sizes, fields and transforms: every
    thread leases its own engine from the pool, with its own twiddle cache.  Results equal the oracle's, which the single-threaded tests
    above pin the same calls to."""
    import threading
    plans = [[("fr761", 18, "fft"), ("fr377", 12, "coset_fft"), ("fr761", 9, "ifft"), ("fr761", 18, "fft"), ("fr377", 17, "coset_ifft")],
             [("fr377", 18, "coset_ifft"), ("fr377", 18, "fft"), ("fr761", 16, "coset_fft"), ("fr377", 5, "ifft"), ("fr761", 17, "ifft")],
             [("fr761", 13, "coset_ifft"), ("fr761", 17, "coset_fft"), ("fr377", 16, "fft"), ("fr761", 13, "coset_ifft"), ("fr377", 18, "ifft")],
             [("fr377", 15, "ifft"), ("fr761", 18, "coset_ifft"), ("fr761", 3, "fft"), ("fr377", 18, "coset_fft"), ("fr761", 12, "fft")]]
    cases = sorted({c for plan in plans for c in plan})
    inputs = {c: nw.FIELDS[c[0]].random_limbs(_seed(c[0], c[1]) + 50, 1 << c[1]) for c in cases}
    want = {c: nw.oracle_ntt(c[0], inputs[c], c[1], nw.kinds(nw.FIELDS[c[0]], c[1])[c[2]]) for c in cases}
    args = {c: _args(nw.FIELDS[c[0]], nw.kinds(nw.FIELDS[c[0]], c[1])[c[2]]) for c in cases}
    results, errors = [[] for _ in plans], []
    start = threading.Barrier(len(plans))

    def run(t):
        try:
            start.wait()
            for _ in range(3):
                for c in plans[t]:
                    results[t].append((c, _entries(gpu, c[0])[0](inputs[c], c[1], *args[c])))
        except BaseException as e:      # reported by the main thread
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=run, args=(t,)) for t in range(len(plans))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t, res in enumerate(results):
        assert len(res) == 3 * len(plans[t])
        for c, got in res:
            assert np.array_equal(got, want[c]), (t, c)


def test_log_n_above_the_limit_is_refused(gpu):
    """include/celo_bls_amd.h: log_n <= 28.  One more returns code 2 from both entries of both fields, before anything is allocated or
    launched (the buffers handed over are one element long and are not touched)."""
    for fname in FIELD_NAMES:
        F = nw.FIELDS[fname]
        host_name, dev_name = ("ntt_bw6_761_fr", "ntt_bw6_761_fr_dev") if fname == "fr761" else ("ntt_bls12_377_fr", "ntt_bls12_377_fr_dev")
        x = F.random_limbs(1, 1)
        keep = x.copy()
        w = np.ascontiguousarray(F.mont1(F.root(1)))
        for log_n in (MAX_LOG_N + 1, 32, 64):
            assert getattr(gpu.lib(), host_name)(gpu._p(x), C.c_uint(log_n), gpu._p(w), None, C.c_int(0), None) == 2
            d = torch.from_numpy(x.view(np.int64).copy()).cuda()
            assert getattr(gpu.lib(), dev_name)(C.c_void_p(d.data_ptr()), C.c_uint(log_n), gpu._p(w), None, C.c_int(0), None, C.c_void_p(0)) == 2
            assert np.array_equal(d.cpu().numpy().view(np.uint64), keep) and np.array_equal(x, keep)
