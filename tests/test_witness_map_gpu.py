"""GPU (-m gpu): the Groth16 witness map (groth16_witness_map_bw6_761[_dev], groth16_witness_map_bls12_377[_dev]) on whole outputs
from 2 to 2^22 points.

What it replaces: R1CStoQAP::witness_map of ark-groth16 inside create_proof_no_zk (crates/epoch-snark/src/api/prover.rs:78,112): three
inverse transforms, three coset transforms, the pointwise (a b - c) / Z, one coset inverse transform.  For both fields, through the
host-pointer and the device-pointer entry, with Montgomery and with canonical output:
  - the whole h equals the oracle's (oracle/py/groth16_prover.py: witness_map), on a satisfied instance (c = a o b) and on arbitrary c;
  - on the satisfied instances from 2^16 up, h also passes the quotient identity h(tau) (tau^n - 1) = A(tau) B(tau) - C(tau) at a random
    tau (tests/ntt_checks.py; no transform of any kind involved) and h[n - 1] = 0;
  - log_n above the limit of include/celo_bls_amd.h is refused with code 2.
Every size above 2^20 needs the NTT's upper power table to hold more than 1024 entries (csrc/ntt.h).  The oracle's side (minutes of CPU
time at 2^22) is computed ahead in worker processes (tests/ntt_workers.py)."""
import ctypes as C
import random

import numpy as np
import pytest
import torch  # before the library: both must share one HIP runtime
from oracle.py import groth16_prover as gp
import ntt_workers as nw

pytestmark = pytest.mark.gpu
FIELD_NAMES = ["fr761", "fr377"]
LOG_NS = [1, 2, 5, 8, 9, 10, 11, 13, 14, 17, 18, 19, 20, 21, 22]
MAX_LOG_N = 28                                   # include/celo_bls_amd.h: log_n <= 28


def _seed(fname, log_n):
    return 31000 + 1000 * FIELD_NAMES.index(fname) + 10 * log_n


@pytest.fixture(scope="module")
def references():
    """(c, h Montgomery, h canonical) of the oracle for every case, the largest first"""
    jobs = {}
    for log_n in sorted(LOG_NS, reverse=True):
        for fname in FIELD_NAMES:
            for satisfied in (True, False):
                jobs[fname, log_n, satisfied] = nw.pool().submit(nw.witness_reference, fname, log_n, _seed(fname, log_n), satisfied)
    yield jobs
    nw.shutdown()


def _consts(F, log_n):
    k = gp.domain_constants(log_n, F.root(log_n), F.coset, field=F.p)
    return {name: F.mont1(v) for name, v in k.items()}


def _dev(x):
    return torch.from_numpy(x.view(np.int64).copy()).cuda()


@pytest.mark.parametrize("log_n", LOG_NS)
@pytest.mark.parametrize("fname", FIELD_NAMES)
def test_witness_map_whole_output(gpu, references, fname, log_n):
    F = nw.FIELDS[fname]
    n = 1 << log_n
    host, dev = (gpu.witness_map, gpu.witness_map_dev) if fname == "fr761" else (gpu.witness_map_fr377, gpu.witness_map_fr377_dev)
    consts = _consts(F, log_n)
    am, bm, _ = nw.witness_inputs(fname, log_n, _seed(fname, log_n))
    checks = []
    for satisfied in (True, False):
        cm, h_mont, h_canon = references.pop((fname, log_n, satisfied)).result()
        assert h_mont.shape == (n, F.limbs)
        for canonical, want in ((False, h_mont), (True, h_canon)):
            got = host(am, bm, cm, log_n, consts, canonical=canonical)
            assert np.array_equal(got, want), (satisfied, canonical, "host entry")
            # the device entry overwrites a with h and b, c with intermediate values: fresh copies for every call, none reused
            da, db, dc = _dev(am), _dev(bm), _dev(cm)
            dev(da.data_ptr(), db.data_ptr(), dc.data_ptr(), log_n, consts, canonical=canonical)
            torch.cuda.synchronize()
            got_dev = da.cpu().numpy().view(np.uint64)
            assert np.array_equal(got_dev, want), (satisfied, canonical, "device entry")
            if satisfied:
                assert not got_dev[n - 1].any()                                  # deg h <= n - 2
                if log_n >= 16 and not canonical:
                    checks.append(nw.Quotient(fname, am, bm, cm, got_dev, log_n, random.Random(_seed(fname, log_n)).randrange(2, F.p)))
    for check in checks:
        assert check.holds()


def test_witness_map_log_n_above_the_limit_is_refused(gpu):
    for fname in FIELD_NAMES:
        F = nw.FIELDS[fname]
        host_name = "groth16_witness_map_bw6_761" if fname == "fr761" else "groth16_witness_map_bls12_377"
        bufs = [F.random_limbs(s, 1) for s in (1, 2, 3)]
        keep = [b.copy() for b in bufs]
        k = [np.ascontiguousarray(F.mont1(v)) for v in (3, 5, 7, 11, 13, 17)]
        for log_n in (MAX_LOG_N + 1, 32):
            rc = getattr(gpu.lib(), host_name)(*[gpu._p(b) for b in bufs], C.c_uint(log_n), *[gpu._p(x) for x in k], C.c_int(0))
            assert rc == 2
            d = [_dev(b) for b in bufs]
            rc = getattr(gpu.lib(), host_name + "_dev")(*[C.c_void_p(t.data_ptr()) for t in d], C.c_uint(log_n), *[gpu._p(x) for x in k], C.c_int(0),
                                                       C.c_void_p(0))
            assert rc == 2
            assert all(np.array_equal(t.cpu().numpy().view(np.uint64), b) for t, b in zip(d, keep))
            assert all(np.array_equal(b, b0) for b, b0 in zip(bufs, keep))
