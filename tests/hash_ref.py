"""The reference side of the hash-to-G1 tests (tests/test_hash_gpu.py, tests/test_hash_host.py): the four try-and-increment modes of
csrc/hash_direct.h restated over the Python oracle, and their evaluation for whole batches on the worker processes of tests/ntt_workers.py.

  direct           TryAndIncrement<DirectHasher>:      candidate c = xof(crh(c || extra || message))
  tail             the CIP22 loop alone:               candidate c = xof(c || extra || inner), `message` being the inner bytes
  composite        TryAndIncrement<CompositeHasher>:   candidate c = xof(pedersen_crh(c || extra || message))
  composite_cip22  TryAndIncrementCIP22:               inner = pedersen_crh(message) once, then the tail

Everything is built from oracle/py/hashing.py (direct_crh, direct_xof, _candidate_to_point), oracle/py/composite.py (composite_crh) and
ecc.E1_377.mul; tests/test_hash_host.py pins reference() to hs.hash_to_g1 (which tests/test_oracle_golden.py pins on the reference's own
vectors) for the three modes the oracle has an entry for, and the tail through composite_cip22.  No tests in this file; nothing here
decides what is compared."""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _d in (os.path.dirname(_HERE), _HERE):
    if _d not in sys.path:
        sys.path.insert(0, _d)

from oracle.py import ecc, hashing as hs          # noqa: E402
from oracle.py import composite as comp           # noqa: E402
from oracle import cpu_oracle as co               # noqa: E402

MODES = ("direct", "tail", "composite", "composite_cip22")
XOF_BYTES = hs.hash_length(48)                    # 64: the XOF length the try-and-increment loops ask for
PEDERSEN_MAX_BYTES = comp.WINDOW_SIZE * comp.NUM_WINDOWS * 3 // 8     # 19 530: the longest string the generator table covers


def _loop(domain, extra, inner, crh):
    """the candidates xof(crh(c || extra || inner)) (crh None: no CRH per attempt) until one selects a point with a cofactor multiple"""
    for c in range(255):
        pre = bytes([c]) + extra + inner
        cand = hs.direct_xof(domain, pre if crh is None else crh(pre), XOF_BYTES)[:48]
        P = hs._candidate_to_point(cand)
        if P is None or P == "zero":
            continue
        S = ecc.E1_377.mul(P, ecc.H1_377)
        if S is None:
            continue
        return S, c
    raise ValueError("HashToCurveError")


def reference(mode, domain, message, extra):
    """-> (affine point of G1, attempt counter)"""
    if mode == "direct":
        return _loop(domain, extra, message, lambda b: hs.direct_crh(domain, b, XOF_BYTES))
    if mode == "tail":
        return _loop(domain, extra, message, None)
    if mode == "composite":
        return _loop(domain, extra, message, comp.composite_crh)
    if mode == "composite_cip22":
        return _loop(domain, extra, comp.composite_crh(message), None)
    raise ValueError(mode)


# ---- the length grids of the streamed modes (shared by the GPU tests and the host build's)
def rand_bytes(rng, n):
    return bytes(rng.integers(0, 256, size=n, dtype=np.uint8))


def tail_length_grid(rng):
    """(inner, extra) of the CIP22 tail: the deployed 48-byte inner with extras of every length 0 ... 80 (counter || extra || inner of
    49 ... 129 bytes: across the 64-byte Blake2s block, 15 and 79 ending on one exactly), then the inner lengths the ABI also accepts"""
    grid = [(rand_bytes(rng, 48), rand_bytes(rng, e)) for e in range(81)]
    for l in (0, 1, 15, 62, 63, 64, 65, 127, 128, 200):
        grid += [(rand_bytes(rng, l), b""), (rand_bytes(rng, l), rand_bytes(rng, 1 + l % 5))]
    return grid


def composite_length_grid(rng):
    """(message, extra) of the composite modes: the counter byte and the extra shift every later 3-bit chunk, so with extras of 0, 1, 7 and
    32 bytes the chunk boundaries of the message fall on all three residues"""
    return [(rand_bytes(rng, m), rand_bytes(rng, e)) for m in (0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 100) for e in (0, 1, 7, 32)]


# ---- whole batches on the worker pool
def _w_batch(mode, domain, msgs, extras):
    pts, att = [], []
    for m, e in zip(msgs, extras):
        P, c = reference(mode, domain, m, e)
        pts.append(P)
        att.append(c)
    return co.pack_g1_377(pts)[0], np.array(att, dtype=np.uint8)


def _w_crh(msgs):
    return [comp.composite_crh(m) for m in msgs]


def _chunks(n, per):
    import ntt_workers as nw
    per = per or max(1, min(512, -(-n // (4 * nw.workers()))))
    return [(s, min(n, s + per)) for s in range(0, n, per)]


class Batch:
    """reference() of every (message, extra) pair, started at once on the pool; rows() waits: (xy (n, 12) uint64 Montgomery limbs as the
    library returns them, attempts (n,) uint8).  per: pairs per task (default: about four tasks per worker, at most 512 pairs each)."""
    def __init__(self, mode, domain, msgs, extras=None, per=None):
        import ntt_workers as nw
        assert mode in MODES
        self.n = len(msgs)
        extras = [b""] * self.n if extras is None else extras
        ex = nw.pool()
        self.futs = [ex.submit(_w_batch, mode, domain, msgs[a:b], extras[a:b]) for a, b in _chunks(self.n, per)]
        self._rows = None

    def rows(self):
        if self._rows is None:
            parts = [f.result() for f in self.futs]
            self._rows = (np.concatenate([p[0] for p in parts]) if parts else np.zeros((0, 12), dtype=np.uint64),
                          np.concatenate([p[1] for p in parts]) if parts else np.zeros(0, dtype=np.uint8))
        return self._rows


class CrhBatch:
    """composite_crh of every message on the pool; hashes() waits: a list of 48-byte strings"""
    def __init__(self, msgs, per=None):
        import ntt_workers as nw
        ex = nw.pool()
        self.futs = [ex.submit(_w_crh, msgs[a:b]) for a, b in _chunks(len(msgs), per)]

    def hashes(self):
        return [h for f in self.futs for h in f.result()]


# ---- the schedule of rounds (csrc/unit_hash.hip: hash_to_g1_direct_run), from reference counters
LANE_BUDGET_LOG, MAX_WIDTH_LOG = 17, 4


def round_widths(attempts):
    """[(width, open messages, first counter)] of the rounds a call runs for messages with these attempt counters: every round gives each open message
    `width` adjacent counters from `base`, the widest power of two up to 16 with open * width <= 2^17; a message closes in the round
    that covers its counter."""
    att = np.sort(np.asarray(attempts, dtype=np.int64))
    rounds, base = [], 0
    while True:
        count = int(len(att) - np.searchsorted(att, base, side="left"))        # counters >= base are still open
        if count == 0 or base >= 255:
            return rounds
        log = 0
        while log < MAX_WIDTH_LOG and (count << (log + 1)) <= (1 << LANE_BUDGET_LOG):
            log += 1
        rounds.append((1 << log, count, base))
        base += 1 << log
