"""GPU: the composed entry points that decode compressed validator keys - epoch_encode_blocks_bls12_377, epoch_public_inputs_bw6_761,
verify_epoch_proofs_bw6_761, verify_epoch_transitions_bls12_377 - with the key de-duplication switch (celo_amd_key_dedup_set) at 0 and at 1:
identical bytes, inputs, statuses and verdicts, on the case lists of tests/epoch_cases.py and tests/transition_cases.py (whole) and on batches
of 65 blocks in which an undecodable key and a key outside G2 recur in blocks 0, 31 and 64 (from a pool of 9 keys for the encoders, the
inputs and the proofs; a batch of the transition case list for the transitions).  The record (celo_amd_key_dedup_last) says which
calls de-duplicated.  Every test leaves the switch at -1.

NOT covered here: more than one device; one table across the first and the last blocks of a proof batch (they are two stages, two tables)."""
import numpy as np
import pytest
import torch  # noqa: F401  (before the library: torch brings its own HIP runtime; loaded after the library's, it finds no device)
import dedup_ref as R
import epoch_cases as EC
import test_epoch_gpu as TE
import test_transitions_gpu as TT
from test_epoch_gpu import key2, vk2, proof_pool  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
BAD_BLOCKS = (0, 31, 64)


def switched(gpu, f):
    """f() under the switch at 0 and at 1: (result at 0, result at 1, record before, record after 0, record after 1)"""
    try:
        gpu.decompress_dedup("g2", EC.pool_bytes(0) + EC.pool_bytes(1))           # the record at (2, 2)
        rec = gpu.key_dedup_last()
        assert rec[:2] == (2, 2)
        gpu.key_dedup_set(0)
        off = f()
        rec0 = gpu.key_dedup_last()
        gpu.key_dedup_set(1)
        on = f()
        rec1 = gpu.key_dedup_last()
    finally:
        gpu.key_dedup_set(-1)
    return off, on, rec, rec0, rec1


def same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


def batch65():
    """65 blocks of 5 keys from a pool of 9; an undecodable key and a key outside G2 in blocks 0, 31 and 64"""
    cases = [EC.Case(500 + b, b % 7, EC.entropy(b + 1), EC.entropy(b + 2), b % 3, 5 + b % 2, [(b + j) % 9 for j in range(5)]) for b in range(65)]
    spoil = {}
    for n, b in enumerate(BAD_BLOCKS):
        spoil[(b, n)] = TE.UNDECODABLE
        spoil[(b, 3 - n)] = TE.OUTSIDE_G2
    return cases, spoil


def test_encodings_in_all_four_kinds(gpu):
    lists = [(EC.small_cases() + [c for k in EC.BORDER_K for c in EC.border_cases(k)], None), batch65()]
    for cases, spoil in lists:
        b = TE.blocks(gpu, cases, spoil=spoil)
        for kind in EC.KINDS:
            off, on, rec, rec0, rec1 = switched(gpu, lambda: gpu.epoch_encode_blocks(b, kind)[:3])
            assert same(off, on), kind
            assert rec0 == rec                                        # at 0 the record is not updated; at 1 it is
            n_keys = sum(len(c.keys) for c in cases)
            assert rec1[0] == n_keys and rec1[1] < n_keys
            if spoil:
                data, _, status = on
                assert status.tolist() == [1 if i in BAD_BLOCKS else 0 for i in range(65)]
                assert all(any(d) != (i in BAD_BLOCKS) for i, d in enumerate(data))
                assert rec1[:2] == (325, 11)                          # the pool's 9 keys and the two bad ones
            else:
                assert not on[2].any() and [d for d in on[0]] == [EC.expected(c, kind)[0] for c in cases]


def test_public_inputs(gpu):
    pairs = TE.pair_pool()
    bf, bl = TE.blocks(gpu, [f for f, _ in pairs]), TE.blocks(gpu, [l for _, l in pairs])
    off, on, rec, rec0, rec1 = switched(gpu, lambda: gpu.epoch_public_inputs(bf, bl))
    assert same(off, on) and not on[1].any() and np.array_equal(on[0], EC.inputs_limbs(pairs)) and rec0 == rec
    cases, spoil = batch65()
    last_spoil = {(b, k): raw for (b, k), raw in spoil.items() if b != 31}
    bf, bl = TE.blocks(gpu, cases, spoil=spoil), TE.blocks(gpu, cases[::-1], spoil={(64 - b, k): raw for (b, k), raw in last_spoil.items()})
    off, on, rec, rec0, rec1 = switched(gpu, lambda: gpu.epoch_public_inputs(bf, bl))
    assert same(off, on) and rec0 == rec and rec1[0] == 325 and rec1[1] < 325
    assert on[1].tolist() == [1 if i in BAD_BLOCKS else 0 for i in range(65)]           # (blocks 0 and 64 are bad on both sides: the first side is named)


def test_verdicts_of_the_epoch_proofs_in_both_modes(gpu, vk2, proof_pool):
    for rotation in (0, 3):
        firsts, lasts, sf, sl, proofs, classes = TE._status_batch(proof_pool, 65, rotation)
        bf, bl = TE.blocks(gpu, firsts, spoil=sf), TE.blocks(gpu, lasts, spoil=sl)
        for mode in (0, 1):
            off, on, rec, rec0, rec1 = switched(gpu, lambda: gpu.verify_epoch_proofs(vk2, proofs, bf, bl, mode=mode, key=TE.KEY8))
            assert same(off, on) and on[1].tolist() == classes and on[0].tolist() == [1 if c == 0 else 0 for c in classes], (rotation, mode)
            assert rec0 == rec and rec1[0] in (sum(len(c.keys) for c in lasts), sum(len(c.keys) for c in firsts)) and rec1[1] < rec1[0]


@pytest.mark.parametrize("group", range(TT.GROUPS))
def test_verdicts_of_the_transitions_in_both_modes_with_every_optional_output(gpu, group):
    """the whole case list of tests/transition_cases.py (every class at every position, 65 transitions a call; the worlds are those of
    tests/test_transitions_gpu.py, built once per session)"""
    for n, chains in enumerate(TT.BATCHES):
        if n % TT.GROUPS != group:
            continue
        b, blocks, sigs, _, _ = TT._world(gpu, tuple(chains), 1000 + n)
        for mode in (0, 1):
            off, on, rec, rec0, rec1 = switched(gpu, lambda: TT._run(gpu, b, blocks, sigs, mode))
            assert same(off, on), (n, mode)
            assert all(on[k] is not None for k in ("ok", "status", "chain_ok", "crh", "attempts", "asig_xy", "asig_inf"))
            TT._check(b, on, mode, chain_ok=b.chain_ok[mode])
            assert rec0 == rec and rec1[0] == int(b.key_off()[-1]) and rec1[1] < rec1[0]


def test_transitions_of_65_blocks_with_recurring_bad_keys(gpu):
    """a batch of the case list with an undecodable key and a key outside G2 written into blocks 0, 31 and 64: the same statuses, verdicts
    and optional outputs under the switch at 0 and 1; the spoiled blocks are refused, and the table decodes the two bad keys once each"""
    b, blocks, sigs, _, _ = TT._world(gpu, tuple(TT.BATCHES[0]), 1000)
    assert b.nb >= 65
    keys, ko = b.key_bytes(TT._pool()[1]).copy(), b.key_off()
    for blk in BAD_BLOCKS:
        assert ko[blk + 1] - ko[blk] >= 2
        keys[ko[blk]] = np.frombuffer(TE.UNDECODABLE, dtype=np.uint8)
        keys[ko[blk + 1] - 1] = np.frombuffer(TE.OUTSIDE_G2, dtype=np.uint8)
    spoiled = gpu.EpochBlocks(keys=keys, key_off=ko, **b.fields())
    for mode in (0, 1):
        off, on, rec, rec0, rec1 = switched(gpu, lambda: TT._run(gpu, b, spoiled, sigs, mode))
        assert same(off, on), mode
        assert all(on["status"][blk] != 0 and on["ok"][blk] == 0 for blk in BAD_BLOCKS)
        assert rec0 == rec and rec1[0] == int(ko[-1]) and rec1[1] == R.first_occurrence(keys)[1]


def big_blocks(gpu, total):
    """blocks of up to 4096 keys, `total` keys in all, from a pool of 9"""
    pool = np.frombuffer(b"".join(EC.pool_bytes(k) for k in range(9)), dtype=np.uint8).reshape(9, 96)
    sizes = [4096] * (total // 4096) + ([total % 4096] if total % 4096 else [])
    key_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    nb = len(sizes)
    return gpu.EpochBlocks(np.arange(nb) % 60000, np.zeros(nb, dtype=np.uint8), np.zeros(nb, dtype=np.uint32), np.array(sizes, dtype=np.uint32), None, None,
                           np.ascontiguousarray(pool[np.arange(total) % 9]), key_off)


def test_the_rule_decides_by_the_number_of_keys(gpu):
    """the switch at -1: a call below N0 leaves the record alone, one at or above it updates it; N0 = 0 is "never" """
    assert gpu.key_dedup_get()[0] == -1
    sizes = [(1024, False)] if R.N0 == 0 else [(R.N0 - 1, False), (R.N0, True)]
    for total, dedup in sizes:
        gpu.decompress_dedup("g2", EC.pool_bytes(0) + EC.pool_bytes(1))           # the record at (2, 2)
        _, _, status, _ = gpu.epoch_encode_blocks(big_blocks(gpu, total), "legacy")
        assert not status.any()
        assert gpu.key_dedup_last()[:2] == ((total, 9) if dedup else (2, 2)), total
