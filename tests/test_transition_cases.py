"""CPU (-m "not gpu"): the case list of tests/transition_cases.py is what it claims.  For one chain of every class the statuses the case list
demands, in both modes, are the ones the contract's steps give when each is done by an independent implementation: the keys and signatures
through the oracle's decoder, the rule's comparisons in Python from the table of include/celo_bls_amd.h, the inner encoding by
oracle/py/epoch.py, the composite CIP22 hash by tests/hash_ref.py, the sums by oracle/py/ecc.py and the products by
cpu_oracle.pairing_product_377.  And the rule the kernel runs (csrc/transitions.h, built for the host in host_test.cpp) against the same table."""
import ctypes as C
import itertools
import numpy as np
import pytest
from helpers import build_hosttest
from oracle.py import ecc
from oracle.py import epoch as ep
from oracle import cpu_oracle as co
import hash_ref as hr
import transition_cases as tc

DOMAIN = b"ULforxof"
E1, E2 = ecc.E1_377, ecc.E2_377


def rule(initial, bad_key, pred_bad_key, index, pred_index, n_keys, pred_n_keys, entropy_live, entropy_equal, signers, pred_mns, padding_selected, sig_wire, attempt):
    """the status table of the contract, statuses 0 to 9"""
    if bad_key:
        return 1
    if initial:
        return 0
    if pred_bad_key:
        return 2
    if index != pred_index + 1:
        return 3
    if n_keys != pred_n_keys:
        return 4
    if entropy_live and not entropy_equal:
        return 5
    if signers == 0 or signers < max(0, pred_n_keys - pred_mns):
        return 6
    if padding_selected:
        return 7
    if sig_wire >= 2:
        return 8
    if attempt == 255:
        return 9
    return 0


@pytest.fixture(scope="module")
def world():
    """the batch of small cases with everything the truth needs, computed once"""
    b = tc.Batch(tc.small_cases(), 11, n_keys=5, tag="cpu")
    pks = [E2.mul(ecc.G2_377, sk) for sk in b.sks]
    pool_enc = [ecc.ser_point(E2, P) for P in pks]
    keys = b.key_bytes(pool_enc)
    _, kst = co.decompress("g2", keys.tobytes())
    ko = b.key_off()
    bad = [bool((kst[ko[i]:ko[i + 1]] >= 2).any()) for i in range(b.nb)]
    # the encodings and hashes of the transitions whose keys decode
    enc = {}
    for i, k in enumerate(b.blocks):
        if b.initial[i] or bad[i]:
            continue
        blk = ep.EpochBlock(k.index, k.round, k.ee, k.pe, k.mns, k.maxv, [pks[j] for j in k.keys])
        enc[i] = ep.encode_inner_to_bytes_cip22(blk)
    order = sorted(enc)
    honest = hr.Batch("composite_cip22", DOMAIN, [enc[i][0] for i in order], [b.sign_extra(i, enc[i][1]) for i in order])
    truth = hr.Batch("composite_cip22", DOMAIN, [enc[i][0] for i in order], [enc[i][1] for i in order])
    hpts = co_unpack_g1(honest.rows()[0])
    tpts = co_unpack_g1(truth.rows()[0])
    skeys = b.sign_keys()
    signed = np.zeros((b.nb, 48), dtype=np.uint8)
    for n, i in enumerate(order):
        signed[i] = np.frombuffer(ecc.ser_point(E1, E1.mul(hpts[n], skeys[i])), dtype=np.uint8)
    sigs = b.signatures(signed)
    return dict(b=b, pks=pks, bad=bad, hash={i: (tpts[n], int(truth.rows()[1][n])) for n, i in enumerate(order)}, sigs=sigs, keys=keys)


def co_unpack_g1(xy):
    """rows of Montgomery limbs -> affine points, through the oracle's canonical form"""
    R_inv = pow(1 << 384, -1, ecc.Q377)
    out = []
    for row in np.asarray(xy, dtype=np.uint64).reshape(-1, 12):
        x = sum(int(v) << (64 * j) for j, v in enumerate(row[:6])) * R_inv % ecc.Q377
        y = sum(int(v) << (64 * j) for j, v in enumerate(row[6:])) * R_inv % ecc.Q377
        out.append((x, y))
    return out


def _product_is_one(pairs):
    g1 = [P for P, _ in pairs]
    g2 = [Q for _, Q in pairs]
    g1xy, i1 = co.pack_g1_377(g1)
    g2xy, i2 = co.pack_g2_377(g2)
    return bool(co.pairing_product_377(g1xy, i1, g2xy, i2)[1])


def _truth(w, mode):
    b, pks, bad = w["b"], w["pks"], w["bad"]
    neg_g2 = E2.neg(ecc.G2_377)
    st = [0] * b.nb
    pair = {}                                           # per clean transition: (signature, hash, apk)
    for c in range(len(b.chain_off) - 1):
        first = b.chain_off[c]
        for i in range(first, b.chain_off[c + 1]):
            k = b.blocks[i]
            if i == first:
                st[i] = rule(True, bad[i], 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
                continue
            p = b.blocks[i - 1]
            signers = sum(1 for x in p.bits if x)
            padding = (not bad[i - 1]) and any(x and j == tc.PAD for j, x in zip(p.keys, p.bits))
            sxy, sst = co.decompress("g1", w["sigs"][i].tobytes())
            att = w["hash"][i][1] if i in w["hash"] else 0
            st[i] = rule(False, bad[i], bad[i - 1], k.index, p.index, len(k.keys), len(p.keys), any(b.blocks[first].ee), k.pe == p.ee, signers, p.mns, padding,
                         int(sst[0]), att)
            if st[i] == 0:
                apk = None
                for j, x in zip(p.keys, p.bits):
                    if x:
                        apk = E2.add(apk, pks[j])
                S = None if sst[0] == 1 else co_unpack_g1(sxy)[0]
                pair[i] = (S, w["hash"][i][0], apk)
    chain_ok = []
    for c in range(len(b.chain_off) - 1):
        blocks = range(b.chain_off[c], b.chain_off[c + 1])
        held = False
        if mode == 1 and not any(st[i] for i in blocks) and len(blocks) > 1:
            total = None
            for i in blocks[1:]:
                total = E1.add(total, pair[i][0])
            held = _product_is_one([(total, neg_g2)] + [(pair[i][1], pair[i][2]) for i in blocks[1:]])
        if not held:
            for i in blocks[1:]:
                if st[i] == 0 and not _product_is_one([(pair[i][0], neg_g2), (pair[i][1], pair[i][2])]):
                    st[i] = 10
        chain_ok.append(int(not any(st[i] for i in blocks)))
    return st, chain_ok


@pytest.mark.parametrize("mode", [0, 1], ids=["each", "chain"])
def test_every_constructed_status_is_the_truth(world, mode):
    b = world["b"]
    st, chain_ok = _truth(world, mode)
    bad = [(lab, g, w) for lab, g, w in zip(b.label, st, b.status[mode]) if g != w]
    assert not bad, bad
    assert chain_ok == b.chain_ok[mode]
    # every class is there, with the status its name promises
    seen = {lab.split(": ")[1]: s for lab, s in zip(b.label, b.status[0])}
    assert set(tc.CLASSES) <= set(seen) and all(seen[c] == tc.STATUS[c] for c in tc.CLASSES)


def test_the_cancelling_pair_is_refused_twice_by_mode_0_and_accepted_by_mode_1(world):
    b = world["b"]
    rows = [i for i, lab in enumerate(b.label) if lab.endswith("cancelling pair")]
    assert len(rows) == 2 and [b.status[0][i] for i in rows] == [10, 10] and [b.status[1][i] for i in rows] == [0, 0]
    assert b.path == {0: 0, 1: 2}                      # (the chains of "wrong message" and "bit flipped" fall back)


def test_every_hash_of_the_cases_finds_a_counter(world):
    assert world["hash"] and all(c < 255 for _, c in world["hash"].values())


def test_the_batches_of_the_gpu_test_hold_65_transitions_and_every_class_at_every_position():
    batches = tc.every_class_everywhere()
    seen = set()
    for chains in batches:
        assert sum(n for n, _, _ in chains) == 65
        seen |= set(chains)
    for cls in tc.CLASSES:
        for n_tr in range(1, 10):
            for pos in range(1, n_tr + 1):
                if cls == "cancelling pair" and pos == n_tr:
                    continue
                assert (n_tr, cls, pos) in seen


# ---- the rule the kernel runs, from a host build of csrc/transitions.h
@pytest.fixture(scope="module")
def ht():
    return C.CDLL(build_hosttest())


def test_the_shared_rule_function_follows_the_table(ht):
    grid = itertools.product((0, 1), (0, 1), (0, 1), ((5, 4), (5, 5), (0, 65535), (0, 7), (65535, 65534)), ((5, 5), (5, 6), (0, 0)), (0, 1), (0, 1),
                             ((0, 2), (2, 2), (3, 2), (4, 1), (5, 0), (1, 9)), (0, 1), (0, 1, 2, 3), (0, 254, 255))
    n = 0
    for initial, bad, pbad, (idx, pidx), (nk, pnk), live, equal, (signers, mns), pad, wire, att in grid:
        f = (C.c_uint32 * 14)(initial, bad, pbad, idx, pidx, nk, pnk, live, equal, signers, mns, pad, wire, att)
        assert ht.ht_transition_status(f) == rule(initial, bad, pbad, idx, pidx, nk, pnk, live, equal, signers, mns, pad, wire, att), tuple(f)
        n += 1
    assert n > 10000


def test_the_helpers_that_gather_the_facts(ht):
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, size=(4, 16), dtype=np.uint8)
    z = np.zeros((4, 16), dtype=np.uint8)
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    ent = lambda x, i, y, j: ht.ht_transition_entropy(p(x), C.c_uint64(i), p(y), C.c_uint64(j))
    assert ent(a, 1, a, 1) == 3 and ent(a, 1, a, 2) == 2 and ent(z, 0, None, 3) == 1 and ent(None, 2, a, 0) == 0 and ent(None, 0, None, 0) == 1
    one = a.copy()
    one[2, 15] ^= 1
    assert ent(a, 2, one, 2) == 2 and ent(z, 3, one, 3) == 0
    gen = co.pack_g2_377([ecc.G2_377])[0][0]
    rows = rng.integers(0, 1 << 63, size=(6, 24), dtype=np.uint64)
    rows[3] = gen
    rows[5] = gen
    rows[5, 23] ^= np.uint64(1)                          # the last limb differs: no padding key
    inf = np.zeros(6, dtype=np.uint8)
    pad = lambda bits, k0, k1, fl=None: ht.ht_transition_padding(p(rows), p(fl), p(np.array(bits, dtype=np.uint8)), C.c_uint32(k0), C.c_uint32(k1), p(gen))
    assert pad([1, 1, 1, 1, 1, 1], 0, 6) == 1 and pad([1, 1, 1, 0, 1, 1], 0, 6) == 0 and pad([0, 0, 0, 0x80, 0, 0], 0, 6) == 1
    assert pad([1, 1, 1, 1, 1, 1], 0, 3) == 0 and pad([1, 1, 1, 1, 1, 1], 4, 6) == 0 and pad([1, 1, 1, 1, 1, 1], 3, 4) == 1
    inf[3] = 1
    assert pad([1, 1, 1, 1, 1, 1], 0, 6, inf) == 0       # a row flagged as absent is no key
