"""GPU: verify_epoch_transitions_bls12_377 (csrc/unit_transitions.hip) on the cases of tests/transition_cases.py, whose verdicts
tests/test_transition_cases.py proves on the CPU.  Keys are made with fixed_base_mul_bls12_377_g2, signatures with sign_batch_bls12_377
(composite CIP22) over the library's own inner encodings (epoch_encode_blocks_bls12_377, which tests/test_epoch_gpu.py holds to the oracle);
statuses, verdicts, chain verdicts and the path are compared whole, in both modes.
NOT covered: more than one device; a hash that exhausts its counters (no findable input)."""
import ctypes as C
import functools
import threading
import numpy as np
import pytest
import torch  # before the library: both must share one HIP runtime
from oracle.py import ecc
from oracle import cpu_oracle as co
import transition_cases as tc

pytestmark = pytest.mark.gpu
NEG_G2 = co.pack_g2_377([ecc.E2_377.neg(ecc.G2_377)])[0][0]
G2_ROW = co.pack_g2_377([ecc.G2_377])[0][0]
E1 = ecc.E1_377


@functools.lru_cache(None)
def _pool():
    """the pool's keys as points, compressed bytes and rows"""
    pts = [ecc.E2_377.mul(ecc.G2_377, sk) for sk in tc.secret_keys()]
    return pts, [ecc.ser_point(ecc.E2_377, P) for P in pts], co.pack_g2_377(pts)[0]


def _blocks(gpu, b, entropies=True, keys_form=0, **change):
    f = dict(b.fields(entropies), **change)
    if keys_form == 0:
        return gpu.EpochBlocks(keys=b.key_bytes(_pool()[1]), key_off=b.key_off(), **f)
    rows = np.array([_pool()[2][j] for k in b.blocks for j in k.keys], dtype=np.uint64).reshape(-1, 24)
    return gpu.EpochBlocks(keys=rows, key_off=b.key_off(), keys_form=1, **f)


def _sign(gpu, b, blocks):
    """(nb, 48) signatures of the batch over the library's inner encodings, the replacements and deltas in place; and (encodings, extras)"""
    enc, extras, _, _ = gpu.epoch_encode_blocks(blocks, "inner")
    sig, att = gpu.sign_batch(co.ints_to_limbs(b.sign_keys(), 4), gpu.SIG_DOMAIN, enc, [b.sign_extra(i, extras[i].tobytes()) for i in range(b.nb)], 3)
    assert (att != 255).all()
    return b.signatures(sig), enc, extras


@functools.lru_cache(None)
def _world(gpu, chains, seed, n_keys=5, entropies=True):
    b = tc.Batch(list(chains), seed, n_keys=n_keys, tag="g")
    blocks = _blocks(gpu, b, entropies)
    sigs, enc, extras = _sign(gpu, b, blocks)
    return b, blocks, sigs, enc, extras


def _run(gpu, b, blocks, sigs, mode, **kw):
    return gpu.verify_epoch_transitions(blocks, b.chain_off, b.bits(), sigs, gpu.SIG_DOMAIN, NEG_G2, mode=mode, **kw)


def _check(b, r, mode, want=None, chain_ok=None):
    want = b.status[mode] if want is None else want
    bad = [(lab, int(g), w) for lab, g, w in zip(b.label, r["status"], want) if g != w]
    assert not bad, bad[:8]
    assert r["ok"].tolist() == [1 if w == 0 else 0 for w in want]
    if chain_ok is None:
        chain_ok = [int(not any(want[b.chain_off[c]:b.chain_off[c + 1]])) for c in range(len(b.chain_off) - 1)]
    assert r["chain_ok"].tolist() == chain_ok


BATCHES = tc.every_class_everywhere()
GROUPS = 8


@pytest.mark.parametrize("mode", [0, 1], ids=["each", "chain"])
@pytest.mark.parametrize("group", range(GROUPS))
def test_every_class_at_every_position_in_calls_of_65_transitions(gpu, group, mode):
    for n, chains in enumerate(BATCHES):
        if n % GROUPS != group:
            continue
        b, blocks, sigs, _, _ = _world(gpu, tuple(chains), 1000 + n)
        assert b.nb - len(chains) == 65
        r = _run(gpu, b, blocks, sigs, mode)
        _check(b, r, mode, chain_ok=b.chain_ok[mode])
        assert gpu.transitions_last()["path"] == b.path[mode], n


def _valid_world(gpu, n_tr, n_chains=1, n_keys=1):
    """n_tr valid transitions in n_chains equal chains of one key per block, built with numpy (no per-block Python objects)"""
    per = n_tr // n_chains
    assert per * n_chains == n_tr
    nb = n_tr + n_chains
    rng = np.random.default_rng(n_tr)
    pos = np.tile(np.arange(per + 1), n_chains)
    index = (1000 + pos + np.repeat(np.arange(n_chains), per + 1) * 7) % 60000
    ee = rng.integers(1, 256, size=(nb, 16), dtype=np.uint8)
    pe = np.roll(ee, 1, axis=0)
    which = rng.integers(0, tc.POOL, size=nb * n_keys)
    keys = np.frombuffer(b"".join(_pool()[1][j] for j in which), dtype=np.uint8).reshape(-1, 96)
    key_off = np.arange(nb + 1, dtype=np.uint32) * n_keys
    blocks = gpu.EpochBlocks(index, rng.integers(0, 256, size=nb), np.zeros(nb, dtype=np.uint32), np.full(nb, n_keys, dtype=np.uint32), ee, pe, keys, key_off)
    sks = tc.secret_keys()
    enc, extras, est, _ = gpu.epoch_encode_blocks(blocks, "inner")
    assert not est.any()
    sk = [0 if pos[i] == 0 else sum(sks[j] for j in which[(i - 1) * n_keys:i * n_keys]) % ecc.R377 for i in range(nb)]
    sig, att = gpu.sign_batch(co.ints_to_limbs(sk, 4), gpu.SIG_DOMAIN, enc, [e.tobytes() for e in extras], 3)
    chain_off = np.arange(n_chains + 1, dtype=np.uint32) * (per + 1)
    return blocks, chain_off, np.ones(nb * n_keys, dtype=np.uint8), sig, pos


@pytest.mark.parametrize("n_tr", [257, 8193])
def test_all_valid_transitions_take_the_chain_path(gpu, n_tr):
    blocks, chain_off, bits, sig, pos = _valid_world(gpu, n_tr)
    for mode, path in ((1, 1), (0, 0)):
        r = gpu.verify_epoch_transitions(blocks, chain_off, bits, sig, gpu.SIG_DOMAIN, NEG_G2, mode=mode, want=("status", "chain_ok"))
        assert not r["status"].any() and r["ok"].all() and r["chain_ok"].tolist() == [1]
        assert gpu.transitions_last()["path"] == path
    rec = gpu.transitions_last()["ms"]
    assert rec["wall"] > 0 and rec["decode"] > 0 and rec["hash"] > 0 and rec["sums"] > 0 and rec["products"] > 0


def test_many_chains_of_one_transition_against_one_chain_of_many(gpu):
    """the 64 transitions of one chain, and the same 64 as chains of their own (predecessor, block): the same verdicts, CRH rows and counters"""
    b, blocks, sigs, _, _ = _world(gpu, ((64, "wrong message", 9),), 5)
    one = _run(gpu, b, blocks, sigs, 0)
    _check(b, one, 0)
    pick = [i for t in range(1, 65) for i in (t - 1, t)]
    ko = b.key_off()
    keys = np.concatenate([b.key_bytes(_pool()[1])[ko[i]:ko[i + 1]] for i in pick])
    f = b.fields()
    many = gpu.EpochBlocks([f["index"][i] for i in pick], [f["round_"][i] for i in pick], [f["max_non_signers"][i] for i in pick], [f["max_validators"][i] for i in pick],
                           f["epoch_entropy"][pick], f["parent_entropy"][pick], keys, np.cumsum([0] + [ko[i + 1] - ko[i] for i in pick]).astype(np.uint32))
    bits = np.concatenate([b.bits()[ko[i]:ko[i + 1]] for i in pick])
    for mode in (0, 1):
        r = gpu.verify_epoch_transitions(many, 2 * np.arange(65, dtype=np.uint32), bits, sigs[pick], gpu.SIG_DOMAIN, NEG_G2, mode=mode)
        assert r["status"][1::2].tolist() == one["status"][1:].tolist() and not r["status"][0::2].any()
        assert r["chain_ok"].tolist() == [int(s == 0) for s in one["status"][1:]]
        assert np.array_equal(r["crh"][1::2], one["crh"][1:]) and np.array_equal(r["attempts"][1::2], one["attempts"][1:])
        assert not r["crh"][0::2].any() and not r["attempts"][0::2].any()
        assert gpu.transitions_last()["path"] == (2 if mode else 0)


def test_one_chain_of_one_transition_and_a_chain_of_an_initial_block_alone(gpu):
    b, blocks, sigs, _, _ = _world(gpu, ((1, "valid", 1),), 6)
    for mode in (0, 1):
        _check(b, _run(gpu, b, blocks, sigs, mode), mode)
        assert gpu.transitions_last()["path"] == mode
    # the initial block alone: nothing to check, accepted
    alone = gpu.EpochBlocks([5], [1], [0], [2], None, None, b.key_bytes(_pool()[1])[:2], [0, 2])
    r = gpu.verify_epoch_transitions(alone, [0, 1], np.ones(2, dtype=np.uint8), np.zeros((1, 48), dtype=np.uint8), gpu.SIG_DOMAIN, NEG_G2, mode=1)
    assert r["ok"].tolist() == [1] and r["chain_ok"].tolist() == [1] and r["asig_inf"].tolist() == [1] and not r["asig_xy"].any() and not r["crh"].any()


def test_the_cancelling_pair(gpu):
    """sig_a + D and sig_b - D: refused twice one by one; accepted by the chain product, as the circuit accepts them"""
    b, blocks, sigs, _, _ = _world(gpu, ((5, "cancelling pair", 2), (3, "valid", 1)), 8)
    r0 = _run(gpu, b, blocks, sigs, 0)
    assert r0["status"].tolist() == [0, 0, 10, 10, 0, 0, 0, 0, 0, 0] and r0["chain_ok"].tolist() == [0, 1] and gpu.transitions_last()["path"] == 0
    r1 = _run(gpu, b, blocks, sigs, 1)
    assert not r1["status"].any() and r1["chain_ok"].tolist() == [1, 1] and gpu.transitions_last()["path"] == 1
    # the sum of the signatures is the honest sum either way
    assert np.array_equal(r0["asig_xy"], r1["asig_xy"])


def test_keys_as_rows(gpu):
    """keys_form 1: the rows the decoder gives, with every class that has no undecodable key"""
    chains = tuple((3, cls, 2) for cls in tc.CLASSES if "bad key" not in cls and cls != "cancelling pair")
    b, blocks, sigs, _, _ = _world(gpu, chains, 9)
    rows = _blocks(gpu, b, keys_form=1)
    for mode in (0, 1):
        r0, r1 = _run(gpu, b, blocks, sigs, mode), _run(gpu, b, rows, sigs, mode)
        _check(b, r1, mode)
        for k in r0:
            assert np.array_equal(r0[k], r1[k]), k


def test_entropies_absent_zero_and_random(gpu):
    chains = ((3, "valid", 1), (3, "wrong parent entropy", 2), (3, "wrong parent entropy, initial zero", 2), (2, "wrong parent entropy", 1))
    b, blocks, sigs, _, _ = _world(gpu, chains, 10)
    for mode in (0, 1):
        _check(b, _run(gpu, b, blocks, sigs, mode), mode)
    # NULL arrays read as zeros: the rule is off in every chain, and the call equals the one with zero arrays
    bn, absent, sigs_n, _, _ = _world(gpu, chains, 10, 5, False)
    zeros = _blocks(gpu, bn, epoch_entropy=np.zeros((bn.nb, 16), dtype=np.uint8), parent_entropy=np.zeros((bn.nb, 16), dtype=np.uint8))
    only_ee = _blocks(gpu, bn, entropies=False, epoch_entropy=np.zeros((bn.nb, 16), dtype=np.uint8))
    for mode in (0, 1):
        r = _run(gpu, bn, absent, sigs_n, mode)
        assert not r["status"].any() and r["chain_ok"].all()
        for other in (zeros, only_ee):
            ro = _run(gpu, bn, other, sigs_n, mode)
            for k in r:
                assert np.array_equal(r[k], ro[k]), k


def test_max_validators_below_equal_above_and_at_the_table(gpu):
    b = tc.Batch([(4, "valid", 1)], 12, n_keys=5)
    maxv = [4, 5, 9, 206, 0]
    blocks = _blocks(gpu, b, max_validators=maxv)
    sigs, enc, _ = _sign(gpu, b, blocks)
    assert [len(e) for e in enc] == [gpu.epoch_encoded_size("inner", 5, v) for v in maxv]
    for mode in (0, 1):
        r = _run(gpu, b, blocks, sigs, mode)
        assert not r["status"].any()
        assert [r["crh"][i].tobytes() for i in range(1, 5)] == gpu.composite_crh(enc[1:])


def test_what_the_prover_takes_away(gpu):
    chains = ((4, "valid", 1), (3, "undecodable signature", 2), (3, "bad key in b", 2), (2, "signature outside G1", 1))
    b, blocks, sigs, enc, extras = _world(gpu, chains, 13)
    r = _run(gpu, b, blocks, sigs, 0)
    _check(b, r, 0)
    tr = [i for i in range(b.nb) if not b.initial[i]]
    crh = gpu.composite_crh([enc[i] for i in tr])
    _, att = gpu.hash_to_g1_composite(gpu.SIG_DOMAIN, [enc[i] for i in tr], [extras[i].tobytes() for i in tr], cip22=True)
    for n, i in enumerate(tr):
        assert r["crh"][i].tobytes() == crh[n] and r["attempts"][i] == att[n], b.label[i]
    for i in range(b.nb):
        if b.initial[i]:
            assert not r["crh"][i].any() and r["attempts"][i] == 0
    # the sum of the chain's signatures that decoded into G1, by the oracle
    for c in range(len(chains)):
        total = None
        for i in range(b.chain_off[c] + 1, b.chain_off[c + 1]):
            if b.blocks[i].raw is None:
                total = E1.add(total, ecc.deser_point(E1, sigs[i].tobytes()))
        wxy, winf = co.pack_g1_377([total])
        assert np.array_equal(r["asig_xy"][c], wxy[0]) and r["asig_inf"][c] == winf[0], c
    # every optional output NULL: the verdicts are the same
    for mode in (0, 1):
        bare = _run(gpu, b, blocks, sigs, mode, want=())
        assert bare["ok"].tolist() == r["ok"].tolist() and all(bare[k] is None for k in ("status", "chain_ok", "crh", "attempts", "asig_xy", "asig_inf"))


def test_one_byte_of_one_block_flips_exactly_what_hashes_or_chains_on_it(gpu):
    b, blocks, sigs, _, _ = _world(gpu, ((5, "valid", 1), (2, "valid", 1)), 14)
    f = b.fields()
    for label, change, want in (("round", dict(round_=[x ^ (1 if i == 2 else 0) for i, x in enumerate(f["round_"])]), {2: 10}),
                                ("epoch entropy", dict(epoch_entropy=_flip(f["epoch_entropy"], 2)), {2: 10, 3: 5}),
                                ("parent entropy", dict(parent_entropy=_flip(f["parent_entropy"], 4)), {4: 5}),
                                ("max_non_signers", dict(max_non_signers=[x ^ (1 if i == 3 else 0) for i, x in enumerate(f["max_non_signers"])]), {3: 10}),
                                ("the initial block's entropy", dict(epoch_entropy=_flip(f["epoch_entropy"], 0)), {1: 5}),
                                ("the last block's entropy", dict(epoch_entropy=_flip(f["epoch_entropy"], 5)), {5: 10})):
        changed = _blocks(gpu, b, **change)
        for mode in (0, 1):
            r = _run(gpu, b, changed, sigs, mode)
            assert r["status"].tolist() == [want.get(i, 0) for i in range(b.nb)], (label, mode)
            assert r["chain_ok"].tolist() == [0, 1]


def _flip(a, row):
    out = np.array(a, dtype=np.uint8).copy()
    out[row, 7] ^= 0x10
    return out


def test_mode_0_agrees_with_the_seals_entry_fed_through_the_host(gpu):
    """verify_aggregated_seals_bls12_377 with per-seal sets (the predecessor's rows), hash mode 3 and min_signers from the rule: what the parent
    commit computes for the transitions whose status the seals know - 0, 6, 8 and 10 as 0, 1, 2 and 4"""
    known = ("valid", "one signer short", "threshold met exactly", "undecodable signature", "signature outside G1", "wrong message", "bit flipped", "padding key unselected")
    chains = tuple((4, cls, 1 + k % 4) for k, cls in enumerate(known * 2)) + ((1, "valid", 1),)
    b, blocks, sigs, enc, extras = _world(gpu, chains, 16)
    assert b.nb - len(chains) == 65
    r = _run(gpu, b, blocks, sigs, 0)
    rows, kst = gpu.decompress("g2", b.key_bytes(_pool()[1]).tobytes())
    ko = b.key_off()
    seals = [i for i in range(b.nb) if not b.initial[i] and r["status"][i] in (0, 6, 8, 10) and not kst[ko[i - 1]:ko[i]].any()]
    assert len(seals) > 40 and {0, 6, 8, 10} <= {int(r["status"][i]) for i in seals}
    pk = np.concatenate([rows[ko[i - 1]:ko[i]] for i in seals])
    bits = np.concatenate([b.bits()[ko[i - 1]:ko[i]] for i in seals])
    off = np.cumsum([0] + [ko[i] - ko[i - 1] for i in seals]).astype(np.uint32)
    mins = np.array([max(0, len(b.blocks[i - 1].keys) - b.blocks[i - 1].mns) for i in seals], dtype=np.uint32)
    ok, st = gpu.verify_aggregated_seals(pk, None, off, bits, mins, gpu.SIG_DOMAIN, [enc[i] for i in seals], [extras[i].tobytes() for i in seals], sigs[seals], NEG_G2,
                                         hash_mode=3, mode=0)
    assert [{0: 0, 1: 6, 2: 8, 3: 9, 4: 10}[int(s)] for s in st] == [int(r["status"][i]) for i in seals]
    assert ok.tolist() == [int(r["ok"][i]) for i in seals]


def test_a_handful_against_seam_a(gpu):
    """the independent path, one transition at a time on handles: encode_epoch_block_to_bytes_cip22 + aggregate_public_keys +
    verify_signature(composite, cip22)"""
    from celo_bls_snark_rs_amd import ffi
    lib = C.CDLL(ffi.LIB_PATH)
    for name in ("deserialize_public_key", "deserialize_signature", "aggregate_public_keys", "verify_signature", "destroy_public_key", "destroy_signature",
                 "encode_epoch_block_to_bytes_cip22", "free_vec"):
        getattr(lib, name).restype = C.c_bool
    b, blocks, sigs, enc, extras = _world(gpu, ((2, "valid", 1), (2, "wrong message", 2), (2, "bit flipped", 1), (2, "threshold met exactly", 2), (2, "padding key unselected", 1)), 15)
    r = _run(gpu, b, blocks, sigs, 0)
    _check(b, r, 0)
    handles = []
    for e in _pool()[1]:
        h = C.c_void_p()
        assert lib.deserialize_public_key(e, C.c_int(96), C.byref(h))
        handles.append(h)
    seen = 0
    for i in range(b.nb):
        if b.initial[i]:
            continue
        k, p = b.blocks[i], b.blocks[i - 1]
        own = (C.c_void_p * len(k.keys))(*[handles[j].value for j in k.keys])
        ob, ol, xb, xl = C.POINTER(C.c_uint8)(), C.c_int(0), C.POINTER(C.c_uint8)(), C.c_int(0)
        assert lib.encode_epoch_block_to_bytes_cip22(C.c_ushort(k.index), C.c_ubyte(k.round), k.ee, k.pe, C.c_uint(k.mns), C.c_uint(k.maxv), own, C.c_int(len(k.keys)),
                                                     C.byref(ob), C.byref(ol), C.byref(xb), C.byref(xl))
        inner, extra = bytes(ob[:ol.value]), bytes(xb[:xl.value])
        assert inner == enc[i] and extra == extras[i].tobytes()
        chosen = [handles[j] for j, x in zip(p.keys, p.bits) if x]
        arr = (C.c_void_p * len(chosen))(*[h.value for h in chosen])
        apk, s, verdict = C.c_void_p(), C.c_void_p(), C.c_bool(False)
        assert lib.aggregate_public_keys(arr, C.c_int(len(chosen)), C.byref(apk))
        assert lib.deserialize_signature(sigs[i].tobytes(), C.c_int(48), C.byref(s))
        assert lib.verify_signature(apk, inner, C.c_int(len(inner)), extra, C.c_int(len(extra)), s, C.c_bool(True), C.c_bool(True), C.byref(verdict))
        assert bool(verdict.value) == bool(r["ok"][i]), b.label[i]
        assert lib.destroy_public_key(apk) and lib.destroy_signature(s) and lib.free_vec(ob, ol) and lib.free_vec(xb, xl)
        seen += 1
    assert seen == 10
    for h in handles:
        assert lib.destroy_public_key(h)


def test_two_threads(gpu):
    b, blocks, sigs, _, _ = _world(gpu, tuple(BATCHES[1]), 1001)
    got, errors = {}, []

    def run(mode):
        try:
            for _ in range(3):
                got[mode] = _run(gpu, b, blocks, sigs, mode)
        except Exception as e:      # noqa: BLE001
            errors.append(e)
    ts = [threading.Thread(target=run, args=(m,)) for m in (0, 1)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errors, errors
    for mode in (0, 1):
        _check(b, got[mode], mode, chain_ok=b.chain_ok[mode])
