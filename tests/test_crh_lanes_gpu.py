"""GPU: the many-lane CRH kernel (csrc/unit_hash_lanes.hip: k_pedersen_crh_lanes behind pedersen_crh_locked of csrc/unit_hash.hip) at every width celo_amd_crh_set_lanes
accepts, whole outputs against oracle/py/composite.py (computed once per session on the pool of tests/hash_ref.py) and against the one-lane
kernel of the same run, through every entry that reaches it.  Every test that moves the width puts the rule back.
NOT covered: the 31-bit grid clamp on the device (tests/test_crh_lanes_host.py holds the rule to it), more than one device, and the
per-attempt CRH of the composite mode without CIP22 (one lane per attempt, unchanged code)."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch  # before the library: both must share one HIP runtime
import hash_ref as hr
from tests import helpers as H

pytestmark = pytest.mark.gpu
WIDTHS = (1, 2, 4, 8, 16, 32, 64, 128, 256)


def _chunks(nbytes):
    return (nbytes * 8 + 2) // 3


class Refs:
    def __init__(self):
        rng = np.random.default_rng(0xC4A1)
        # every length 0 ... 200: chunk counts from 0 to 534 in steps of 2 or 3, on both sides of L and 2 L for every L up to 256
        self.short = [hr.rand_bytes(rng, l) for l in range(201)]
        # empty, short, an epoch-sized one, the longest the table covers (all 52 080 chunks), empty
        self.long = [b"", hr.rand_bytes(rng, 12), hr.rand_bytes(rng, 14200), hr.rand_bytes(rng, hr.PEDERSEN_MAX_BYTES), b""]
        self.many = [hr.rand_bytes(rng, 40) for _ in range(257)]
        self.long_ref = hr.CrhBatch(self.long, per=1)          # the two long ones first: they are the longest tasks
        self.short_ref = hr.CrhBatch(self.short)
        self.many_ref = hr.CrhBatch(self.many)


@pytest.fixture(scope="session")
def refs():
    return Refs()


@pytest.fixture()
def lanes(gpu):
    """the setter; the rule is back when the test ends, however it ends"""
    try:
        yield gpu.crh_set_lanes
    finally:
        gpu.crh_set_lanes(0)


def test_short_messages_of_every_length_at_every_width(gpu, refs, lanes):
    want = refs.short_ref.hashes()
    for L in WIDTHS:
        lanes(L)
        for bad in (-1, 3, 257, 512):                     # a refused value changes nothing
            assert gpu.lib().celo_amd_crh_set_lanes(C.c_int(bad)) == 2
        assert gpu.composite_crh(refs.short) == want, L
        assert gpu.crh_last_lanes() == L


def test_long_messages_at_every_width(gpu, refs, lanes):
    want = refs.long_ref.hashes()
    assert want[0] == want[4] == hr.comp.composite_crh(b"")
    for L in WIDTHS:
        lanes(L)
        assert gpu.composite_crh(refs.long) == want, L
        assert gpu.crh_last_lanes() == L


@pytest.mark.parametrize("n", [1, 2, 127, 128, 129, 257])
def test_message_counts_across_the_workgroup_border_of_every_width(gpu, refs, lanes, n):
    """256 / L messages per workgroup: 1, 2, 127, 128, 129 and 257 messages leave dead lanes in the last workgroup of every width, which
    must reach the fold's barriers"""
    want = refs.many_ref.hashes()[:n]
    lanes(1)
    one = gpu.composite_crh(refs.many[:n])
    assert one == want
    for L in WIDTHS[1:]:
        lanes(L)
        assert gpu.composite_crh(refs.many[:n]) == one, L
        assert gpu.crh_last_lanes() == L


def test_rows_are_independent(gpu, lanes):
    rng = np.random.default_rng(9)
    msgs = [hr.rand_bytes(rng, 2000) for _ in range(9)]
    changed = list(msgs)
    changed[5] = msgs[5][:1234] + bytes([msgs[5][1234] ^ 0x20]) + msgs[5][1235:]
    lanes(1)
    one, one_changed = gpu.composite_crh(msgs), gpu.composite_crh(changed)
    lanes(64)
    base, got = gpu.composite_crh(msgs), gpu.composite_crh(changed)
    assert base == one and got == one_changed
    assert [i for i in range(9) if got[i] != base[i]] == [5]


def test_the_rule_picks_one_lane_for_many_short_messages_and_many_for_one_long(gpu, refs, lanes):
    ht = C.CDLL(H.build_hosttest())
    ht.ht_crh_pick_lanes.restype = C.c_uint32
    ht.ht_crh_pick_lanes.argtypes = [C.c_uint32, C.c_size_t, C.c_size_t]
    rng = np.random.default_rng(10)
    short = [hr.rand_bytes(rng, 12) for _ in range(257)]
    lanes(0)
    by_rule = gpu.composite_crh(short)
    assert gpu.crh_last_lanes() == 1 == ht.ht_crh_pick_lanes(0, _chunks(12), 257)
    lanes(16)
    assert gpu.composite_crh(short) == by_rule and gpu.crh_last_lanes() == 16
    lanes(0)
    long_rule = gpu.composite_crh(refs.long[2:3])
    L = gpu.crh_last_lanes()
    assert L > 1 and L == ht.ht_crh_pick_lanes(0, _chunks(14200), 1)
    lanes(1)
    assert gpu.composite_crh(refs.long[2:3]) == long_rule == refs.long_ref.hashes()[2:3] and gpu.crh_last_lanes() == 1


def _pack(msgs):
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
    return np.frombuffer(b"".join(msgs) + bytes(8), dtype=np.uint8).copy(), off


def test_the_device_form_on_a_callers_stream(gpu, refs, lanes):
    msgs = refs.short[150:] + refs.many[:30] + [refs.long[2]]
    want = refs.short_ref.hashes()[150:] + refs.many_ref.hashes()[:30] + [refs.long_ref.hashes()[2]]
    mdat, moff = _pack(msgs)
    n = len(msgs)
    for L in (1, 64):
        lanes(L)
        stream = torch.cuda.Stream()
        d_m = torch.from_numpy(mdat).cuda()
        d_out = torch.full((n * 48 + 8,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert gpu.composite_crh_dev(d_m.data_ptr(), moff, n, d_out.data_ptr(), stream=stream.cuda_stream) == 0
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        assert [out[48 * i:48 * i + 48].tobytes() for i in range(n)] == want, L
        assert (out[48 * n:] == 0xA5).all() and gpu.crh_last_lanes() == L


def test_cip22_composite_hash_to_g1(gpu, lanes):
    rng = np.random.default_rng(11)
    msgs = [hr.rand_bytes(rng, l) for l in (0, 1, 200, 2000)]
    extras = [hr.rand_bytes(rng, e) for e in (0, 1, 7, 2)]
    lanes(1)
    xy, att = gpu.hash_to_g1_composite(gpu.SIG_DOMAIN, msgs, extras, cip22=True)
    P, c = hr.reference("composite_cip22", gpu.SIG_DOMAIN, msgs[2], extras[2])
    assert np.array_equal(xy[2], hr.co.pack_g1_377([P])[0][0]) and att[2] == c
    for L in (16, 256):
        lanes(L)
        xy_l, att_l = gpu.hash_to_g1_composite(gpu.SIG_DOMAIN, msgs, extras, cip22=True)
        assert np.array_equal(xy_l, xy) and np.array_equal(att_l, att), L
        assert gpu.crh_last_lanes() == L


def test_a_chain_of_three_transitions_over_four_keys(gpu, lanes):
    import transition_cases as tc
    from test_transitions_gpu import _blocks, _sign, _run, _check
    b = tc.Batch([(3, "valid", 1)], 77, n_keys=4, tag="g")
    blocks = _blocks(gpu, b)
    sigs, enc, _ = _sign(gpu, b, blocks)
    got = {}
    for L in (1, 16):
        lanes(L)
        for mode in (0, 1):
            got[L, mode] = _run(gpu, b, blocks, sigs, mode)
            _check(b, got[L, mode], mode)
            assert gpu.crh_last_lanes() == L
    for mode in (0, 1):
        for k in got[1, mode]:
            assert np.array_equal(got[1, mode][k], got[16, mode][k]), (mode, k)
    lanes(0)
    assert [got[16, 0]["crh"][i].tobytes() for i in range(1, 4)] == gpu.composite_crh(enc[1:])


def test_two_threads_at_width_8(gpu, refs, lanes):
    lanes(8)
    jobs = {0: (refs.short, refs.short_ref.hashes()), 1: (refs.many, refs.many_ref.hashes())}
    got, errors = {}, []

    def run(k):
        try:
            for _ in range(3):
                got[k] = gpu.composite_crh(jobs[k][0])
        except Exception as e:      # noqa: BLE001
            errors.append(e)
    ts = [threading.Thread(target=run, args=(k,)) for k in jobs]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errors, errors
    for k in jobs:
        assert got[k] == jobs[k][1]
    assert gpu.crh_last_lanes() == 8
