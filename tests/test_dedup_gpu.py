"""GPU: decompress_bls12_377_g1/_g2_dedup(_dev) (csrc/unit_dedup.hip, csrc/dedup.h) against the plain decoders on whole outputs: every key
its representative's row and status, bit for bit.  Valid keys are made on the device (fixed_base_mul + compress); the encoding of infinity,
undecodable strings (x >= q, no root), a curve point outside the subgroup and a key with its flag bit flipped are mixed in.  The
representatives are checked against np.unique where tests/dedup_ref.py shows that no probe sequence can reach the cap in any insertion
order, and against the order-independent contract everywhere else.

NOT covered here: more than one device; more than 2^31 distinct keys (n itself is refused above 2^31 - 1); which keys hit the cap under a
race (it differs from run to run: only what is decoded from them is asserted)."""
import ctypes as C
import threading
import numpy as np
import pytest
import torch  # noqa: F401  (before the library: torch brings its own HIP runtime; loaded after the library's, it finds no device)
import dedup_ref as R
from oracle.py import ecc
from oracle import cpu_oracle as co

pytestmark = pytest.mark.gpu
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1025, 8193)
KB = {"g2": 96, "g1": 48}


class Keys:
    """8193 distinct valid keys of a group (the first 40 are "the pool"), the bad keys, and the plain decoder's verdict on the bad ones"""

    def __init__(self, gpu, g):
        self.g, kb = g, KB[g]
        name, gen, curve = (("bls12_377_g2", co.pack_g2_377([ecc.G2_377])[0][0], ecc.E2_377) if g == "g2" else ("bls12_377_g1", co.pack_g1_377([ecc.G1_377])[0][0], ecc.E1_377))
        rows, inf = gpu.fixed_base_mul(name, gen, co.ints_to_limbs([3 + 7 * k for k in range(max(SIZES))], 4))
        enc, st = gpu.encode_points(g, rows, inf)
        assert not inf.any() and not st.any() and len(np.unique(enc, axis=0)) == max(SIZES)
        self.valid, self.rows = enc, rows
        flipped = enc[0].copy()
        flipped[kb - 1] ^= 0x80                                      # the other root: a valid key, another row
        x_ge_q = np.zeros(kb, dtype=np.uint8)
        x_ge_q[:48] = 0xFF
        x_ge_q[47] = 0x3F                                            # 2^382 - 1 >= q in the first coordinate, no flag set
        small = [np.frombuffer(bytes([x]) + bytes(kb - 1), dtype=np.uint8) for x in range(1, 9)]      # x = 1 .. 8: no root, or outside the subgroup
        self.bad = np.stack([np.frombuffer(ecc.ser_point(curve, None), dtype=np.uint8), x_ge_q, flipped] + small)
        xy, st = gpu.decompress(g, self.bad.tobytes())
        self.bad_status = st
        assert st[0] == 1 and st[1] == 2 and st[2] == 0 and 2 in st[3:] and 3 in st[3:], st.tolist()
        assert np.array_equal(xy[2][:kb // 8], rows[0][:kb // 8]) and not np.array_equal(xy[2], rows[0])

    def pool(self, k=40):
        """k valid keys with the bad ones mixed in"""
        out = self.valid[:k].copy()
        for j, b in enumerate(self.bad):
            if 3 * j + 1 < k:
                out[3 * j + 1] = b
        return out


@pytest.fixture(scope="module")
def g2(gpu):
    return Keys(gpu, "g2")


@pytest.fixture(scope="module")
def g1(gpu):
    return Keys(gpu, "g1")


def both(gpu, g, keys, check=True):
    """the de-duplicating entry against the plain one on whole outputs; returns (rep, decoded)"""
    data = np.ascontiguousarray(keys).tobytes()
    want_xy, want_st = gpu.decompress(g, data, check)
    xy, st, rep, decoded = gpu.decompress_dedup(g, data, check)
    assert np.array_equal(st, want_st), np.nonzero(st != want_st)[0][:8]
    assert np.array_equal(xy, want_xy), np.nonzero((xy != want_xy).any(axis=1))[0][:8]
    R.contract(keys, rep, decoded)
    assert gpu.key_dedup_last()[:2] == (len(keys), decoded)
    return rep, decoded


def exact(keys, rep, decoded):
    assert R.exact(keys), R.longest_run(keys)                        # the restatement: below the cap in every insertion order
    want, distinct = R.first_occurrence(keys)
    assert np.array_equal(rep, want) and decoded == distinct


def bad_rows(k, n):
    """a pool of 3 cycled, with a bad key at rows 0, 63, 64 and n - 1 that also stands at another row"""
    keys = R.patterned(k.pool()[[0, 2, 3]], "pool of 3", n)
    for j, r in enumerate(r for r in (0, 63, 64, n - 1) if r < n):
        bad = k.bad[(j + n) % len(k.bad)]
        keys[r] = bad
        if n > 8:
            keys[(r + 5) % n] = bad
    return keys


@pytest.mark.parametrize("n", SIZES)
def test_whole_outputs_equal_the_plain_decoder_g2(gpu, g2, n):
    for pattern in R.PATTERNS:
        keys = R.patterned(g2.valid if pattern in ("all distinct", "twice in a row", "halves") else g2.pool(), pattern, n)
        exact(keys, *both(gpu, "g2", keys))
    keys = bad_rows(g2, n)
    exact(keys, *both(gpu, "g2", keys))
    mixed = g2.pool()[np.arange(n) % 40]                              # every bad kind among valid keys
    exact(mixed, *both(gpu, "g2", mixed))


@pytest.mark.parametrize("n", SIZES)
def test_whole_outputs_equal_the_plain_decoder_g1(gpu, g1, n):
    for pattern in R.PATTERNS:
        keys = R.patterned(g1.valid if pattern in ("all distinct", "twice in a row", "halves") else g1.pool(), pattern, n)
        exact(keys, *both(gpu, "g1", keys))
    keys = bad_rows(g1, n)
    exact(keys, *both(gpu, "g1", keys))


def test_without_the_subgroup_check(gpu, g2, g1):
    for k in (g2, g1):
        keys = k.pool()[np.arange(257) % 40]
        exact(keys, *both(gpu, k.g, keys, check=False))
        assert 3 not in gpu.decompress_dedup(k.g, keys.tobytes(), False)[1]


def test_a_full_table_one_probe_and_a_crowded_slot(gpu, g2):
    """settings under which keys hit the cap: the outputs are still those of the plain decoder, the contract holds, decoded lies in [distinct, n]"""
    try:
        gpu.key_dedup_set(-1, 0, 0)
        for n in (64, 256):
            keys = g2.valid[:n]
            rep, decoded = both(gpu, "g2", keys)                     # slack_log = 0, n a power of two, all distinct: the table is full
            assert R.slots(n, 0) == n and decoded == n
            both(gpu, "g2", R.patterned(g2.pool(), "halves", n))
        gpu.key_dedup_set(-1, -1, 1)
        for n in (65, 1025):
            for pattern in R.PATTERNS:
                both(gpu, "g2", R.patterned(g2.valid, pattern, n))
            both(gpu, "g2", bad_rows(g2, n))
        gpu.key_dedup_set(-1, -1, 0)
        crowd = R.same_home(300, R.slots(300), 96)
        assert not R.exact(crowd)
        rep, decoded = both(gpu, "g2", crowd)
        assert decoded == 300
        twice = np.concatenate([crowd, crowd[::-1]])                 # every key of the crowd again: home slots differ at this S, the bytes repeat
        both(gpu, "g2", twice)
        crowd600 = R.same_home(300, R.slots(600), 96)
        both(gpu, "g2", np.concatenate([crowd600, crowd600]))         # 300 keys on one home slot of THIS table, each twice: capped keys may repeat
    finally:
        gpu.key_dedup_set(-1, -1, 0)


def test_dev_form_on_a_stream_with_an_unaligned_input(gpu, g2, g1):
    for k in (g2, g1):
        kb, words = KB[k.g], KB[k.g] // 4
        n = 1025
        keys = bad_rows(k, n)
        want_xy, want_st, want_rep, want_dec = gpu.decompress_dedup(k.g, keys.tobytes())
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            buf = torch.zeros(n * kb + 1, dtype=torch.uint8, device="cuda")
            buf[1:] = torch.from_numpy(keys.reshape(-1).copy()).cuda()
            d_xy = torch.full((n * words + 2,), 0x5A5A, dtype=torch.int64, device="cuda")
            d_st = torch.full((n + 1,), 9, dtype=torch.uint8, device="cuda")
            d_rep = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda")
        stream.synchronize()
        for off in (0, 1):                                            # rows at a multiple of 16, and at 8 more
            dec = gpu.decompress_dedup_dev(k.g, buf.data_ptr() + 1, n, d_xy.data_ptr() + 8 * off, d_st.data_ptr(), d_rep.data_ptr(), stream=stream.cuda_stream)
            got = d_xy.cpu().numpy().view(np.uint64)
            assert np.array_equal(got[off:off + n * words].reshape(n, words), want_xy) and got[off + n * words] == 0x5A5A
            assert np.array_equal(d_st.cpu().numpy()[:n], want_st) and d_st[n].item() == 9
            assert np.array_equal(d_rep.cpu().numpy()[:n].view(np.uint32), want_rep) and d_rep[n].item() == -1 and dec == want_dec
        d_st.fill_(9)
        dec = gpu.decompress_dedup_dev(k.g, buf.data_ptr() + 1, n, d_xy.data_ptr(), d_st.data_ptr(), 0, stream=stream.cuda_stream)      # no out_rep
        assert dec == want_dec and np.array_equal(d_st.cpu().numpy()[:n], want_st)
        fn = getattr(gpu.lib(), "decompress_bls12_377_%s_dedup_dev" % k.g)
        rc = fn(C.c_void_p(buf.data_ptr() + 1), C.c_size_t(n), C.c_int(1), C.c_void_p(d_xy.data_ptr()), C.c_void_p(d_st.data_ptr()), None, None, C.c_void_p(stream.cuda_stream))
        assert rc == 0                                                # neither out_rep nor out_decoded


def test_without_rep_and_decoded(gpu, g2):
    keys = R.patterned(g2.pool(), "pool of 3", 257)
    want_xy, want_st = gpu.decompress("g2", keys.tobytes())
    xy, st, rep, _ = gpu.decompress_dedup("g2", keys.tobytes(), want_rep=False)
    assert rep is None and np.array_equal(xy, want_xy) and np.array_equal(st, want_st)
    xy2 = np.zeros_like(xy)
    st2 = np.zeros_like(st)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert gpu.lib().decompress_bls12_377_g2_dedup(p(keys), C.c_size_t(257), C.c_int(1), p(xy2), p(st2), None, None) == 0
    assert np.array_equal(xy2, want_xy) and np.array_equal(st2, want_st)


def test_one_changed_byte_changes_one_row_and_decodes_one_key_more(gpu, g2):
    keys = R.patterned(g2.valid[:3], "pool of 3", 257)
    xy, st, rep, decoded = gpu.decompress_dedup("g2", keys.tobytes())
    assert decoded == 3
    for row, byte in ((100, 0), (256, 95), (4, 47), (64, 48)):          # (no first occurrence: the other rows keep their representatives)
        k2 = keys.copy()
        k2[row, byte] ^= 0x40 if byte == 95 else 0x01
        rep2, decoded2 = both(gpu, "g2", k2)
        xy2, st2, _, _ = gpu.decompress_dedup("g2", k2.tobytes())
        others = np.arange(257) != row
        assert decoded2 == 4 and rep2[row] == row and np.array_equal(rep2[others], rep[others])
        assert np.array_equal(xy2[others], xy[others]) and np.array_equal(st2[others], st[others])
        assert not (np.array_equal(xy2[row], xy[row]) and st2[row] == st[row])


def test_two_threads(gpu, g2, g1):
    jobs = {0: ("g2", bad_rows(g2, 1025)), 1: ("g1", R.patterned(g1.pool(), "halves", 8193))}
    want = {t: gpu.decompress(g, keys.tobytes()) for t, (g, keys) in jobs.items()}
    out, errs = {}, []

    def work(t):
        try:
            gpu.use_device(0)
            g, keys = jobs[t]
            for _ in range(3):
                out[t] = gpu.decompress_dedup(g, keys.tobytes())
        except Exception as e:      # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=work, args=(t,)) for t in jobs]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for t, (g, keys) in jobs.items():
        assert np.array_equal(out[t][0], want[t][0]) and np.array_equal(out[t][1], want[t][1])
        exact(keys, out[t][2], out[t][3])


def test_the_record_reports_keys_and_decoded_and_a_refused_call_leaves_it(gpu, g2):
    keys = R.patterned(g2.pool(), "pool of 3", 1025)
    gpu.decompress_dedup("g2", keys.tobytes())
    n, U, ms = gpu.key_dedup_last()
    assert (n, U) == (1025, 3) and all(v > 0 for v in ms)
    xy = np.zeros((2, 24), dtype=np.uint64)
    st = np.zeros(2, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert gpu.lib().decompress_bls12_377_g2_dedup(None, C.c_size_t(2), C.c_int(1), p(xy), p(st), None, None) == 2
    assert gpu.lib().decompress_bls12_377_g2_dedup(p(keys), C.c_size_t(1 << 31), C.c_int(1), p(xy), p(st), None, None) == 2
    assert gpu.lib().decompress_bls12_377_g2_dedup(None, C.c_size_t(0), C.c_int(1), None, None, None, None) == 0
    assert gpu.key_dedup_last() == (n, U, ms)
    gpu.decompress("g2", keys.tobytes())                              # the plain decoder has a record of its own
    assert gpu.key_dedup_last() == (n, U, ms)
