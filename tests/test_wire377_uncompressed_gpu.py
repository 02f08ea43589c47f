"""GPU: bulk decoding of uncompressed BLS12-377 points (decode_uncompressed_bls12_377_*; csrc/unit_wire.hip k_decode377u) against the status
rules restated in tests/bls377_serial.py, whole outputs (rows and statuses), bit for bit.

The shared case list (tests/bls377_serial.uncompressed_cases: generators, the reference's hash-to-curve points, the identity, both flags, the
range failures, an off-curve pair, points outside the subgroup, a set 0x80 bit) is laid out cyclically; at n = 1 and n = 65 from every start,
so every case is met alone in lane 0, in the lanes on both sides of the 64-lane block border and alone in a ragged last block; n = 63, 64 and
257 (a short block, a full one, several with a ragged tail) from two starts.  The expectation is computed once per (group, check) and shared."""
import ctypes as C
import threading
import numpy as np
import pytest
import torch  # before the library: both must share one HIP runtime
import bls377_serial as bs

pytestmark = pytest.mark.gpu
SIZES = [1, 63, 64, 65, 257]
GROUPS = ["g1", "g2"]


def batch(g2, n, start):
    """n encodings: case (start + i) mod len at position i -> (bytes, the cases' indices)"""
    cases = bs.uncompressed_cases(g2)
    idx = [(start + i) % len(cases) for i in range(n)]
    return b"".join(cases[j][1] for j in idx), np.array(idx)


def expected(g2, idx, check):
    st, rows = bs.uncompressed_expected(g2, check)
    return st[idx], rows[idx]


@pytest.mark.parametrize("check", [True, False], ids=["checked", "unchecked"])
@pytest.mark.parametrize("group", GROUPS)
def test_whole_outputs_match_the_rules_at_every_size(gpu, group, check):
    g2 = int(group == "g2")
    ncases = len(bs.uncompressed_cases(g2))
    seen = set()
    for n in SIZES:
        for start in (range(ncases) if n in (1, 65) else (0, 7)):               # n = 1 and 65: every rotation of the list
            data, idx = batch(g2, n, start)
            xy, st = gpu.decode_uncompressed(group, data, check=check)
            want_st, want_xy = expected(g2, idx, check)
            assert np.array_equal(st, want_st), (n, start, np.nonzero(st != want_st)[0][:4])
            assert np.array_equal(xy, want_xy), (n, start)
            seen |= {(int(j), n, i) for i, j in enumerate(idx) if i in (0, 62, 63, 64)}
    # every case was met alone in lane 0, in the last two lanes of a block that has a successor, and alone in the ragged second block
    for j in range(ncases):
        assert {(j, 1, 0), (j, 65, 62), (j, 65, 63), (j, 65, 64)} <= seen, j
    assert gpu.decompress_last_ms() > 0


@pytest.mark.parametrize("group", GROUPS)
def test_dev_form_equals_host_form(gpu, group):
    g2, words, size = int(group == "g2"), 24 if group == "g2" else 12, 192 if group == "g2" else 96
    n = 257
    data, idx = batch(g2, n, 3)
    for check in (True, False):
        xy, st = gpu.decode_uncompressed(group, data, check=check)
        d_in = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
        d_out = torch.full((n * words,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
        d_st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        assert gpu.decode_uncompressed_dev(group, d_in.data_ptr(), n, d_out.data_ptr(), d_st.data_ptr(), check=check, stream=stream.cuda_stream) == 0
        torch.cuda.synchronize()
        assert np.array_equal(d_st.cpu().numpy(), st) and np.array_equal(d_out.cpu().numpy().view(np.uint64).reshape(n, words), xy)
        assert d_in.numel() == n * size


@pytest.mark.parametrize("group", GROUPS)
def test_encode_then_decode_and_agreement_with_decompress(gpu, group):
    """encode_uncompressed_* then the new decode gives back the rows; the new decode and decompress_* agree on the same points, statuses
    included (subgroup points, points outside it, the identity)"""
    g2 = int(group == "g2")
    curve = bs.E2 if g2 else bs.E1
    cases = bs.uncompressed_cases(g2)
    keep = [i for i, (name, _, want) in enumerate(cases) if want in ((0, 0), (3, 0), (1, 1)) and name not in ("0x80 set", "identity over junk")]
    idx = np.array([keep[i % len(keep)] for i in range(65)])
    st_u, rows = expected(g2, idx, False)                                       # the points as rows (zero rows: the identity)
    enc_u, est = gpu.encode_points(group, rows, compressed=False)
    assert np.array_equal(est, st_u) and enc_u.tobytes() == b"".join(cases[j][1] for j in idx)
    back, bst = gpu.decode_uncompressed(group, enc_u.tobytes(), check=False)
    assert np.array_equal(bst, st_u) and np.array_equal(back, rows)
    enc_c, _ = gpu.encode_points(group, rows, compressed=True)
    assert enc_c.tobytes() == b"".join(bs.ser(curve, P, 0) for P in bs.rows_to_points(curve, rows))
    for check in (True, False):
        a_xy, a_st = gpu.decode_uncompressed(group, enc_u.tobytes(), check=check)
        b_xy, b_st = gpu.decompress(group, enc_c.tobytes(), check_subgroup=check)
        assert np.array_equal(a_st, b_st) and np.array_equal(a_xy, b_xy), check
        assert np.array_equal(a_st, expected(g2, idx, check)[0])
    assert set(a_st.tolist()) == {0, 1} and set(gpu.decode_uncompressed(group, enc_u.tobytes(), check=True)[1].tolist()) == {0, 1, 3}


@pytest.mark.parametrize("group", GROUPS)
def test_refused_arguments_write_nothing(gpu, group):
    g2, words = int(group == "g2"), 24 if group == "g2" else 12
    n = 3
    data, _ = batch(g2, n, 0)
    buf = np.frombuffer(data, dtype=np.uint8)
    xy = np.full((n, words), 0x5A, dtype=np.uint64)
    st = np.full(n, 0xEE, dtype=np.uint8)
    fn = getattr(gpu.lib(), "decode_uncompressed_bls12_377_" + group)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for args in ((None, p(xy), p(st)), (p(buf), None, p(st)), (p(buf), p(xy), None)):
        assert fn(args[0], C.c_size_t(n), C.c_int(1), args[1], args[2]) == 2
    assert fn(p(buf), C.c_size_t(1 << 31), C.c_int(1), p(xy), p(st)) == 2
    assert (xy == 0x5A).all() and (st == 0xEE).all()
    assert fn(None, C.c_size_t(0), C.c_int(1), None, None) == 0                 # n == 0 touches nothing
    d_in = torch.from_numpy(buf.copy()).cuda()
    d_out = torch.full((n * words + 1,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    d_st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for d_i, d_o, d_s in ((0, d_out.data_ptr(), d_st.data_ptr()), (d_in.data_ptr(), 0, d_st.data_ptr()), (d_in.data_ptr(), d_out.data_ptr(), 0),
                          (d_in.data_ptr(), d_out.data_ptr() + 4, d_st.data_ptr())):          # the last: rows not 8-byte aligned
        assert gpu.decode_uncompressed_dev(group, d_i, n, d_o, d_s) == 2
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0x5A5A5A5A).all() and (d_st.cpu().numpy() == 0xEE).all()
    assert gpu.decode_uncompressed_dev(group, d_in.data_ptr(), n, d_out.data_ptr(), d_st.data_ptr()) == 0      # ... and the next call is a normal one
    torch.cuda.synchronize()
    want_st, want_xy = expected(g2, np.arange(n), True)
    assert np.array_equal(d_st.cpu().numpy(), want_st) and np.array_equal(d_out.cpu().numpy()[:n * words].view(np.uint64).reshape(n, words), want_xy)


def test_two_host_threads(gpu):
    jobs = [("g1", 65, 2, True), ("g2", 65, 5, True)]
    got, errs = [None, None], []

    def work(i):
        try:
            group, n, start, check = jobs[i]
            data, _ = batch(int(group == "g2"), n, start)
            for _ in range(3):
                got[i] = gpu.decode_uncompressed(group, data, check=check)
        except Exception as e:                                                  # reported below: an exception in a thread is not a test failure by itself
            errs.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for (group, n, start, check), (xy, st) in zip(jobs, got):
        g2 = int(group == "g2")
        want_st, want_xy = expected(g2, batch(g2, n, start)[1], check)
        assert np.array_equal(st, want_st) and np.array_equal(xy, want_xy)
