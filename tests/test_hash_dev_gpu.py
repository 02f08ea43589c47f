"""GPU: the device-resident hash entries (include/celo_bls_amd.h: composite_crh_bls12_377_dev, hash_to_g1_{direct,cip22_tail,composite}_bls12_377_dev;
csrc/unit_hash.hip) against their host-pointer twins on whole outputs - rows, attempts, CRH bytes, the number of rounds - and against
tests/hash_ref.py on a subset.  Sizes 1, 63, 64, 65, 257 and 8193 (the first at which the first round is 8 counters wide, not 16), lengths 0, 1,
32 and 200, with and without extra data, all four modes.
NOT coverable: a cofactor multiple that is the identity (the host's serial fallback of the device form) and counter exhaustion - no input that
reaches either is known."""
import ctypes as C
import threading
import numpy as np
import pytest
import torch  # before the library: both must share one HIP runtime
import hash_ref as hr

pytestmark = pytest.mark.gpu
DOMAIN = b"ULforxof"
LENGTHS = (0, 1, 32, 200)
EXTRA_LENGTHS = (0, 7, 2, 33)
MODE_NAME = {0: "direct", 1: "tail", 2: "composite", 3: "composite_cip22"}


def _messages(n, seed):
    rng = np.random.default_rng(seed)
    msgs = [hr.rand_bytes(rng, LENGTHS[(i + seed) % 4]) for i in range(n)]
    extras = [hr.rand_bytes(rng, EXTRA_LENGTHS[(i // 4 + seed) % 4]) for i in range(n)]
    return msgs, extras


def _pack(items):
    off = np.zeros(len(items) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(b) for b in items], dtype=np.uint64)
    return np.frombuffer(b"".join(items) + b"\0", dtype=np.uint8), off


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _hash_dev(gpu, msgs, extras, mode, stream=0):
    """-> (code, xy (n, 12) uint64, attempts (n,) uint8) through the device entry; the outputs start as 0xA5 bytes"""
    n = len(msgs)
    mdat, moff = _pack(msgs)
    d_m = _dev(mdat)
    d_e, eoff = None, None
    if extras is not None:
        edat, eoff = _pack(extras)
        d_e = _dev(edat)
    d_xy = torch.full((n * 96 + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    d_att = torch.full((n + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = gpu.hash_to_g1_dev(DOMAIN, d_m.data_ptr(), moff, d_e.data_ptr() if d_e is not None else 0, eoff, n, d_xy.data_ptr(), d_att.data_ptr(), mode=mode, stream=stream)
    xy, att = d_xy.cpu().numpy(), d_att.cpu().numpy()
    assert (xy[n * 96:] == 0xA5).all() and (att[n:] == 0xA5).all()          # nothing past the rows
    return rc, xy[:n * 96].copy().view(np.uint64).reshape(n, 12), att[:n].copy()


def _hash_host(gpu, msgs, extras, mode):
    if mode >= 2:
        return gpu.hash_to_g1_composite(DOMAIN, msgs, extras, cip22=mode == 3)
    return gpu.hash_to_g1_direct(DOMAIN, msgs, extras, cip22_tail=mode == 1)


@pytest.mark.parametrize("mode", [0, 1, 2, 3], ids=[MODE_NAME[m] for m in range(4)])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 8193])
def test_device_form_equals_host_form(gpu, n, mode):
    msgs, extras = _messages(n, 10 * n + mode)
    for ex in (extras, None):
        want_xy, want_att = _hash_host(gpu, msgs, ex, mode)
        want_rounds = gpu.hash_last_rounds()
        rc, xy, att = _hash_dev(gpu, msgs, ex, mode)
        assert rc == 0
        assert np.array_equal(att, want_att) and np.array_equal(xy, want_xy)
        assert (att != 255).all()
        assert gpu.hash_last_rounds() == want_rounds == len(hr.round_widths(att))
        assert hr.round_widths(att)[0][0] == (8 if n == 8193 else 16)


@pytest.mark.parametrize("mode", [0, 1, 2, 3], ids=[MODE_NAME[m] for m in range(4)])
def test_device_form_against_the_reference(gpu, mode):
    msgs, extras = _messages(65, 77 + mode)
    sub = list(range(0, 65, 5))
    want = hr.Batch(MODE_NAME[mode], DOMAIN, [msgs[i] for i in sub], [extras[i] for i in sub])
    rc, xy, att = _hash_dev(gpu, msgs, extras, mode)
    assert rc == 0
    wxy, watt = want.rows()
    assert np.array_equal(xy[sub], wxy) and np.array_equal(att[sub], watt)


def _crh_dev(gpu, msgs):
    n = len(msgs)
    mdat, moff = _pack(msgs)
    d_m = _dev(mdat)
    d_out = torch.full((n * 48 + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = gpu.composite_crh_dev(d_m.data_ptr(), moff, n, d_out.data_ptr())
    return rc, d_out


@pytest.mark.parametrize("n", [1, 65, 257, 8193])
def test_crh_device_form_and_its_output_fed_to_the_device_tail_is_mode_3(gpu, n):
    msgs, extras = _messages(n, 3 * n)
    want = gpu.composite_crh(msgs)
    rc, d_out = _crh_dev(gpu, msgs)
    out = d_out.cpu().numpy()
    assert rc == 0 and (out[n * 48:] == 0xA5).all()
    assert [out[48 * i:48 * i + 48].tobytes() for i in range(n)] == want
    if n <= 65:
        ref = hr.CrhBatch(msgs[:8]).hashes()
        assert want[:8] == ref
    # the rows, where the CRH kernel left them, as the inner hashes of the tail
    edat, eoff = _pack(extras)
    d_e = _dev(edat)
    d_xy = torch.zeros(n * 96, dtype=torch.uint8, device="cuda")
    d_att = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert gpu.hash_to_g1_dev(DOMAIN, d_out.data_ptr(), 48 * np.arange(n + 1, dtype=np.uint64), d_e.data_ptr(), eoff, n, d_xy.data_ptr(), d_att.data_ptr(), mode=1) == 0
    wxy, watt = gpu.hash_to_g1_composite(DOMAIN, msgs, extras, cip22=True)
    assert np.array_equal(d_xy.cpu().numpy().view(np.uint64).reshape(n, 12), wxy) and np.array_equal(d_att.cpu().numpy(), watt)


def test_on_a_stream_of_the_callers(gpu):
    """the work is ordered behind what the caller enqueued on the stream: the messages are written there by a copy on that stream"""
    msgs, extras = _messages(257, 5)
    mdat, moff = _pack(msgs)
    edat, eoff = _pack(extras)
    s = torch.cuda.Stream()
    src_m, src_e = _dev(mdat), _dev(edat)
    d_m, d_e = torch.zeros_like(src_m), torch.zeros_like(src_e)
    d_xy = torch.zeros(257 * 96, dtype=torch.uint8, device="cuda")
    d_att = torch.zeros(257, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        d_m.copy_(src_m, non_blocking=True)
        d_e.copy_(src_e, non_blocking=True)
        assert gpu.hash_to_g1_dev(DOMAIN, d_m.data_ptr(), moff, d_e.data_ptr(), eoff, 257, d_xy.data_ptr(), d_att.data_ptr(), mode=3, stream=s.cuda_stream) == 0
    wxy, watt = gpu.hash_to_g1_composite(DOMAIN, msgs, extras, cip22=True)
    assert np.array_equal(d_xy.cpu().numpy().view(np.uint64).reshape(257, 12), wxy) and np.array_equal(d_att.cpu().numpy(), watt)


def test_refused_arguments_return_2_and_write_nothing(gpu):
    msgs, extras = _messages(9, 1)
    mdat, moff = _pack(msgs)
    edat, eoff = _pack(extras)
    d_m, d_e = _dev(mdat), _dev(edat)
    long_off = np.array([0, hr.PEDERSEN_MAX_BYTES + 1], dtype=np.uint64)
    d_long = torch.zeros(hr.PEDERSEN_MAX_BYTES + 8, dtype=torch.uint8, device="cuda")
    dec = moff.copy()
    dec[2], dec[3] = moff[3], moff[2]                  # (message 2 is 200 bytes long)
    assert dec[3] < dec[2]
    for mode in range(4):
        base = dict(dom=DOMAIN, m=d_m.data_ptr(), moff=moff, e=d_e.data_ptr(), eoff=eoff, n=9, xy=True, att=True)
        cases = [("domain NULL", dict(dom=None)), ("msg_off NULL", dict(moff=None)), ("out_xy NULL", dict(xy=False)), ("attempts NULL", dict(att=False)),
                 ("msgs NULL", dict(m=0)), ("extras NULL", dict(e=0)), ("decreasing offsets", dict(moff=dec)), ("decreasing extra offsets", dict(eoff=dec))]
        if mode >= 2:
            cases.append(("past the generator table", dict(m=d_long.data_ptr(), moff=long_off, e=0, eoff=None, n=1)))
        for label, ch in cases:
            a = dict(base, **ch)
            d_xy = torch.full((9 * 96,), 0xA5, dtype=torch.uint8, device="cuda")
            d_att = torch.full((9,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            rc = gpu.hash_to_g1_dev(a["dom"], a["m"], a["moff"], a["e"], a["eoff"], a["n"], d_xy.data_ptr() if a["xy"] else 0, d_att.data_ptr() if a["att"] else 0, mode=mode)
            assert rc == 2, (label, mode)
            assert (d_xy.cpu().numpy() == 0xA5).all() and (d_att.cpu().numpy() == 0xA5).all(), (label, mode)
    d_out = torch.full((9 * 48,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for label, rc in (("msg_off NULL", gpu.composite_crh_dev(d_m.data_ptr(), None, 9, d_out.data_ptr())), ("out NULL", gpu.composite_crh_dev(d_m.data_ptr(), moff, 9, 0)),
                      ("msgs NULL", gpu.composite_crh_dev(0, moff, 9, d_out.data_ptr())), ("decreasing offsets", gpu.composite_crh_dev(d_m.data_ptr(), dec, 9, d_out.data_ptr())),
                      ("past the generator table", gpu.composite_crh_dev(d_long.data_ptr(), long_off, 1, d_out.data_ptr()))):
        assert rc == 2, label
    assert (d_out.cpu().numpy() == 0xA5).all()
    # n = 0: nothing to do, in every form
    assert gpu.composite_crh_dev(0, None, 0, 0) == 0
    for mode in range(4):
        assert gpu.hash_to_g1_dev(DOMAIN, 0, np.zeros(1, dtype=np.uint64), 0, None, 0, 0, 0, mode=mode) == 0


def test_a_device_call_and_a_host_call_from_two_threads(gpu):
    msgs, extras = _messages(257, 9)
    want = {m: _hash_host(gpu, msgs, extras, m) for m in (0, 3)}
    got, errors = {}, []

    def run(kind, mode):
        try:
            for _ in range(3):
                got[kind] = _hash_dev(gpu, msgs, extras, mode)[1:] if kind == "dev" else _hash_host(gpu, msgs, extras, mode)
        except Exception as e:      # noqa: BLE001
            errors.append(e)
    for dev_mode, host_mode in ((3, 0), (0, 3)):
        ts = [threading.Thread(target=run, args=("dev", dev_mode)), threading.Thread(target=run, args=("host", host_mode))]
        [t.start() for t in ts]
        [t.join() for t in ts]
        assert not errors, errors
        for kind, mode in (("dev", dev_mode), ("host", host_mode)):
            assert np.array_equal(got[kind][0], want[mode][0]) and np.array_equal(got[kind][1], want[mode][1])
