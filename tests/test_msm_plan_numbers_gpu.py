"""GPU (-m gpu): the shape decisions of the big-MSM driver (csrc/msm_engine.h plan / fixed_plan / big_layout) on every path of run_device_windows -
resident, GLV split, window shard, fixed base in both forms, host-pointer pipeline, batched affine - at the smallest shape that reaches it: the
window size, the window count and the bucket count that msm_timings reports after the call.  The VALUES of the same paths are checked against the
oracle elsewhere (tests/test_msm_gpu.py, test_fixed_base_gpu.py, test_host_pipeline_gpu.py, test_multi_device_gpu.py, test_msm_ba_gpu.py); here
the points come from gen_points_dev and no oracle time is spent."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

G1, G2, BW = "bls12_377_g1", "bls12_377_g2", "bw6_761_g1"

# (window_bits, windows, buckets) per call, RECORDED on an MI355X from commit 2647c4a ("Load and write serialized Groth16 proving keys over BLS12-377"),
# the parent of the driver's split into stages - never taken from the code under test.  Three of them follow from that commit's rules by hand:
# G1 n = 300: c = 11, (253 + 11) / 11 = 24 windows of 2^10 buckets; G1 n = 2^15: c = 15, 17 windows of 2^14; BW6-761 n = 40: c = 9, (377 + 9) / 9 = 42 of 2^8.
EXPECTED = {
    "g1_300": (11, 24, 24576),
    "g1_2^15": (15, 17, 278528),
    "g1_glv_2^14": (16, 8, 262144),                # 2^15 expanded terms of 127 bits
    "g2_300": (11, 24, 24576),
    "bw6_40": (9, 42, 10752),
    "bw6_2048": (13, 30, 122880),
    "g1_shard_2^13": (11, 12, 12288),              # the last shard's half of the 24 windows
    "g1_fixed_cf16": (16, 1, 32768),               # NV = 1 virtual window
    "g1_fixed_cf17": (16, 3, 98304),               # NV = 3: the digits are compacted by window first
    "g1_host_pipeline_2^17": (15, 17, 278528),
    "bw6_ba_2^12": (13, 30, 122880),
}


def _inputs(group, n, seed):
    from celo_bls_snark_rs_amd import synthetic as syn
    pts = syn.device_points(group, n, seed)
    sc = syn.uniform_scalars(group, n, seed + 1)
    return pts, sc, torch.from_numpy(sc.view(np.int64)).cuda()


def _host_rows(gpu, group, pts):
    return pts.cpu().numpy().view(np.uint64).reshape(-1, gpu.GROUP_SHAPE[group][0])


def _shape(gpu, group):
    t = gpu.msm_timings(group)
    return t["window_bits"], t["windows"], t["buckets"]


@pytest.mark.parametrize("name,group,n,subgroup", [("g1_300", G1, 300, False), ("g1_2^15", G1, 1 << 15, False), ("g1_glv_2^14", G1, 1 << 14, True),
                                                   ("g2_300", G2, 300, False), ("bw6_40", BW, 40, False), ("bw6_2048", BW, 2048, False)])
def test_resident_calls(gpu, name, group, n, subgroup):
    pts, _, d_sc = _inputs(group, n, 11)
    gpu.msm_dev(group, pts.data_ptr(), 0, d_sc.data_ptr(), n, subgroup=subgroup)
    assert _shape(gpu, group) == EXPECTED[name]


def test_window_shard(gpu):
    pts, sc, _ = _inputs(G1, 1 << 13, 21)
    gpu.msm_multi_windows(G1, [0, 0], _host_rows(gpu, G1, pts), None, sc)
    assert _shape(gpu, G1) == EXPECTED["g1_shard_2^13"]


@pytest.mark.parametrize("cf", [16, 17])
def test_fixed_base_uncompacted_and_compacted(gpu, cf):
    pts, _, d_sc = _inputs(G1, 300, 31)
    fb = gpu.FixedBase(G1, d_bases=pts.data_ptr(), n=300, window_bits=cf)
    try:
        fb.msm_dev(d_sc.data_ptr(), 300)
    finally:
        fb.release()
    assert _shape(gpu, G1) == EXPECTED["g1_fixed_cf%d" % cf]


def test_host_pointer_pipeline(gpu):
    pts, sc, _ = _inputs(G1, 1 << 17, 41)
    xy = _host_rows(gpu, G1, pts)
    gpu.set_host_chunks(2)
    try:
        gpu.msm(G1, xy, None, sc)
    finally:
        gpu.set_host_chunks(-1)
    assert _shape(gpu, G1) == EXPECTED["g1_host_pipeline_2^17"]


def test_batched_affine(gpu):
    pts, _, d_sc = _inputs(BW, 1 << 12, 51)
    gpu.set_batched_affine(1)
    try:
        gpu.msm_dev(BW, pts.data_ptr(), 0, d_sc.data_ptr(), 1 << 12)
    finally:
        gpu.set_batched_affine(-1)
    assert _shape(gpu, BW) == EXPECTED["bw6_ba_2^12"]
