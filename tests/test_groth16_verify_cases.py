"""CPU (-m "not gpu"): the constructed Groth16 proofs of tests/groth16_verify_cases.py against the oracle, the exponent rule, the host twins
of the verifier's lane routines under bounds tracking, the argument refusals and the serialized key parse.

Mutation pairs of the verifier (tests/test_groth16_verify_gpu.py runs them on the device): all r_i = 1 -> the cancelling pair; dropping the
input range test -> the r / r + 1 inputs; an off-by-one in the window count -> the all-ones inputs; the k = 7 / 8 border -> m = 4 / 5."""
import ctypes as C
import numpy as np
import pytest
from oracle.py import ecc
from oracle.py import epoch as ep
from oracle import cpu_oracle as co
from tests import groth16_verify_cases as gc
from tests import helpers as H

R = gc.R


@pytest.fixture(scope="module")
def key2():
    return gc.Key(2, 0x6116)


@pytest.fixture(scope="module")
def ht():
    return C.CDLL(H.build_hosttest())


def test_builder_verdicts_equal_the_oracles(key2):
    """every case class once, the cancelling and the swapped pair: the verdict the scalars give is the oracle's product of the four pairs"""
    rng = ecc.SplitMix64(11)
    proofs = [gc.special_proof(key2, rng, k) for k in gc.classes_for(key2)] + list(gc.cancelling_pair(key2, rng)) + list(gc.swapped_pair(key2, rng))
    b = gc.Batch(key2, proofs)
    want = {"valid": 1, "rerandomised": 1, "inf_a_accept": 1, "edge_0": 1, "edge_1": 1, "edge_rm1": 1, "edge_ones": 1}
    for i, p in enumerate(proofs):
        assert b.expect[i] == want.get(p.kind, 0), p.kind
        assert gc.oracle_verdict(b, i) == b.expect[i], p.kind


def test_key_without_inputs_and_identity_cases():
    key0 = gc.Key(0, 5)
    rng = ecc.SplitMix64(12)
    proofs = [gc.special_proof(key0, rng, k) for k in gc.classes_for(key0)]
    assert {p.kind for p in proofs}.isdisjoint(gc.INPUT_CLASSES)
    b = gc.Batch(key0, proofs)
    for i in range(b.m):
        assert gc.oracle_verdict(b, i) == b.expect[i], proofs[i].kind


def test_exponent_rule_restated():
    """the top bit is set, the low 127 bits are the stream's, block i belongs to proof i; the block function is pinned on RFC 7539
    section 2.3.2 (key 00 .. 1f, counter 1, nonce 00 00 00 09 00 00 00 4a 00 00 00 00: its words 13 and 14)"""
    key = np.arange(8, dtype=np.uint32) * 0x04040404 + 0x03020100
    rfc = gc.chacha20_block(key, 1 | (0x09000000 << 32), tail=(0x4A000000, 0))
    assert rfc[0] == 0xE4E7F110 and rfc[1] == 0x15593BD1 and rfc[15] == 0x4E3C50A2
    ex = gc.exponents_ref(key, 5)
    assert all(e >> 127 == 1 and e < 1 << 128 for e in ex) and len(set(ex)) == 5
    b = gc.chacha20_block(key, 3)
    assert ex[3] & ((1 << 127) - 1) == (b[0] | b[1] << 32 | b[2] << 64 | b[3] << 96) & ((1 << 127) - 1)


def test_cancelling_pair_passes_unweighted_and_fails_weighted(key2):
    """the reason the combination is random: (C_1 + D, C_2 - D) satisfies the combined equation with r = (1, 1) and not with drawn exponents"""
    b = gc.Batch(key2, list(gc.cancelling_pair(key2, ecc.SplitMix64(13))))
    assert b.expect.tolist() == [0, 0]
    assert gc.oracle_combined(b, [1, 1]) == 1
    assert gc.oracle_combined(b, gc.exponents_ref(np.arange(8, dtype=np.uint32), 2)) == 0
    ok = gc.batch_with(key2, 2, {}, 14)
    assert gc.oracle_combined(ok, gc.exponents_ref(np.arange(8, dtype=np.uint32), 2)) == 1


@pytest.mark.parametrize("n_in", [0, 1, 2, 3, 8])
def test_host_twin_input_row(ht, n_in):
    """ht_g16_input_row (the body of k_g16_inputs, bounds tracked) against the oracle's MSM: the edge inputs, random ones, r and r + 1"""
    key = gc.Key(n_in, 100 + n_in)
    rng = ecc.SplitMix64(200 + n_in)
    xs = [[v] * n_in for v in gc.EDGE_INPUTS] + [[ecc.random_scalar(rng, R) for _ in range(n_in)] for _ in range(2)]
    if n_in:
        xs += [[R] + [1] * (n_in - 1), [2] * (n_in - 1) + [R + 1]]
    n = len(xs)
    inputs = co.ints_to_limbs([v for x in xs for v in x], 6).reshape(n, n_in, 6) if n_in else np.zeros((n, 0, 6), dtype=np.uint64)
    for c in ({0: (4,), 8: (7,)}.get(n_in, (4, 5))):
        out = np.zeros((n, 24), dtype=np.uint64)
        inf = np.zeros(n, dtype=np.uint8)
        st = np.zeros(n, dtype=np.uint8)
        abc = np.ascontiguousarray(key.abc)
        ht.ht_g16_input_row(co._p(abc), C.c_size_t(n_in + 1), co._p(inputs), C.c_size_t(n), C.c_int(c), co._p(out), co._p(inf), co._p(st))
        assert st.tolist() == [0 if all(v < R for v in x) else 1 for x in xs]
        good = [i for i in range(n) if not st[i]]
        want, winf = gc.acc_rows(key, inputs[good])
        assert np.array_equal(out[good], want) and np.array_equal(inf[good], winf), (n_in, c)


def test_host_twin_scale(ht):
    """ht_g16_scale (the body of k_g16_scale) against orc_mul_bw6_761: 2^127, 2^128 - 1, random exponents; a point of small x"""
    G1, _ = gc.generators()
    rng = ecc.SplitMix64(31)
    small = next(P for P in ((x, ecc.sqrt_fp((x ** 3 - 1) % ecc.Q761, ecc.Q761)) for x in range(2, 200)) if P[1] is not None)
    pts = np.concatenate([gc.mul_rows(G1, [1 + ecc.random_scalar(rng, R - 1) for _ in range(4)])[0], co.pack_761([small])[0]])
    exps = [1 << 127, (1 << 128) - 1, (1 << 127) | ecc.random_scalar(rng, 1 << 127), (1 << 127) | ecc.random_scalar(rng, 1 << 127), (1 << 127) | 5]
    r2 = co.ints_to_limbs([e & ((1 << 127) - 1) for e in exps], 2)            # the top bit is the routine's own
    n = len(exps)
    out = np.zeros((n, 24), dtype=np.uint64)
    inf = np.zeros(n, dtype=np.uint8)
    ht.ht_g16_scale(co._p(np.ascontiguousarray(pts)), co._p(r2), C.c_size_t(n), co._p(out), co._p(inf))
    for i in range(n):
        k6 = co.ints_to_limbs([exps[i]], 6)[0]
        jac = np.zeros(36, dtype=np.uint64)
        assert co.lib().orc_mul_bw6_761(co._p(np.ascontiguousarray(pts[i])), co._p(k6), co._p(jac)) == 0
        assert co.jac_to_affine(jac, "761") == tuple(co.from_mont(out[i].reshape(2, 12), ecc.Q761)) and inf[i] == 0, i


def test_window_bits_stay_within_the_budget(ht):
    got = {n: ht.ht_g16_window_bits(C.c_size_t(n)) for n in (0, 1, 2, 3, 8, 15, 16, 64)}
    assert got[1] == 10 and got[15] == 10 and got[16] == 9 and got[64] == 7
    for n, c in got.items():
        windows = (377 + 1 + c - 1) // c
        assert n * windows * (1 << (c - 1)) * 224 <= 64 << 20


def test_argument_refusals_need_no_device():
    from celo_bls_snark_rs_amd import ffi
    lib = ffi.lib()
    z = np.zeros(24, dtype=np.uint64)
    abc = np.zeros((66, 24), dtype=np.uint64)
    h = C.c_void_p()
    p = co._p
    assert lib.groth16_vk_load_bw6_761(None, p(z), p(z), p(z), p(abc), C.c_size_t(1), C.byref(h)) == 2
    assert lib.groth16_vk_load_bw6_761(p(z), p(z), p(z), p(z), None, C.c_size_t(1), C.byref(h)) == 2
    assert lib.groth16_vk_load_bw6_761(p(z), p(z), p(z), p(z), p(abc), C.c_size_t(1), None) == 2
    assert lib.groth16_vk_load_bw6_761(p(z), p(z), p(z), p(z), p(abc), C.c_size_t(0), C.byref(h)) == 2
    assert lib.groth16_vk_load_bw6_761(p(z), p(z), p(z), p(z), p(abc), C.c_size_t(66), C.byref(h)) == ffi.VK_ERR_INPUTS == 36
    short = np.zeros(391, dtype=np.uint8)
    assert lib.groth16_vk_load_bw6_761_serialized(p(short), C.c_size_t(391), C.byref(h)) == 30
    assert lib.groth16_vk_load_bw6_761_serialized(None, C.c_size_t(500), C.byref(h)) == 2
    hdr = np.zeros(392 + 96, dtype=np.uint8)
    hdr[384] = 2                                       # two rows announced, one present
    assert lib.groth16_vk_load_bw6_761_serialized(p(hdr), C.c_size_t(hdr.size), C.byref(h)) == 30
    hdr[384] = 66
    assert lib.groth16_vk_load_bw6_761_serialized(p(hdr), C.c_size_t(hdr.size), C.byref(h)) == 36
    assert not h.value
    assert lib.groth16_vk_free(None) == 2
    out = np.zeros(1, dtype=np.uint8)
    assert lib.groth16_verify_batch_bw6_761(None, p(z), None, p(z), None, p(z), None, None, C.c_size_t(0), C.c_int(0), None, p(out)) == 0      # m = 0
    assert lib.groth16_verify_batch_bw6_761(None, p(z), None, p(z), None, p(z), None, None, C.c_size_t(1), C.c_int(0), None, p(out)) == 2
    assert lib.groth16_verify_batch_bw6_761(C.c_void_p(0x1000), p(z), None, p(z), None, p(z), None, None, C.c_size_t(1), C.c_int(0), None, p(out)) == 2   # no live handle
    assert lib.groth16_verify_batch_bw6_761_serialized(C.c_void_p(0x1000), None, None, C.c_size_t(1), C.c_int(0), None, p(out)) == 2
    assert lib.celo_amd_groth16_draw_exponents(None, C.c_size_t(1), p(z)) == 2
    assert lib.celo_amd_groth16_verify_last(None, None, None) == 0


def test_serialized_key_parse_matches_the_oracle(ht, golden, key2):
    """groth16_vk_load_bw6_761_serialized's host parse (g16_vk_parse, through its twin) on the reference's own verifying key against
    oracle.py.epoch.parse_vk, on a constructed key's serialization, and its refusals"""
    def parse(data, cap=70):
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        rows = np.zeros((cap, 24), dtype=np.uint64)
        inf = np.zeros(cap, dtype=np.uint8)
        n = C.c_uint64(0)
        rc = ht.ht_g16_vk_parse(co._p(buf), C.c_size_t(buf.size), C.c_size_t(cap), co._p(rows), co._p(inf), C.byref(n))
        return rc, rows[:4 + n.value], inf[:4 + n.value]
    data = bytes.fromhex(golden["groth16_bw6_761"]["vk"])
    vk = ep.parse_vk(data)
    rc, rows, inf = parse(data)
    assert rc == 0 and not inf.any()
    want = co.pack_761([vk["alpha_g1"], vk["beta_g2"], vk["gamma_g2"], vk["delta_g2"]] + list(vk["gamma_abc_g1"]))[0]
    assert np.array_equal(rows, want)
    rc, rows, inf = parse(key2.serialize())
    assert rc == 0 and np.array_equal(rows, np.concatenate([np.stack([key2.alpha, key2.beta, key2.gamma, key2.delta]), key2.abc]))
    assert parse(data[:-1])[0] == 30 and parse(data + b"\0")[0] == 31
    bad = bytearray(data)
    bad[392 + 5] ^= 1                                  # gamma_abc[0]: another x - off the curve or off the subgroup
    assert parse(bad)[0] == 33
