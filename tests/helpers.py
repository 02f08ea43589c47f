"""Shared test helpers: seeded workloads and oracle/product comparisons."""
import numpy as np
from oracle.py import ecc
from oracle import cpu_oracle as co


def seeded_scalars(n, seed, modulus, edge=True):
    rng = ecc.SplitMix64(seed)
    sc = [ecc.random_scalar(rng, modulus) for _ in range(n)]
    if edge and n >= 8:
        sc[0] = 0
        sc[1] = 1
        sc[2] = modulus - 1
        sc[3] = 1 << 64
        sc[4] = (1 << 136) - 1  # Batch::verify-sized exponent (crates/bls-crypto/src/bls/batch.rs:23-28)
        sc[5] = 2
    return sc


def seeded_points(curve, gen, n, seed):
    rng = ecc.SplitMix64(seed)
    return [curve.mul(gen, rng.next() | 1) for _ in range(n)]


def scalars_np(sc, limbs):
    return co.ints_to_limbs(sc, limbs)


def splitmix64_at(seed, i):
    M = (1 << 64) - 1
    z = (seed + (i + 1) * 0x9E3779B97F4A7C15) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)


def build_hosttest():
    """Builds (make decides whether anything is stale) and returns the path of the host-only bounds-tracking library: host_test.cpp
    with -DCELO_FP_TRACK plus the host units it exercises (the IFMA Horner epilogue and the CPU probe)."""
    import os, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "celo-bls-snark-rs_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", csrc, "../build/libcelo_hosttest.so"])
    return os.path.join(root, "celo-bls-snark-rs_amd", "build", "libcelo_hosttest.so")


def groth16_setup(golden):
    """(vk, proof, public inputs) of the reference's Groth16 known-answer vector (crates/bls-snark-sys/src/snark/mod.rs:52-119) from
    tests/golden/reference_vectors.json: the inputs are the packed hash of its first and last epoch block"""
    from oracle.py import epoch as ep
    g = golden["groth16_bw6_761"]
    vk = ep.parse_vk(bytes.fromhex(g["vk"]))
    pr = ep.parse_proof(bytes.fromhex(g["proof"]))

    def pks(hx):
        b = bytes.fromhex(hx)
        return [ecc.deser_point(ecc.E2_377, b[96 * i:96 * i + 96]) for i in range(len(b) // 96)]

    first = ep.EpochBlock(g["first"]["index"], g["first"]["round"], bytes.fromhex(g["first_epoch_entropy"]),
                          bytes.fromhex(g["first_parent_entropy"]), g["first"]["maximum_non_signers"],
                          g["first"]["maximum_validators"], pks(g["first_pubkeys"]))
    last = ep.EpochBlock(g["last"]["index"], g["last"]["round"], bytes.fromhex(g["last_epoch_entropy"]),
                         bytes.fromhex(g["last_parent_entropy"]), g["last"]["maximum_non_signers"],
                         g["last"]["maximum_validators"], pks(g["last_pubkeys"]))
    inputs = ep.pack(ep.hash_first_last_epoch_block(first, last))
    return vk, pr, inputs
