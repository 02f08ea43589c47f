"""The loaded HashToBits circuit of m epochs with the parameters of a fixed setup, and seeded CRH rows: what the GPU tests of the helper proof's
verifier share (no GPU import at module level; `gpu` is the ffi module the tests' fixture returns)."""
import random
import numpy as np
from oracle.py import ecc
from oracle.py import groth16_prover as gp
from oracle import cpu_oracle as co
import groth16_setup_ref as gs
import hashbits_ref as hr
import r1cs_cases as rc

CURVE = "bls12_377"
P = hr.R377


def rows_for(m, seed):
    """m CRH rows of 48 bytes from a seed"""
    rng = random.Random(7000 * m + seed)
    return np.frombuffer(bytes(rng.randrange(256) for _ in range(48 * m)), dtype=np.uint8).reshape(m, 48).copy()


def domain_consts(log_n):
    k = gp.domain_constants(log_n, gs.root_of_unity(CURVE, log_n), gs.coset_generator(P), P)
    return {name: co.to_mont([v], P)[0] for name, v in k.items()}


class Circuit:
    """hash_to_bits_r1cs_load(m) and the library's setup over it with fixed toxic values: .r, .key (proving key), .vk_rows, .log_n, .consts"""
    def __init__(self, gpu, m):
        self.m, self.sizes = m, gpu.hash_to_bits_size(m)[1]
        self.log_n = self.sizes["log_n"]
        self.r = gpu.hash_to_bits_r1cs_load(m)
        rng = random.Random(11)
        tau, toxic = rng.randrange(2, P), [rng.randrange(1, P) for _ in range(4)]
        out = gpu.groth16_setup_r1cs(self.r, self.log_n, rc.mont([gs.root_of_unity(CURVE, self.log_n)], P)[0], rc.mont([tau], P)[0], rc.mont(toxic, P),
                                     gs.pack(CURVE, 1, [ecc.G1_377])[0][0], gs.pack(CURVE, 2, [ecc.G2_377])[0][0], want_rows=False, want_key=True)
        self.key, self.vk_rows = out["key"], out["vk"]
        self.consts = domain_consts(self.log_n)

    def release(self):
        self.key.release()
        self.r.release()
