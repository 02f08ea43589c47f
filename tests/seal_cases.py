"""The cases of verify_aggregated_seals_bls12_377 (csrc/unit_seals.hip), shared by tests/test_seal_cases.py (which proves on the CPU that each
constructed verdict is the truth) and tests/test_verify_seals_gpu.py.  Keys are seeded secrets sk_j with pk_j = sk_j G2; a seal's valid
signature is [(sum of the selected sk_j) mod r] H(m).  This module holds data only: who signs what under which key, which bytes replace a
signature, and the status the contract then demands.  The curve work is the caller's (Python on the CPU, the library on the GPU)."""
import random
import numpy as np
from oracle.py import ecc

CLASSES = ("valid", "wrong message", "bit flipped", "another seal's signature", "undecodable", "outside G1", "one signer short", "threshold met exactly",
           "zero signers")
# the classes whose seals are clean and whose product is one, or that never reach a product: a batch of these passes the combined check
NO_BAD_PRODUCT = ("valid", "undecodable", "threshold met exactly", "outside G1", "one signer short", "zero signers")
STATUS = {"valid": 0, "wrong message": 4, "bit flipped": 4, "another seal's signature": 4, "undecodable": 2, "outside G1": 2, "one signer short": 1,
          "threshold met exactly": 0, "zero signers": 1}
EXTRA = b"\x01\x02"


def secret_keys(n, seed=2024):
    rng = random.Random(seed)
    return [rng.randrange(1, ecc.R377) for _ in range(n)]


def undecodable_signature():
    """x = q, not below the modulus: no encoding of a field element"""
    return ecc.Q377.to_bytes(48, "little")


def point_outside_g1():
    """a point of the curve y^2 = x^3 + 1 that the cofactor does not kill, in compressed form"""
    x = 2
    while True:
        y = ecc.sqrt_fp((x * x * x + 1) % ecc.Q377, ecc.Q377)
        if y is not None and not ecc.E1_377.in_subgroup((x, y)):
            return ecc.ser_point(ecc.E1_377, (x, y))
        x += 1


def message(i, tag):
    return ("block %d of epoch %s" % (i, tag)).encode()


class Batch:
    """m seals over n keys.  sets: None for one shared set of keys 0 .. n - 1, else per seal the list of key indices it owns.  Per seal i:
    bitmap[i] (over its set), msg[i], min_signers[i], sign_key[i] and sign_msg[i] (what an honest signer of that scalar and message produces),
    raw[i] (bytes that replace the signature, or None), label[i], status[i].  Seal i is of class classes[(i + rotation) % len(classes)]."""

    def __init__(self, m, n, rotation, seed, tag, per_seal_sets=False, classes=CLASSES):
        rng = random.Random(seed)
        self.m, self.n, self.sks = m, n, secret_keys(n)
        self.sets = None
        if per_seal_sets:
            self.sets = [sorted(rng.sample(range(n), rng.randrange(3, n + 1))) for _ in range(m)]
        self.bitmap, self.msg, self.min_signers, self.sign_key, self.sign_msg, self.raw, self.label, self.status = [], [], [], [], [], [], [], []
        bad_sig, off_g1 = undecodable_signature(), point_outside_g1()
        for i in range(m):
            cls = classes[(i + rotation) % len(classes)]
            own = list(range(n)) if self.sets is None else self.sets[i]
            k = len(own)
            bits = [0] * k
            for j in rng.sample(range(k), rng.randrange(2 * k // 3 + 1, k + 1)):
                bits[j] = rng.choice((1, 1, 1, 0x80, 0xFF))         # any non-zero byte is "set"
            count = sum(1 for b in bits if b)
            msg, sign_msg, sign_bits, raw, mins = message(i, tag), message(i, tag), list(bits), None, rng.randrange(0, count)
            if cls == "wrong message":
                sign_msg = message(i, tag + "'")
            elif cls == "bit flipped":                              # signed by the set the bitmap names, but for one key
                j = rng.randrange(k)
                sign_bits[j] = 0 if sign_bits[j] else 1
            elif cls == "another seal's signature":                 # a valid signature: of other signers on another block
                sign_msg = message(i + 1, tag)
                sign_bits = [1 if j % 2 == 0 else 0 for j in range(k)] if any(bits[j] and j % 2 for j in range(k)) else [1] * k
            elif cls == "undecodable":
                raw = bad_sig
            elif cls == "outside G1":
                raw = off_g1
            elif cls == "one signer short":
                mins = count + 1
            elif cls == "threshold met exactly":
                mins = count
            elif cls == "zero signers":
                bits, mins = [0] * k, 0                             # its signature stays a valid one of the intended signers
            self.bitmap.append(bits)
            self.msg.append(msg)
            self.min_signers.append(mins)
            self.sign_key.append(sum(self.sks[own[j]] for j in range(k) if sign_bits[j]) % ecc.R377)
            self.sign_msg.append(sign_msg)
            self.raw.append(raw)
            self.label.append("%d: %s" % (i, cls))
            self.status.append(STATUS[cls])

    def offsets(self):
        if self.sets is None:
            return np.array([0, self.n], dtype=np.uint32)
        return np.cumsum([0] + [len(s) for s in self.sets]).astype(np.uint32)

    def key_rows(self):
        """the indices of the keys in row order (per-seal sets repeat keys)"""
        return list(range(self.n)) if self.sets is None else [j for s in self.sets for j in s]

    def bits(self):
        if self.sets is None:
            return np.array(self.bitmap, dtype=np.uint8).reshape(self.m, self.n)
        return np.concatenate([np.asarray(b, dtype=np.uint8) for b in self.bitmap])

    def signatures(self, signed):
        """signed: (m, 48) honest signatures of (sign_key, sign_msg); returns the seals' signatures with the raw replacements in place"""
        out = np.array(signed, dtype=np.uint8).reshape(self.m, 48).copy()
        for i, raw in enumerate(self.raw):
            if raw is not None:
                out[i] = np.frombuffer(raw, dtype=np.uint8)
        return out
