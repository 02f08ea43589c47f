"""The cases of verify_epoch_transitions_bls12_377 (csrc/unit_transitions.hip, csrc/transitions.h), shared by tests/test_transition_cases.py
(which proves on the CPU that each constructed verdict is the truth) and tests/test_transitions_gpu.py.  Keys come from a pool of seeded secrets
sk_j with pk_j = sk_j G2 (entry PAD of the pool is sk = 1: the padding key, the G2 generator); a transition's valid signature is
[(sum of the selected sk_j of the predecessor) mod r] H(inner encoding of the block, its 7 extra bytes) under the composite CIP22 hasher.

This module holds data only: the fields of every block, who signs what, which bytes replace a signature, and the status the contract then
demands in either mode.  The curve work, the encodings and the hashes are the caller's (Python on the CPU, the library on the GPU).

One chain carries ONE class, at transition `pos` (1 = the first transition); every other transition of the chain is valid, except where the
class itself reaches further (a bad key spoils the next transition too; the cancelling pair is two transitions)."""
import random
import numpy as np
from oracle.py import ecc

CLASSES = ("valid", "bad key in b", "bad key in p", "index + 2", "index 0", "key count changed", "wrong parent entropy", "wrong parent entropy, initial zero",
           "threshold met exactly", "one signer short", "padding key selected", "padding key unselected", "undecodable signature", "signature outside G1",
           "wrong message", "bit flipped", "cancelling pair")
# the status of the transition that carries the class, mode 0
STATUS = {"valid": 0, "bad key in b": 1, "bad key in p": 2, "index + 2": 3, "index 0": 3, "key count changed": 4, "wrong parent entropy": 5,
          "wrong parent entropy, initial zero": 0, "threshold met exactly": 0, "one signer short": 6, "padding key selected": 7, "padding key unselected": 0,
          "undecodable signature": 8, "signature outside G1": 8, "wrong message": 10, "bit flipped": 10, "cancelling pair": 10}
POOL = 12                # secrets 0 .. POOL - 1
PAD = POOL               # the padding key's place in the pool (sk = 1)
BAD = -1                 # a key whose bytes do not decode
DELTA = 7                # the cancelling pair: sig + [7] G1 and sig - [7] G1


def secret_keys(seed=2025):
    rng = random.Random(seed)
    return [rng.randrange(2, ecc.R377) for _ in range(POOL)] + [1]


def undecodable_key(enc96):
    """x.c0 = q, not below the modulus: no encoding of a field element"""
    return ecc.Q377.to_bytes(48, "little") + bytes(enc96[48:])


def undecodable_signature():
    return ecc.Q377.to_bytes(48, "little")


def point_outside_g1():
    """a point of the curve y^2 = x^3 + 1 that the cofactor does not kill, in compressed form"""
    x = 2
    while True:
        y = ecc.sqrt_fp((x * x * x + 1) % ecc.Q377, ecc.Q377)
        if y is not None and not ecc.E1_377.in_subgroup((x, y)):
            return ecc.ser_point(ecc.E1_377, (x, y))
        x += 1


class Block:
    """index, round, mns, maxv, ee / pe (16 bytes), keys (pool indices, BAD for bytes that do not decode), bits (bytes over its own keys: who
    signs the NEXT block).  A transition also has: sign_bits (whom the honest signer sums), sign_flip (the signer's extra data has one bit
    flipped: another message), raw (bytes that replace the signature), delta (+1 / -1: DELTA G1 added / subtracted), label."""
    def __init__(self):
        self.raw, self.delta, self.sign_flip, self.sign_bits, self.label = None, 0, False, None, ""


def _chain(rng, n_tr, cls, pos, n_keys, tag):
    assert 1 <= pos <= n_tr and (cls != "cancelling pair" or pos < n_tr)
    blocks = []
    index = rng.randrange(1, 60000)
    prev_ee = None
    for b in range(n_tr + 1):
        k = Block()
        k.index, k.round, k.mns = index + b, rng.randrange(256), 2
        k.maxv = n_keys + rng.choice((-1, 0, 2))
        k.ee = bytes(rng.randrange(1, 256) for _ in range(16))
        k.pe = prev_ee if b else bytes(rng.randrange(256) for _ in range(16))
        prev_ee = k.ee
        k.keys = rng.sample(range(POOL), n_keys)
        k.bits = [rng.choice((1, 1, 0x80, 0xFF)) for _ in range(n_keys)]
        k.bits[rng.randrange(n_keys)] = 0                       # n - 1 of n sign: above the threshold n - 2, one key left to flip
        k.label = "%s/%d: %s" % (tag, b, "initial" if b == 0 else "valid")
        blocks.append(k)
    st = [0] * (n_tr + 1)
    b, p = blocks[pos], blocks[pos - 1]
    b.label = "%s/%d: %s" % (tag, pos, cls)
    st[pos] = STATUS[cls]
    if cls == "bad key in b":
        b.keys[rng.randrange(n_keys)] = BAD
        if pos < n_tr:
            st[pos + 1] = 2
    elif cls == "bad key in p":
        p.keys[rng.randrange(n_keys)] = BAD
        st[pos - 1] = 1
    elif cls == "index + 2":
        for k in blocks[pos:]:
            k.index += 1
    elif cls == "index 0":
        for j, k in enumerate(blocks[pos:]):
            k.index = j
    elif cls == "key count changed":
        for k in blocks[pos:]:
            k.keys.append(next(j for j in range(POOL) if j not in k.keys))
            k.bits.append(1)
    elif cls == "wrong parent entropy":
        b.pe = bytes(x ^ 0x55 for x in p.ee)
    elif cls == "wrong parent entropy, initial zero":
        b.pe = bytes(x ^ 0x55 for x in p.ee)
        blocks[0].ee = bytes(16)
        if pos > 1:
            blocks[1].pe = bytes(16)
    elif cls == "threshold met exactly":
        p.mns = 1
    elif cls == "one signer short":
        p.mns = 0
    elif cls == "padding key selected":
        p.keys[next(j for j in range(n_keys) if p.bits[j])] = PAD
    elif cls == "padding key unselected":
        p.keys[p.bits.index(0)] = PAD
    elif cls == "undecodable signature":
        b.raw = undecodable_signature()
    elif cls == "signature outside G1":
        b.raw = point_outside_g1()
    elif cls == "wrong message":
        b.sign_flip = True
    elif cls == "cancelling pair":
        b.delta, blocks[pos + 1].delta = 1, -1
        blocks[pos + 1].label = "%s/%d: %s" % (tag, pos + 1, cls)
        st[pos + 1] = 10
    for j in range(1, n_tr + 1):
        blocks[j].sign_bits = [1 if x else 0 for x in blocks[j - 1].bits]
    if cls == "bit flipped":                                    # signed by the set the bitmap named before one more byte was set
        p.bits[p.bits.index(0)] = 1
    st1 = [0] * (n_tr + 1) if cls == "cancelling pair" else list(st)
    return blocks, st, st1


class Batch:
    """chains: a list of (transitions, class, pos).  blocks: every Block in call order; chain_off; status[mode][b]; chain_ok[mode][c];
    path[mode] (celo_amd_transitions_last)."""
    def __init__(self, chains, seed, n_keys=5, tag="t"):
        rng = random.Random(seed)
        self.sks = secret_keys()
        self.blocks, self.chain_off, self.status, self.chain_ok, self.chains = [], [0], {0: [], 1: []}, {0: [], 1: []}, list(chains)
        fell_back = False
        for c, (n_tr, cls, pos) in enumerate(chains):
            blocks, st0, st1 = _chain(rng, n_tr, cls, pos, n_keys, "%s%d" % (tag, c))
            self.blocks += blocks
            self.chain_off.append(len(self.blocks))
            self.status[0] += st0
            self.status[1] += st1
            self.chain_ok[0].append(int(not any(st0)))
            self.chain_ok[1].append(int(not any(st1)))
            fell_back = fell_back or (10 in st1 and set(st1) <= {0, 10})
        self.path = {0: 0, 1: 2 if fell_back else 1}
        self.nb = len(self.blocks)
        self.initial = [False] * self.nb
        for o in self.chain_off[:-1]:
            self.initial[o] = True
        self.label = [k.label for k in self.blocks]

    def key_off(self):
        return np.cumsum([0] + [len(k.keys) for k in self.blocks]).astype(np.uint32)

    def bits(self):
        return np.array([x for k in self.blocks for x in k.bits], dtype=np.uint8)

    def key_bytes(self, pool_enc):
        """pool_enc: the POOL + 1 compressed keys; -> (key_off[nb], 96) uint8"""
        rows = [undecodable_key(pool_enc[0]) if j == BAD else bytes(pool_enc[j]) for k in self.blocks for j in k.keys]
        return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(-1, 96)

    def fields(self, entropies=True):
        f = dict(index=[k.index for k in self.blocks], round_=[k.round for k in self.blocks], max_non_signers=[k.mns for k in self.blocks],
                 max_validators=[k.maxv for k in self.blocks])
        f["epoch_entropy"] = np.frombuffer(b"".join(k.ee for k in self.blocks), dtype=np.uint8).reshape(-1, 16) if entropies else None
        f["parent_entropy"] = np.frombuffer(b"".join(k.pe for k in self.blocks), dtype=np.uint8).reshape(-1, 16) if entropies else None
        return f

    def sign_keys(self):
        """per block the scalar its honest signer holds (0 for an initial block)"""
        out = []
        for b, k in enumerate(self.blocks):
            if self.initial[b]:
                out.append(0)
                continue
            p = self.blocks[b - 1]
            out.append(sum(self.sks[j] for j, x in zip(p.keys, k.sign_bits) if x and j != BAD) % ecc.R377)
        return out

    def sign_extra(self, b, extra7):
        """the 7 extra bytes block b's signer signs over"""
        e = bytes(extra7)
        return bytes([e[0] ^ 1]) + e[1:] if self.blocks[b].sign_flip else e

    def signatures(self, signed):
        """signed: (nb, 48) honest signatures of (sign_keys, inner, sign_extra); -> the call's signatures with the replacements and the deltas in place"""
        out = np.array(signed, dtype=np.uint8).reshape(self.nb, 48).copy()
        E = ecc.E1_377
        D = E.mul(ecc.G1_377, DELTA)
        for b, k in enumerate(self.blocks):
            if k.raw is not None:
                out[b] = np.frombuffer(k.raw, dtype=np.uint8)
            elif k.delta:
                P = ecc.deser_point(E, out[b].tobytes())
                out[b] = np.frombuffer(ecc.ser_point(E, E.add(P, D if k.delta > 0 else E.neg(D))), dtype=np.uint8)
        return out


def every_class_everywhere():
    """every class at every position of chains of 1 to 9 transitions, spread over batches of 65 transitions; -> a list of chain lists"""
    all_chains = []
    for cls in CLASSES:
        for n_tr in range(1, 10):
            for pos in range(1, n_tr + 1):
                if cls == "cancelling pair" and pos == n_tr:
                    continue
                all_chains.append((n_tr, cls, pos))
    random.Random(7).shuffle(all_chains)
    batches, cur, count = [], [], 0
    for ch in all_chains:
        if count + ch[0] > 65:
            cur.append((65 - count, "valid", 1)) if count < 65 else None
            batches.append(cur)
            cur, count = [], 0
        cur.append(ch)
        count += ch[0]
    if cur:
        if count < 65:
            cur.append((65 - count, "valid", 1))
        batches.append(cur)
    return batches


def small_cases():
    """one chain per class, two or three transitions each: the list the CPU test proves"""
    chains = []
    for i, cls in enumerate(CLASSES):
        n_tr = 2 + i % 2
        chains.append((n_tr, cls, 1 + i % 2 if cls != "cancelling pair" else 1))
    return chains
