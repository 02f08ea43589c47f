"""A Python restatement of csrc/dedup.h - the mix, the slot, the sequential table, key_dedup_pick - and the key sets of the de-duplication
tests.  No GPU import; numpy only.

A key set is an (n, kb) uint8 array, kb = 96 (G2) or 48 (G1).  The table here is the host twin's: keys inserted in index order.  What the
device may do differently is the order, so the tests assert exact representatives only on sets for which longest_run() shows that no probe
sequence can reach the cap in ANY insertion order: the set of occupied slots of a linear-probing table does not depend on the order."""
import numpy as np

M64 = (1 << 64) - 1
EMPTY = NONE = 0xFFFFFFFF
SLACK_DEFAULT, PROBES_DEFAULT, PROBES_MAX = 1, 64, 1024
N0 = 0          # csrc/dedup.h DEDUP_N0: the composed callers de-duplicate from N0 keys up under the rule; 0 = never


def key_dedup_pick(n):
    return N0 != 0 and n >= N0


def slots(n, slack_log=SLACK_DEFAULT):
    s = 1
    while s < n:
        s <<= 1
    return min(s << slack_log, 1 << 31)


def mix(key):
    """64 bits from the key's little-endian 64-bit words (bytes of length 48 or 96)"""
    key = bytes(key)
    words = len(key) // 8
    h = (0x9E3779B97F4A7C15 * (words + 1)) & M64
    for j in range(words):
        h ^= int.from_bytes(key[8 * j:8 * j + 8], "little")
        h = (h * 0xBF58476D1CE4E5B9) & M64
        h ^= h >> 29
    h ^= h >> 30
    h = (h * 0xBF58476D1CE4E5B9) & M64
    h ^= h >> 27
    h = (h * 0x94D049BB133111EB) & M64
    return h ^ (h >> 31)


def home(key, S):
    return mix(key) & (S - 1)


def table(keys, slack_log=SLACK_DEFAULT, max_probes=PROBES_DEFAULT):
    """the sequential table: (rep, slot_of, U) as dedup_host gives them"""
    n = len(keys)
    S = slots(n, slack_log)
    owner, first = {}, {}
    raw = [bytes(k) for k in keys]
    slot_of = np.full(n, NONE, dtype=np.uint32)
    for i in range(n):
        s = home(raw[i], S)
        for _ in range(max_probes):
            o = owner.setdefault(s, i)
            if o == i or raw[o] == raw[i]:
                first[s] = min(first.get(s, i), i)
                slot_of[i] = s
                break
            s = (s + 1) & (S - 1)
    rep = np.array([i if slot_of[i] == NONE else first[int(slot_of[i])] for i in range(n)], dtype=np.uint32)
    return rep, slot_of, int((rep == np.arange(n)).sum())


def first_occurrence(keys):
    """np.unique's first-occurrence index of every row, and the distinct count"""
    keys = np.ascontiguousarray(keys)
    _, idx, inv = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    return idx[np.asarray(inv).reshape(-1)].astype(np.uint32), len(idx)


def longest_run(keys, slack_log=SLACK_DEFAULT):
    """the longest cyclic run of occupied slots after every distinct key found a slot without a cap (order-independent).  A probe sequence
    visits at most longest_run + 1 slots, so no key reaches a cap above it, whatever the insertion order."""
    S = slots(len(keys), slack_log)
    occ = set()
    for raw in {bytes(k) for k in keys}:
        s = home(raw, S)
        while s in occ:
            s = (s + 1) & (S - 1)
        occ.add(s)
    if len(occ) == S:
        return S
    best = 0
    for s in occ:
        if ((s - 1) & (S - 1)) not in occ:
            run, t = 0, s
            while t in occ:
                run, t = run + 1, (t + 1) & (S - 1)
            best = max(best, run)
    return best


def exact(keys, slack_log=SLACK_DEFAULT, max_probes=PROBES_DEFAULT):
    """whether rep must be the smallest equal index on this set in every insertion order"""
    return longest_run(keys, slack_log) < max_probes


def contract(keys, rep, decoded=None):
    """the three properties that hold for every input and race order; decoded (U) within [distinct, n]"""
    keys = np.ascontiguousarray(keys)
    rep = np.asarray(rep, dtype=np.int64)
    n = len(keys)
    assert (rep <= np.arange(n)).all(), "rep[i] <= i"
    assert np.array_equal(keys[rep], keys), "key rep[i] has the bytes of key i"
    assert np.array_equal(rep[rep], rep), "rep[rep[i]] == rep[i]"
    if decoded is not None:
        assert first_occurrence(keys)[1] <= decoded <= n and decoded == int((rep == np.arange(n)).sum())


# ---- key sets
def random_keys(k, kb=96, seed=1):
    """k distinct random strings"""
    out = np.random.default_rng(seed).integers(0, 256, size=(k, kb), dtype=np.uint8)
    assert len(np.unique(out, axis=0)) == k
    return out


PATTERNS = ("all equal", "all distinct", "pool of 3", "twice in a row", "halves")


def pattern_ids(pattern, n):
    """which pool key stands at each of n positions"""
    i = np.arange(n)
    return {"all equal": i * 0, "all distinct": i, "pool of 3": i % 3, "twice in a row": i // 2, "halves": i % ((n + 1) // 2)}[pattern]


def patterned(pool, pattern, n):
    ids = pattern_ids(pattern, n)
    return np.ascontiguousarray(np.asarray(pool)[ids % len(pool)])


_M1, _M2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
_I1, _I2 = pow(_M1, -1, 1 << 64), pow(_M2, -1, 1 << 64)


def _unshift(h, k):
    """x with x ^ (x >> k) == h (uint64 arrays)"""
    x = h.copy()
    for _ in range(64 // k + 1):
        x = h ^ (x >> np.uint64(k))
    return x


def mix_np(keys):
    """mix() of every row of an (n, kb) uint8 array, as uint64"""
    w = np.ascontiguousarray(keys).view("<u8")
    with np.errstate(over="ignore"):
        h = np.full(len(w), (0x9E3779B97F4A7C15 * (w.shape[1] + 1)) & M64, dtype=np.uint64)
        for j in range(w.shape[1]):
            h = (h ^ w[:, j]) * np.uint64(_M1)
            h ^= h >> np.uint64(29)
        h ^= h >> np.uint64(30)
        h *= np.uint64(_M1)
        h ^= h >> np.uint64(27)
        h *= np.uint64(_M2)
        return h ^ (h >> np.uint64(31))


def same_home(k, S, kb=96, seed=7, slot=None):
    """k distinct keys whose home slot in a table of S slots is the same.  Every step of the mix is a bijection of the state, so the last
    word of a key can be solved for any wanted hash: random leading words, random high hash bits, the low bits the slot."""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 256, size=(k, kb), dtype=np.uint8)
    w = keys.view("<u8")
    slot = int(rng.integers(0, S)) if slot is None else slot
    want = (rng.integers(0, 1 << 63, size=k, dtype=np.uint64) & ~np.uint64(S - 1)) | np.uint64(slot)
    with np.errstate(over="ignore"):
        h = _unshift(want, 31) * np.uint64(_I2)          # back through the finaliser ...
        h = _unshift(h, 27) * np.uint64(_I1)
        h = _unshift(h, 30)
        h = _unshift(h, 29) * np.uint64(_I1)             # ... and the last word's step: h = state before it ^ the word
        keys[:, kb - 8:] = 0
        pre = np.full(k, (0x9E3779B97F4A7C15 * (kb // 8 + 1)) & M64, dtype=np.uint64)
        for j in range(kb // 8 - 1):
            pre = (pre ^ w[:, j]) * np.uint64(_M1)
            pre ^= pre >> np.uint64(29)
        w[:, kb // 8 - 1] = h ^ pre
    assert len(np.unique(keys, axis=0)) == k and ((mix_np(keys) & np.uint64(S - 1)) == np.uint64(slot)).all()
    return np.ascontiguousarray(keys)


def near_pairs(kb=96, seed=3):
    """pairs of keys that differ in one byte only: byte 0, the last byte (the flag byte), and the bytes on either side of a word border"""
    base = random_keys(1, kb, seed)[0]
    out = [base]
    for pos in (0, kb - 1, kb // 2 - 1, kb // 2):
        k = base.copy()
        k[pos] ^= 0x80
        out.append(k)
    return np.ascontiguousarray(np.stack(out))
