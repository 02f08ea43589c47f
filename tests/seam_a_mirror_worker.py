"""The body of tests/test_seam_a.py::test_batch_verify_strict_mirror_growth_keeps_rows, run as a process of its own: the handle arenas
and the device mirrors of batch_verify_strict live as long as the process, so only a fresh one starts with both empty - which is what
makes the slot numbers below known (the first handle is slot 0, the 66 000th later one lies beyond the mirrors' first capacity of
65 536 slots).  Exits 0 when every step holds; a failed assert ends it with a traceback and a non-zero status."""
import ctypes as C
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(_HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(_HERE))

from celo_bls_snark_rs_amd import ffi   # noqa: E402

EXTRA = 66000        # more than the mirrors' first capacity, 65 536 slots
CHUNK, FIRST_ROWS = 1 << 14, 1 << 16


class Buffer(C.Structure):
    _fields_ = [("ptr", C.c_char_p), ("len", C.c_size_t)]


class BatchMessageFFI(C.Structure):
    _fields_ = [("data", Buffer), ("extra", Buffer), ("public_keys", C.POINTER(C.c_void_p)), ("public_keys_len", C.c_size_t),
                ("signatures", C.POINTER(C.c_void_p)), ("signatures_len", C.c_size_t)]


def main():
    lib = C.CDLL(ffi.LIB_PATH)
    for f in ("init", "generate_private_key", "private_key_to_public_key", "sign_message", "batch_verify_strict", "serialize_public_key",
              "deserialize_public_key_cached", "aggregate_signatures", "destroy_public_key", "destroy_signature", "destroy_private_key", "free_vec"):
        getattr(lib, f).restype = C.c_bool
    assert lib.init()
    CF = C.c_bool(False)
    msgs = [b"growth-0", b"growth-1"]

    def sign(sk, msg):
        s = C.c_void_p()
        assert lib.sign_message(sk, msg, C.c_int(len(msg)), b"", C.c_int(0), CF, CF, C.byref(s))
        return s

    def key_bytes(pk):
        out, n = C.c_void_p(), C.c_int()
        assert lib.serialize_public_key(pk, C.byref(out), C.byref(n)) and n.value == 96
        data = bytes(C.cast(out, C.POINTER(C.c_ubyte * 96)).contents)
        assert lib.free_vec(out, n)
        return data

    def cached_key(data):
        h = C.c_void_p()
        assert lib.deserialize_public_key_cached(data, C.c_int(96), C.byref(h))
        return h

    def clone_sig(s):
        o = C.c_void_p()
        assert lib.aggregate_signatures((C.c_void_p * 1)(s), C.c_int(1), C.byref(o))
        return o

    def call(pks, sgs):            # pks[b][i], sgs[b][i]: 2 batches x 4 signers
        keep, arr, out = [], (BatchMessageFFI * 2)(), (C.c_bool * 2)()
        for b in range(2):
            p = (C.c_void_p * 4)(*[h.value for h in pks[b]])
            s = (C.c_void_p * 4)(*[h.value for h in sgs[b]])
            keep.append((p, s))
            arr[b] = BatchMessageFFI(Buffer(msgs[b], len(msgs[b])), Buffer(b"", 0), p, 4, s, 4)
        rc = lib.batch_verify_strict(arr, C.c_size_t(2), CF, CF, out)
        return rc, list(out)

    # 1. four key pairs, two messages: both mirrors get their first capacity
    sks, pks = [], []
    for _ in range(4):
        sk, pk = C.c_void_p(), C.c_void_p()
        assert lib.generate_private_key(C.byref(sk)) and lib.private_key_to_public_key(sk, C.byref(pk))
        sks.append(sk)
        pks.append(pk)
    sigs = [[sign(sk, m) for sk in sks] for m in msgs]
    assert call([pks, pks], sigs) == (True, [True, True])
    # 2. 66 000 more handles of either kind, all alive: the arenas' high-water marks pass the mirrors' capacity
    kb = [key_bytes(pk) for pk in pks]
    more_pk = [cached_key(kb[0]) for _ in range(EXTRA)]
    more_sg = [clone_sig(sigs[0][0]) for _ in range(EXTRA)]
    assert len({h.value for h in more_pk}) == EXTRA and len({h.value for h in more_sg}) == EXTRA
    # the slot numbers are the creation order: a fresh process has no free slots, and the arenas fill chunks of 2^14 handles back to back
    # (csrc/seam_handles.hip HandleArena) - the j-th handle lies j % 2^14 handles behind the one that opened its chunk.  So the last
    # handles hold slots 66 003 and 66 007, beyond the 65 536 rows either mirror has after step 1: step 3 cannot pass without a growth.
    for made, size in ((pks + more_pk, 304), (sigs[0] + sigs[1] + more_sg, 160)):     # sizeof(PublicKey), sizeof(Signature)
        assert all(made[j].value - made[j - j % CHUNK].value == (j % CHUNK) * size for j in range(len(made)))
        assert len(made) - 1 >= FIRST_ROWS
    hi_pk, hi_sg = more_pk[-1], more_sg[-1]
    # 3. one signer through handles beyond the first capacity: the mirrors grow; the old handles' tags are unchanged, nothing uploads
    # their rows again - they verify only if the growth carried them over
    grown_pk = [[hi_pk] + pks[1:], pks]
    grown_sg = [[hi_sg] + sigs[0][1:], sigs[1]]
    assert call(grown_pk, grown_sg) == (True, [True, True])
    # 4. ... and the verdicts are verdicts: batch 1's signer 2 with its signature of the other message
    assert call(grown_pk, [grown_sg[0], sigs[1][:2] + [sigs[0][2]] + sigs[1][3:]]) == (False, [True, False])
    # 5. the high key slot changes tenant (LIFO free list: same address, new serial, key 1's point): its row is replaced
    addr = hi_pk.value
    assert lib.destroy_public_key(hi_pk)
    more_pk[-1] = hi_pk = cached_key(kb[1])
    assert hi_pk.value == addr, "the arena reuses the released slot (this test relies on it)"
    assert call([[hi_pk] + pks[1:], pks], grown_sg) == (False, [False, True])
    # 6. everything goes
    for h in more_pk + pks:
        assert lib.destroy_public_key(h)
    for h in more_sg + sigs[0] + sigs[1]:
        assert lib.destroy_signature(h)
    for sk in sks:
        assert lib.destroy_private_key(sk)
    print("mirror growth ok")


if __name__ == "__main__":
    main()
