"""CPU (-m "not gpu"): the case list of tests/seal_cases.py is what it claims.  For every case class, with shared and per-seal sets, the
status the case list demands is the one the contract's steps give when each is done by an independent implementation: counts and thresholds
in Python, the signature through the oracle's decoder, the hash by oracle/py/hashing.py, the sum of the selected keys by oracle/py/ecc.py and
the product by cpu_oracle.pairing_product_377.  And every message the GPU tests use hashes with a counter below 255."""
import numpy as np
import pytest
from oracle.py import ecc
from oracle.py import hashing as hs
from oracle import cpu_oracle as co
import seal_cases as sc

DOMAIN = b"ULforxof"


def _truth(b, pks, sigs):
    out = []
    neg_g2 = ecc.E2_377.neg(ecc.G2_377)
    for i in range(b.m):
        own = list(range(b.n)) if b.sets is None else b.sets[i]
        count = sum(1 for x in b.bitmap[i] if x)
        if count == 0 or count < b.min_signers[i]:
            out.append(1)
            continue
        sxy, st = co.decompress("g1", sigs[i].tobytes())
        if st[0] >= 2:
            out.append(2)
            continue
        H, c = hs.hash_to_g1_direct(DOMAIN, b.msg[i], sc.EXTRA)
        if c == 255:
            out.append(3)
            continue
        apk = None
        for j, x in zip(own, b.bitmap[i]):
            if x:
                apk = ecc.E2_377.add(apk, pks[j])
        hxy, hinf = co.pack_g1_377([H])
        g2, i2 = co.pack_g2_377([neg_g2, apk])
        g1 = np.concatenate([sxy, hxy])
        i1 = np.array([1 if st[0] == 1 else 0, hinf[0]], dtype=np.uint8)
        out.append(0 if co.pairing_product_377(g1, i1, g2, i2)[1] else 4)
    return out


@pytest.mark.parametrize("per_seal_sets", [False, True], ids=["shared", "per_seal"])
def test_every_constructed_status_is_the_truth(per_seal_sets):
    b = sc.Batch(2 * len(sc.CLASSES), 9, 4, 31, "cpu", per_seal_sets=per_seal_sets)
    assert sorted(set(lab.split(": ")[1] for lab in b.label)) == sorted(sc.CLASSES)
    pks = [ecc.E2_377.mul(ecc.G2_377, k) for k in b.sks]
    signed = []
    for k, msg in zip(b.sign_key, b.sign_msg):
        H, c = hs.hash_to_g1_direct(DOMAIN, msg, sc.EXTRA)
        assert c < 255
        signed.append(np.frombuffer(ecc.ser_point(ecc.E1_377, ecc.E1_377.mul(H, k)), dtype=np.uint8))
    sigs = b.signatures(np.stack(signed))
    got = _truth(b, pks, sigs)
    assert got == b.status, [(lab, g, w) for lab, g, w in zip(b.label, got, b.status) if g != w]


def test_replacement_signatures_are_what_they_claim():
    _, st = co.decompress("g1", sc.undecodable_signature() + sc.point_outside_g1())
    assert st.tolist() == [2, 3]
    _, st = co.decompress("g1", sc.point_outside_g1(), check_subgroup=False)
    assert st.tolist() == [0]


def test_chosen_messages_hash_below_255():
    """the direct hasher on every message of the 65- and 257-seal batches of the GPU tests (their tags), the composite hashers on the messages
    of their 9-seal batches"""
    for tag in ("gpu", "gpu'", "sizes", "sizes'"):
        for i in range(258 if tag.startswith("sizes") else 66):
            assert hs.hash_to_g1_direct(DOMAIN, sc.message(i, tag), sc.EXTRA)[1] < 255
    for cip22 in (False, True):
        for tag in ("modes", "modes'"):
            for i in range(10):
                assert hs.hash_to_g1(DOMAIN, sc.message(i, tag), sc.EXTRA, composite=True, cip22=cip22)[1] < 255
