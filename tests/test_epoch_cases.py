"""CPU (-m "not gpu"): the case list of tests/epoch_cases.py, proved on the oracle alone (oracle/py/epoch.py) - the reference's golden encodings
reproduce, the size formula of include/celo_bls_amd.h holds for every case and kind, the Blake2s border lengths are what the GPU test claims,
and the inputs derived from the reference vector's blocks make the reference proof's four-pair product one."""
import numpy as np
import pytest
import epoch_cases as EC
from oracle.py import ecc
from oracle.py import epoch as ep
from oracle import cpu_oracle as co


def test_golden_encodings_reproduce_from_the_case_list(golden):
    e = golden["epoch_encoding"]
    gen10 = [ecc.G2_377] * 10
    f, g = bytes([255] * 16), bytes([254] * 16)
    assert ep.EpochBlock(120, 5, f, g, 3, 10, gen10).encode_first_epoch_to_bytes_cip22().hex() == e["EXPECTED_ENCODING_WITH_ENTROPY"]
    assert ep.EpochBlock(120, 5, None, None, 3, 10, gen10).encode_first_epoch_to_bytes_cip22().hex() == e["EXPECTED_ENCODING_WITHOUT_ENTROPY"]
    assert ep.EpochBlock(120, 10, None, None, 3, 10, gen10).encode_to_bytes().hex() == e["EXPECTED_ENCODING_BEFORE_DONUT"]
    assert ep.EpochBlock(120, 5, f, g, 3, 11, gen10).encode_first_epoch_to_bytes_cip22().hex() == e["EXPECTED_ENCODING_WITH_ENTROPY_PADDED"]
    # the same strings as padding only: maximum_validators keys of the generator and no key of the block's own
    assert EC.expected(EC.Case(120, 5, f, g, 3, 10, []), "first")[0].hex() == e["EXPECTED_ENCODING_WITH_ENTROPY"]
    assert EC.expected(EC.Case(120, 5, None, None, 3, 10, []), "first")[0].hex() == e["EXPECTED_ENCODING_WITHOUT_ENTROPY"]
    # an absent entropy and sixteen zero bytes are one encoding
    assert EC.expected(EC.Case(120, 5, bytes(16), bytes(16), 3, 10, []), "first")[0].hex() == e["EXPECTED_ENCODING_WITHOUT_ENTROPY"]


def test_size_formula_holds_for_every_case_and_kind():
    cases = EC.small_cases() + EC.null_entropy_cases() + [c for k in EC.BORDER_K for c in EC.border_cases(k)]
    for c in cases:
        for kind in EC.KINDS:
            data, extra = EC.expected(c, kind)
            assert len(data) == EC.encoded_size(kind, len(c.keys), c.maxv), (c.ident(), kind)
            assert (extra is None) == (kind != "inner") and (extra is None or len(extra) == 7)
    assert len(EC.expected(EC.Case(0, 0, None, None, 0, 0, []), "first")[0]) == 22


def test_border_lengths_are_what_is_claimed():
    for kind, lens in EC.BORDER_LEN.items():
        got = [len(EC.expected(c, kind)[0]) for c in EC.border_cases(kind)]
        assert tuple(got) == lens, kind
        assert [n % 64 for n in got] == [0, 1, 63], kind


def test_case_list_covers_the_alignments_and_the_field_extremes():
    cases = EC.small_cases()
    assert sorted({len(c.keys) for c in cases if EC.IDENTITY not in c.keys and len(set(c.keys)) == len(c.keys)}) == list(range(10))
    assert {(755 * k) % 8 for k in range(10)} == set(range(8))
    rel = {("below" if c.maxv < len(c.keys) else "equal" if c.maxv == len(c.keys) else "above") for c in cases if c.keys}
    assert rel == {"below", "equal", "above"} and any(c.maxv == 0 and c.keys for c in cases)
    for field, top in (("index", EC.U16), ("round", EC.U8), ("mns", EC.U32)):
        assert {0, top} <= {getattr(c, field) for c in cases}, field
    assert any(c.ee is None for c in cases) and any(c.ee == bytes(16) for c in cases) and any(c.ee not in (None, bytes(16)) for c in cases)
    assert any(EC.IDENTITY in c.keys for c in cases)


def test_inputs_of_the_reference_blocks_make_the_reference_product_one(golden):
    """the oracle's route from blocks to inputs, the one the GPU tests compare with: blocks -> bytes -> Blake2s -> 376 | 136 -> the product"""
    g = golden["groth16_bw6_761"]
    vk, pr = ep.parse_vk(bytes.fromhex(g["vk"])), ep.parse_proof(bytes.fromhex(g["proof"]))
    first, last = EC.reference_cases(golden)

    def block(s):
        pks = [ecc.deser_point(ecc.E2_377, s["raw"][96 * i:96 * i + 96]) for i in range(len(s["raw"]) // 96)]
        return ep.EpochBlock(s["index"], s["round"], s["ee"], s["pe"], s["mns"], s["maxv"], pks)
    inputs = ep.pack(ep.hash_first_last_epoch_block(block(first), block(last)))
    assert len(inputs) == 2 and inputs[0] < 1 << 376 and inputs[1] < 1 << 136
    for x, want in ((inputs, True), ([inputs[0], inputs[1] ^ 1], False)):
        pairs = ep.groth16_pairs(vk, pr, x)
        g1, i1 = co.pack_761([p for p, _ in pairs])
        g2, i2 = co.pack_761([q for _, q in pairs])
        assert bool(co.pairing_product_761(g1, i1, g2, i2)[1]) == want


def test_arrays_describe_the_cases():
    cases = EC.small_cases()
    a = EC.arrays(cases, keys_form=0)
    assert a["key_off"][-1] == sum(len(c.keys) for c in cases) == a["keys"].shape[0]
    b = EC.arrays(cases, keys_form=1)
    assert b["keys"].shape == (a["keys"].shape[0], 24) and int(b["keys_inf"].sum()) == sum(c.keys.count(EC.IDENTITY) for c in cases)
    with pytest.raises(AssertionError):
        EC.arrays(cases, null_entropy=True)
    assert EC.arrays(EC.null_entropy_cases(), null_entropy=True)["epoch_entropy"] is None
    assert np.array_equal(EC.inputs_limbs([(cases[1], cases[2])])[0], co.ints_to_limbs(EC.expected_inputs(cases[1], cases[2]), 6))
