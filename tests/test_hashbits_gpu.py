"""GPU (-m gpu): the HashToBits circuit on the device (csrc/unit_hashbits.hip) - assignment, public inputs and the helper proof in one call -
against the host twin (which tests/test_hashbits_host.py holds to the Python restatement), the restatement itself (tests/hashbits_ref.py) and
the library's own setup, prover, proof writer and batch verifier.  Whole outputs, compared exactly.
NOT covered: more than one device; the reference's variable order and ceremony keys (the layout is this library's, csrc/hashbits.h)."""
import functools
import random
import threading
import numpy as np
import pytest
import torch  # before the library: both must share one HIP runtime
from oracle.py import ecc
from oracle.py import composite
from oracle.py import groth16_prover as gp
from oracle import cpu_oracle as co
import groth16_setup_ref as gs
import hashbits_ref as hr
import r1cs_cases as rc
import transition_cases as tc

pytestmark = pytest.mark.gpu
CURVE = "bls12_377"
P = hr.R377
KEY8 = np.array([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0, 0x082EFA98, 0xEC4E6C89], dtype=np.uint32)


def rows_for(m, seed):
    rng = random.Random(7000 * m + seed)
    return np.frombuffer(bytes(rng.randrange(256) for _ in range(48 * m)), dtype=np.uint8).reshape(m, 48).copy()


@functools.lru_cache(maxsize=None)
def host_twin(gpu, m, seed, order):
    z = gpu.hash_to_bits_assignment(rows_for(m, seed), order, host=True)
    z.setflags(write=False)
    return z


def canonical(z_rows):
    return co.ints_to_limbs(hr.from_mont(z_rows), 4)


def affine(a, b, c):
    return [co.jac_to_affine(o, k) for o, k in zip((a, b, c), ("g1_377", "g2_377", "g1_377"))]


def domain_consts(log_n):
    k = gp.domain_constants(log_n, gs.root_of_unity(CURVE, log_n), gs.coset_generator(P), P)
    return {name: co.to_mont([v], P)[0] for name, v in k.items()}


class Circuit:
    """the loaded circuit of m epochs with the parameters of a fixed setup (the toxic values of the existing BLS12-377 end-to-end test)"""
    def __init__(self, gpu, m, want_key=True):
        self.m, self.sizes = m, gpu.hash_to_bits_size(m)[1]
        self.log_n = self.sizes["log_n"]
        self.r = gpu.hash_to_bits_r1cs_load(m)
        rng = random.Random(11)
        tau, toxic = rng.randrange(2, P), [rng.randrange(1, P) for _ in range(4)]
        out = gpu.groth16_setup_r1cs(self.r, self.log_n, rc.mont([gs.root_of_unity(CURVE, self.log_n)], P)[0], rc.mont([tau], P)[0], rc.mont(toxic, P),
                                     gs.pack(CURVE, 1, [ecc.G1_377])[0][0], gs.pack(CURVE, 2, [ecc.G2_377])[0][0], want_rows=False, want_key=want_key)
        self.key, self.vk_rows = out.get("key"), out["vk"]
        self.consts = domain_consts(self.log_n)

    def release(self):
        if self.key is not None:
            self.key.release()
        self.r.release()


@pytest.fixture(scope="module")
def circuits(gpu):
    made = {}

    def get(m):
        if m not in made:
            made[m] = Circuit(gpu, m)
        return made[m]
    yield get
    for c in made.values():
        c.release()


# ---- assignment
# 20 / 21 / 22 and 63 / 64: one either side of the chunk borders of the message pack (384 * 21 = 32 * 252) and the XOF pack (512 * 63 = 128 * 252);
# 2 m lanes of the trace kernel: 40 .. 44 below a wave, 126 / 128 across its 64-lane workgroups; every m * stride crosses the 256-lane blocks of
# the expand kernel (the grid is one-dimensional and not clamped)
@pytest.mark.parametrize("m", [1, 2, 3, 20, 21, 22, 63, 64])
def test_assignment_equals_the_host_twin_row_for_row(gpu, m):
    sizes = gpu.hash_to_bits_size(m)[1]
    for order in (0, 1):
        want = host_twin(gpu, m, 1, order)
        assert want.shape == (sizes["n_vars"], 4)
        assert np.array_equal(gpu.hash_to_bits_assignment(rows_for(m, 1), order), want), order
    # the device-pointer form on a caller's stream, into a buffer with a guard row either side
    d_rows = torch.from_numpy(rows_for(m, 1)).cuda()
    d_z = torch.full(((sizes["n_vars"] + 2) * 4,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        gpu.hash_to_bits_assignment_dev(d_rows.data_ptr(), m, 1, d_z.data_ptr() + 32, s.cuda_stream)
    got = d_z.cpu().numpy().view(np.uint64).reshape(-1, 4)
    assert np.array_equal(got[1:-1], host_twin(gpu, m, 1, 1))
    assert (got[0] == 0x5A5A5A5A5A5A5A5A).all() and (got[-1] == 0x5A5A5A5A5A5A5A5A).all()


@pytest.mark.parametrize("m", [1, 3])
def test_the_loaded_circuit_accepts_the_assignment_and_names_a_row_of_a_perturbed_one(gpu, circuits, m):
    c = circuits(m)
    info = c.r.info()
    assert [info[k] for k in ("curve", "n_constraints", "n_vars", "n_inputs", "nnz_a", "nnz_b", "nnz_c")] == \
        [1] + [c.sizes[k] for k in ("n_constraints", "n_vars", "n_inputs", "nnz_a", "nnz_b", "nnz_c")]
    z = gpu.hash_to_bits_assignment(rows_for(m, 2), 0)
    assert c.r.check(z) == -1
    n_in, stride = c.sizes["n_inputs"], c.sizes["stride"]
    one = co.to_mont([1], P)[0]
    # first / last variable of the first / last epoch, a message bit in the middle, an instance variable
    for v in {n_in, n_in + stride - 1, n_in + (m - 1) * stride, n_in + m * stride - 1, n_in + (m - 1) * stride + 200, 1, n_in - 1}:
        bad = z.copy()
        bad[v] = 0 if bad[v].any() else one
        assert c.r.check(bad) >= 0, v


# ---- public inputs
@pytest.mark.parametrize("m", [1, 3, 21])
@pytest.mark.parametrize("n_proofs", [1, 2, 65])
def test_public_inputs_equal_the_statement_and_the_assignments_instance_rows(gpu, n_proofs, m):
    rows = rows_for(n_proofs * m, 3)
    order = (n_proofs + m) % 2
    got = gpu.hash_to_bits_public_inputs(rows, n_proofs, m, order)
    n_in = hr.n_inputs(m)
    assert got.shape == (n_proofs, n_in - 1, 4)
    want = [hr.instance(rows[p * m:(p + 1) * m], order)[1:] for p in range(n_proofs)]
    assert np.array_equal(got, co.ints_to_limbs([v for w in want for v in w], 4).reshape(got.shape))
    for p in sorted({0, n_proofs // 2, n_proofs - 1}):
        z = gpu.hash_to_bits_assignment(rows[p * m:(p + 1) * m], order)
        assert np.array_equal(canonical(z[1:n_in]), got[p])
    # the device-pointer form
    d_rows = torch.from_numpy(rows).cuda()
    d_out = torch.zeros(got.size, dtype=torch.int64, device="cuda")
    gpu.hash_to_bits_public_inputs_dev(d_rows.data_ptr(), n_proofs, m, order, d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64).reshape(got.shape), got)


def test_one_message_byte_changes_only_its_epoch_and_the_inputs_its_bits_fall_into(gpu):
    m, e = 3, 1
    sizes = gpu.hash_to_bits_size(m)[1]
    n_in, stride, mc = sizes["n_inputs"], sizes["stride"], -(-384 * m // 252)
    rows = rows_for(m, 4)
    z0 = gpu.hash_to_bits_assignment(rows, 0)
    rows[e, 17] ^= 0x24
    z1 = gpu.hash_to_bits_assignment(rows, 0)
    changed = np.nonzero((z0 != z1).any(axis=1))[0]
    witness = changed[changed >= n_in]
    assert witness.size and witness.min() >= n_in + e * stride and witness.max() < n_in + (e + 1) * stride
    bits = [8 * 17 + 2, 8 * 17 + 5]                                   # the two flipped message bits of epoch e
    msg_inputs = {1 + (384 * e + j) // 252 for j in bits}
    xof_inputs = {1 + mc + g // 252 for g in range(512 * e, 512 * (e + 1))}
    inputs = set(int(v) for v in changed[changed < n_in])
    assert inputs & set(range(1, 1 + mc)) == msg_inputs
    assert inputs - msg_inputs and inputs - msg_inputs <= xof_inputs


# ---- end to end: hash_to_bits_r1cs_load -> setup -> the helper proof in one call -> the proof's bytes -> the batch verifier
@pytest.mark.parametrize("m", [1, 3, 17])
def test_end_to_end_from_rows_to_an_accepted_helper_proof(gpu, circuits, m):
    c = circuits(m)
    v = c.vk_rows
    vk = gpu.VerifyingKey(v["alpha_g1"], v["beta_g2"], v["gamma_g2"], v["delta_g2"], v["gamma_abc_g1"], curve=CURVE)
    try:
        assert vk.n_inputs == c.sizes["n_inputs"] - 1
        rows, other = rows_for(m, 5), rows_for(m, 6)
        a, b, cc, inputs = gpu.hash_helper_prove(c.key, c.r, rows, 1, c.log_n, c.consts)
        last = gpu.hash_helper_last()
        assert last["wall"] > 0 and last["prove"] > 0 and last["expand"] > 0 and last["trace"] > 0 and last["pack"] > 0
        assert np.array_equal(inputs, co.ints_to_limbs(hr.instance(rows, 1)[1:], 4))
        # the same proof from the existing entry fed the host twin's z, and from the device-pointer entry: the same three points, so the same
        # 192 bytes of Proof::serialize bit for bit.  (The Jacobian triples the prover returns are NOT compared: the MSMs' summation order is not
        # fixed, and two calls of one entry on one z return different representatives of the same points.)
        ser = gpu.groth16_serialize_proof(a, b, cc, curve=CURVE)
        points = affine(a, b, cc)
        z = gpu.hash_to_bits_assignment(rows, 1, host=True)
        with_key = c.key.prove_r1cs(c.r, z, c.log_n, c.consts)
        assert affine(*with_key) == points and gpu.groth16_serialize_proof(*with_key, curve=CURVE) == ser
        d_z = torch.from_numpy(z.view(np.int64)).cuda()
        torch.cuda.synchronize()
        with_key_dev = c.key.prove_r1cs_dev(c.r, d_z.data_ptr(), c.log_n, c.consts)
        assert affine(*with_key_dev) == points and gpu.groth16_serialize_proof(*with_key_dev, curve=CURVE) == ser
        assert np.array_equal(d_z.cpu().numpy().view(np.uint64), z)                     # the caller's z is read, not written
        oa, ob, oc, other_inputs = gpu.hash_helper_prove(c.key, c.r, other, 1, c.log_n, c.consts)
        ser_other = gpu.groth16_serialize_proof(oa, ob, oc, curve=CURVE)
        wrong = inputs.copy()
        wrong[-1, 0] ^= 1
        x = np.stack([inputs, wrong, other_inputs, inputs, other_inputs])
        # (true proof, true inputs), (.., one changed input), (.., the inputs of other messages), (the proof of other messages, true inputs), and that proof with its own
        assert vk.verify_serialized(ser + ser + ser + ser_other + ser_other, x, mode=0, key=KEY8).tolist() == [1, 0, 0, 0, 1]
    finally:
        vk.release()


def test_the_batch_verifier_refuses_the_key_of_18_epochs(gpu):
    """the documented limit: 64 public inputs, 17 epochs have 61 and 18 have 65"""
    c = Circuit(gpu, 18, want_key=False)
    try:
        v = c.vk_rows
        assert np.asarray(v["gamma_abc_g1"]).reshape(-1, 12).shape[0] == 66
        with pytest.raises(gpu.VerifyError) as e:
            gpu.VerifyingKey(v["alpha_g1"], v["beta_g2"], v["gamma_g2"], v["delta_g2"], v["gamma_abc_g1"], curve=CURVE)
        assert e.value.code == gpu.VK_ERR_INPUTS == 36
    finally:
        c.release()


# ---- the chain hand-off: out_crh of verify_epoch_transitions_bls12_377 as it lies, bit_order 1
def test_crh_rows_of_a_checked_chain_give_the_statements_inputs(gpu):
    b = tc.Batch([(3, "valid", 1)], 31, n_keys=5, tag="h")
    pool = [ecc.ser_point(ecc.E2_377, ecc.E2_377.mul(ecc.G2_377, sk)) for sk in tc.secret_keys()]
    blocks = gpu.EpochBlocks(keys=b.key_bytes(pool), key_off=b.key_off(), **b.fields(True))
    enc, extras, _, _ = gpu.epoch_encode_blocks(blocks, "inner")
    sig, att = gpu.sign_batch(co.ints_to_limbs(b.sign_keys(), 4), gpu.SIG_DOMAIN, enc, [b.sign_extra(i, extras[i].tobytes()) for i in range(b.nb)], 3)
    assert (att != 255).all()
    neg_g2 = co.pack_g2_377([ecc.E2_377.neg(ecc.G2_377)])[0][0]
    r = gpu.verify_epoch_transitions(blocks, b.chain_off, b.bits(), b.signatures(sig), gpu.SIG_DOMAIN, neg_g2, mode=1)
    assert r["chain_ok"].tolist() == [1] and b.nb == 4
    crh = np.ascontiguousarray(r["crh"][1:])                                            # the three transitions' rows (the initial block has none)
    want_rows = [composite.composite_crh(bytes(enc[i])) for i in range(1, 4)]
    assert [row.tobytes() for row in crh] == want_rows
    got = gpu.hash_to_bits_public_inputs(crh, 1, 3, 1)[0]
    assert np.array_equal(got, co.ints_to_limbs(hr.instance(want_rows, 1)[1:], 4))


# ---- threads and refusals
def test_two_threads_with_different_sizes(gpu):
    want = {m: host_twin(gpu, m, 1, 0) for m in (2, 21)}
    out = {}

    def work(m):
        gpu.use_device(0)
        out[m] = [gpu.hash_to_bits_assignment(rows_for(m, 1), 0) for _ in range(3)]
    th = [threading.Thread(target=work, args=(m,)) for m in want]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert sorted(out) == [2, 21] and all(np.array_equal(z, want[m]) for m, zs in out.items() for z in zs)


def test_foreign_handles_and_sizes_are_refused(gpu, circuits):
    c1, c3 = circuits(1), circuits(3)
    rows1, rows3 = rows_for(1, 1), rows_for(3, 1)
    assert gpu.hash_helper_prove_rc(c1.key, c3.r, rows3, 0, c3.log_n, c3.consts)[0] == 2      # a key of another circuit size
    assert gpu.hash_helper_prove_rc(c3.key, c1.r, rows1, 0, c1.log_n, c1.consts)[0] == 2
    assert gpu.hash_helper_prove_rc(c1.key, c1.r, rows3, 0, c3.log_n, c3.consts)[0] == 2      # a circuit of another size than the rows
    assert gpu.hash_helper_prove_rc(c1.key, c1.r, rows1, 2, c1.log_n, c1.consts)[0] == 2
    assert gpu.hash_helper_prove_rc(c1.key, c1.r, rows1, 0, c1.log_n - 1, c1.consts)[0] == 2
    case = rc.toy("bw6_761")
    foreign = gpu.R1CS.load(case.curve, case.m, case.n_vars, case.n_inputs, case.csr())
    try:
        assert gpu.hash_helper_prove_rc(c1.key, foreign, rows1, 0, c1.log_n, c1.consts)[0] == 2  # an R1CS handle of the other curve
    finally:
        foreign.release()
    a, b, c, _ = gpu.hash_helper_prove(c1.key, c1.r, rows1, 0, c1.log_n, c1.consts)            # ... and the handles still serve
    assert a.any() and b.any() and c.any()
