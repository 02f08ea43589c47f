"""GPU: batched fixed-base scalar multiplication fixed_base_mul_* / _dev (csrc/unit_setup.hip) for the four groups, and normalize_bw6_761_*.

Every call is checked twice: sampled rows (the edge scalars among them) exactly against oracle/py/ecc, and EVERY row at once by a random
linear combination, sum_i r_i out_i = (sum_i r_i k_i) G, the left side by the oracle's MSM."""
import random
import numpy as np
import pytest
import torch  # before the library: both must share one HIP runtime
from oracle import cpu_oracle as co
import groth16_setup_ref as gs

pytestmark = pytest.mark.gpu
JAC_KIND = {"bls12_377_g1": "g1_377", "bls12_377_g2": "g2_377", "bw6_761_g1": "761", "bw6_761_g2": "761"}


def _case(group, n, seed):
    _, curve, g, sw, aw = gs.GROUPS[group]
    r, E1, E2, _, _, _ = gs.CURVES[curve]
    E = E1 if g == 1 else E2
    G = gs.generators(curve)[g - 1]
    if seed & 1:
        G = E.mul(G, 0xC0FFEE + seed)                                   # a non-standard generator of the same subgroup
    rng = random.Random(seed)
    sc = gs.edge_scalars(r, r.bit_length(), 10, rng)[:n]
    sc += [rng.randrange(r) for _ in range(n - len(sc))]
    return curve, g, E, G, r, sc


def _check(group, out, inf, E, G, r, sc, curve, g, seed):
    n = len(sc)
    assert inf.tolist() == [1 if k == 0 else 0 for k in sc]
    assert not out[inf == 1].any()
    rng = random.Random(seed + 1)
    idx = sorted(set(list(range(min(n, 40))) + [rng.randrange(n) for _ in range(24)]))
    rows, _ = gs.pack(curve, g, [E.mul(G, sc[i]) for i in idx])
    assert np.array_equal(out[idx], rows)
    w = [rng.getrandbits(64) for _ in range(n)]
    lhs = co.jac_to_affine(co.msm(group, np.ascontiguousarray(out), inf, co.ints_to_limbs(w, gs.GROUPS[group][3]), threads=8), JAC_KIND[group])
    assert lhs == E.mul(G, sum(a * b for a, b in zip(w, sc)) % r)


@pytest.mark.wall_clock(1200)
@pytest.mark.parametrize("n", [1, 7, 1000, 1 << 16])
@pytest.mark.parametrize("group", sorted(gs.GROUPS))
def test_fixed_base_mul_matches_oracle(gpu, group, n):
    seed = n + len(group)
    curve, g, E, G, r, sc = _case(group, n, seed)
    gen = gs.pack(curve, g, [G])[0][0]
    out, inf = gpu.fixed_base_mul(group, gen, co.ints_to_limbs(sc, gs.GROUPS[group][3]))
    _check(group, out, inf, E, G, r, sc, curve, g, seed)


@pytest.mark.parametrize("group", sorted(gs.GROUPS))
def test_fixed_base_mul_dev_matches_host_entry_and_rejects(gpu, group):
    _, curve, g, sw, aw = gs.GROUPS[group]
    n = 1000
    curve, g, E, G, r, sc = _case(group, n, 77)
    gen = gs.pack(curve, g, [G])[0][0]
    limbs = co.ints_to_limbs(sc, sw)
    want, winf = gpu.fixed_base_mul(group, gen, limbs)
    d_sc = torch.from_numpy(limbs.view(np.int64).copy()).cuda()
    d_out = torch.zeros(n * aw, dtype=torch.int64, device="cuda")
    d_inf = torch.zeros(n, dtype=torch.uint8, device="cuda")
    assert gpu.fixed_base_mul_dev(group, gen, d_sc.data_ptr(), n, d_out.data_ptr(), d_inf.data_ptr()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64).reshape(n, aw), want) and np.array_equal(d_inf.cpu().numpy(), winf)
    # a scalar >= r: code 2, nothing written (host and device entries)
    bad = limbs.copy()
    bad[500] = co.ints_to_limbs([r], sw)[0]
    with pytest.raises(ValueError):
        gpu.fixed_base_mul(group, gen, bad)
    d_bad = torch.from_numpy(bad.view(np.int64).copy()).cuda()
    d_out2 = torch.full((n * aw,), 7, dtype=torch.int64, device="cuda")
    assert gpu.fixed_base_mul_dev(group, gen, d_bad.data_ptr(), n, d_out2.data_ptr(), d_inf.data_ptr()) == 2
    torch.cuda.synchronize()
    assert (d_out2.cpu().numpy() == 7).all()
    # the identity as generator: code 2
    with pytest.raises(ValueError):
        gpu.fixed_base_mul(group, np.zeros(aw, dtype=np.uint64), limbs[:4])


@pytest.mark.parametrize("group", ["bw6_761_g1", "bw6_761_g2"])
def test_normalize_bw6_761(gpu, group):
    """Jacobian (X, Y, Z) = (x Z^2, y Z^3, Z) for random Z, identities (Z = 0) among them, back to (x, y)"""
    _, curve, g, _, _ = gs.GROUPS[group]
    r, E1, E2, q, _, _ = gs.CURVES[curve]
    E = E1 if g == 1 else E2
    G = gs.generators(curve)[g - 1]
    rng = random.Random(5 + g)
    pts = [None if i % 37 == 5 else E.mul(G, rng.randrange(1, r)) for i in range(300)]
    flat = []
    for P in pts:
        if P is None:
            flat += [1, 1, 0]
        else:
            Z = rng.randrange(1, q)
            flat += [P[0] * Z * Z % q, P[1] * Z * Z * Z % q, Z]
    jac = co.to_mont(flat, q).reshape(len(pts), 36)
    xy, inf = gpu.normalize(group, jac)
    want, winf = co.pack_761(pts)
    assert np.array_equal(xy, want) and np.array_equal(inf, winf)


def _dev_mul(gpu, group, gen, limbs):
    n, aw = limbs.shape[0], gs.GROUPS[group][4]
    d_sc = torch.from_numpy(limbs.view(np.int64).copy()).cuda()
    d_out = torch.full((n * aw,), 7, dtype=torch.int64, device="cuda")
    d_inf = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = gpu.fixed_base_mul_dev(group, gen, d_sc.data_ptr(), n, d_out.data_ptr(), d_inf.data_ptr())
    torch.cuda.synchronize()
    return rc, d_out.cpu().numpy().view(np.uint64).reshape(n, aw), d_inf.cpu().numpy()


@pytest.mark.parametrize("group", sorted(gs.GROUPS))
def test_host_and_device_forms_and_the_device_range_check(gpu, group):
    """n = 1 and 65: the two forms return the same bytes.  n = 257 (the range check runs 256 lanes per block: row 256 sits alone in the
    second): all r - 1 passes; r in row 256 and all-ones in row 0 are refused with nothing written; the next call is a normal one."""
    _, curve, g, sw, aw = gs.GROUPS[group]
    curve, g, E, G, r, sc = _case(group, 65, 91)
    gen = gs.pack(curve, g, [G])[0][0]
    limbs = co.ints_to_limbs(sc, sw)
    for n in (1, 65):
        want, winf = gpu.fixed_base_mul(group, gen, limbs[:n])
        rc, out, inf = _dev_mul(gpu, group, gen, limbs[:n])
        assert rc == 0 and np.array_equal(out, want) and np.array_equal(inf, winf)
    top = np.repeat(co.ints_to_limbs([r - 1], sw), 257, axis=0)
    want, winf = gpu.fixed_base_mul(group, gen, top)
    assert np.array_equal(want[0], gs.pack(curve, g, [E.neg(G)])[0][0]) and not winf.any()
    rc, out, inf = _dev_mul(gpu, group, gen, top)
    assert rc == 0 and np.array_equal(out, want) and np.array_equal(inf, winf)
    last, first = top.copy(), top.copy()
    last[256] = co.ints_to_limbs([r], sw)[0]
    first[0] = 0xFFFFFFFFFFFFFFFF
    for bad in (last, first):
        rc, out, inf = _dev_mul(gpu, group, gen, bad)
        assert rc == 2 and (out.view(np.int64) == 7).all() and (inf == 9).all()
    rc, out, inf = _dev_mul(gpu, group, gen, top)
    assert rc == 0 and np.array_equal(out, want)
