"""GPU (-m gpu): the BW6-761 pairing on every dispatch path of PairingEngine<PP761>::run_staged (csrc/pairing.h), whole batches against
the oracle.  Every comparison is bit for bit on arkworks Montgomery limbs: GT values against co.pairing_product_761, Miller values
against co.miller_loop_761; verdicts are read twice, from pairing_gt_bw6 (GT row == the packed one) and from the batched verdict entry
pairing_product_is_one_batch_bw6, and compared with the verdict each product has BY CONSTRUCTION (tests/pairing761_cases.py, whose inputs
tests/test_pairing761_cases.py checks on the CPU without the library).

  latency ("wide") path      m == 1, 1 <= k <= 7                     test_latency_path_*
  per pair + ragged product  1 < m < 16384, any product > 4 pairs    test_single_product_* (k = 8), test_ragged_*, test_chain_*, test_threshold_*
  per pair + product tree    m == 1, k > 8                           test_single_product_* (k = 9 ... 64)
  shared accumulator         m >= 16384, every product <= 4 pairs    test_threshold_*

Left out on purpose: malformed offsets (non-monotone, offsets[0] != 0, offsets[m] beyond the arrays).  The library does not validate
them, a test must not provoke a fault, and validation is a separate change.  Also not here: more than 64 pairs in one product."""
import threading
import numpy as np
import pytest
import torch  # noqa: F401  (before the library: torch brings its own HIP runtime; loaded after the library's, it finds no device)
from oracle.py import ecc
from oracle import cpu_oracle as co
from tests import pairing761_cases as pc

pytestmark = pytest.mark.gpu

SEED_SMALL, SEED_BIG = 0x761A11E, 0x761B16
N_BIG = 90000
GROUPS = 21                      # LP761::GROUPS: lane groups per 64-thread block
SHARED_MIN = 16384               # PairingEngine::SHARED_MIN_PRODUCTS


@pytest.fixture(scope="module")
def small():
    return pc.python_points(160, SEED_SMALL)


@pytest.fixture(scope="module")
def big(gpu):
    return pc.device_points(N_BIG, SEED_BIG)


@pytest.fixture(scope="module")
def one_gt():
    z = np.zeros((0, 24), dtype=np.uint64)
    gt, one = co.pairing_product_761(z, None, z, None)
    assert one
    return gt


def _sub(batch, a, b):
    """products a ... b - 1 of a batch as a batch of their own"""
    g1, i1, g2, i2, offs, expect = batch
    lo, hi = int(offs[a]), int(offs[b])
    return g1[lo:hi], i1[lo:hi], g2[lo:hi], i2[lo:hi], (offs[a:b + 1] - offs[a]).astype(np.uint32), expect[a:b]


def _run(gpu, batch, one_gt, what):
    """GT rows and both verdict vectors of one batch; the verdicts must agree with each other and with construction"""
    g1, i1, g2, i2, offs, expect = batch
    gt = gpu.pairing_gt_bw6(g1, i1, g2, i2, offs)
    by_gt = (gt == one_gt[None, :]).all(axis=1)
    by_entry = gpu.pairing_product_is_one_batch_bw6(g1, i1, g2, i2, offs)
    bad = np.nonzero(by_gt != expect.astype(bool))[0]
    assert bad.size == 0, "%s: GT verdict differs from construction at products %s (block %s, group %s)" % (what, bad[:8], bad[:8] // GROUPS, bad[:8] % GROUPS)
    bad = np.nonzero(by_entry.astype(bool) != expect.astype(bool))[0]
    assert bad.size == 0 and set(np.unique(by_entry)) <= {0, 1}, "%s: is_one differs from construction at products %s" % (what, bad[:8])
    return gt


def _against_oracle(batch, gt, products, what, ml=None):
    for p in products:
        want, one = pc.oracle_gt(batch, int(p))
        assert bool(one) == bool(batch[5][p]), "%s: oracle verdict of product %d differs from construction" % (what, p)
        assert np.array_equal(gt[p], want), "%s: GT value of product %d (block %d, group %d, %d pairs)" % (
            what, p, p // GROUPS, p % GROUPS, int(batch[4][p + 1] - batch[4][p]))
        if ml is not None:
            assert np.array_equal(ml[p], pc.oracle_miller(batch, int(p))), "%s: Miller value of product %d" % (what, p)


def test_device_generated_points_are_the_oracles(big):
    """the large cases rely on rows k_i A, k_i B from the generator kernel: a sample of them, bit for bit, against the Python oracle's"""
    idx = sorted({0, 1, 20, 21, 22, 4095, 16383, 16384, 65535, N_BIG - 1} | set(np.random.default_rng(1).integers(0, N_BIG, size=22).tolist()))
    g1, g2 = pc.python_rows(SEED_BIG, idx)
    assert np.array_equal(big.P[idx], g1) and np.array_equal(big.Q[idx], g2)


# ------------------------------------------------------------------------------------------------ latency path: m == 1, k = 1 ... 7
def _single(gpu, batch, one_gt, what):
    """one product: Miller value, GT value, verdict (both entries and the single-product entry) against the oracle"""
    g1, i1, g2, i2, offs, expect = batch
    ml = gpu.pairing_gt_bw6(g1, i1, g2, i2, offs, miller_only=True)
    gt = _run(gpu, batch, one_gt, what)
    _against_oracle(batch, gt, [0], what, ml)
    assert bool(gpu.pairing_product_is_one_bw6(g1, i1, g2, i2)) == bool(expect[0]), what
    return gt


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7])
def test_latency_path_every_k(gpu, small, one_gt, k):
    """csrc/unit_pairing761_wide.hip: k unrelated pairs; then the infinity flag in every position, once through inf1 and once through inf2;
    all pairs flagged; an accepting product at every even k."""
    live = pc.layout(small, [pc.product(small, k, "unrelated", 7 * k)])
    _single(gpu, live, one_gt, "wide k=%d" % k)
    g1, _, g2, _, offs, _ = live
    for pos in range(k):
        for which in (1, 2):
            i1 = np.zeros(k, dtype=np.uint8); i2 = np.zeros(k, dtype=np.uint8)
            (i1 if which == 1 else i2)[pos] = 1
            a1, a2 = g1.copy(), g2.copy()
            if pos & 1:
                (a1 if which == 1 else a2)[pos] = 0              # what pack_761 writes for a point at infinity; otherwise a stale valid row
            _single(gpu, (a1, i1, a2, i2, offs, np.array([1 if k == 1 else 0], dtype=np.uint8)), one_gt, "wide k=%d inf%d[%d]" % (k, which, pos))
    off = pc.layout(small, [pc.product(small, k, "all_off", 5 * k)])
    gt = _single(gpu, off, one_gt, "wide k=%d all pairs flagged" % k)
    assert np.array_equal(gt[0], one_gt)
    # without flag arrays at all (NULL pointers), after calls that had them
    gt = gpu.pairing_gt_bw6(g1, None, g2, None, offs)
    assert np.array_equal(gt[0], co.pairing_product_761(g1, None, g2, None)[0])
    if k % 2 == 0:
        acc = pc.layout(small, [pc.product(small, k, "accept", 3 * k)])
        assert not acc[1].any() and not acc[3].any() and acc[5][0] == 1
        assert np.array_equal(_single(gpu, acc, one_gt, "wide k=%d accepting" % k)[0], one_gt)
        _single(gpu, pc.layout(small, [pc.product(small, k, "mismatch", 3 * k)]), one_gt, "wide k=%d mismatch" % k)


def test_latency_path_reference_vector(gpu, small, one_gt, golden):
    """k = 4: the reference's own Groth16 product accepts, its tampered forms reject, Miller and GT values as the oracle's"""
    for g1, g2, want, name in pc.reference_products(golden):
        pts, at = small.with_rows(g1, g2)
        _single(gpu, pc.layout(pts, [pc.fixed_product(at, 4, want, name)]), one_gt, "wide " + name)


# ------------------------------------------------------------------------------------------------ one product on the throughput kernels
@pytest.mark.parametrize("k", [8, 9, 20, 21, 22, 42, 43, 64])
def test_single_product_on_the_throughput_kernels(gpu, small, one_gt, k):
    """m == 1, k >= 8: k_miller_lanes<LP761> over one and two blocks of 21 groups and either side of them, then k_gt_product_lanes (k = 8)
    or the product tree k_gt_tree_lanes (k > 8; 9 -> 5 -> 3 -> 2 -> 1 and 43 -> 22 -> 11 -> 6 -> 3 -> 2 -> 1 have levels with an odd
    count), then k_final_exp_lanes."""
    path = "ragged product" if k == 8 else "product tree"
    _single(gpu, pc.layout(small, [pc.product(small, k, "unrelated", k)]), one_gt, "%s k=%d unrelated" % (path, k))
    acc = pc.layout(small, [pc.product(small, k, "accept", k + 1, flag_pos=k - 1)])      # couples; odd k: and a flagged pair, the last
    assert acc[5][0] == 1
    assert np.array_equal(_single(gpu, acc, one_gt, "%s k=%d accepting" % (path, k))[0], one_gt)
    # the infinity flag on the first and on the last pair: half a couple switched off (even k), or the odd pair out (odd k)
    for pos in (0, k - 1):
        s = pc.product(small, k, "half_off" if k % 2 == 0 else "accept", k + 2, flag_pos=pos)
        assert (s.f1[pos] | s.f2[pos]) == 1
        _single(gpu, pc.layout(small, [s]), one_gt, "%s k=%d flag on pair %d" % (path, k, pos))
    # the LAST pair decides: accepting couples and one live unrelated pair at the end (odd k: the element an odd tree level carries
    # unpaired; were it dropped the product would be 1), or a foreign Q in the last pair (even k)
    s = pc.product(small, k, "extra_live" if k % 2 else "mismatch", k + 3, flag_pos=k - 1)
    assert s.expect == 0 and not any(s.f1) and not any(s.f2)
    _single(gpu, pc.layout(small, [s]), one_gt, "%s k=%d, last pair decides (odd carry)" % (path, k))


def test_empty_call_shapes(gpu, small, one_gt):
    """k = 0: one empty product is 1 and its GT value is one; so are several, and m = 0 is accepted"""
    z = np.zeros((0, 24), dtype=np.uint64); f = np.zeros(0, dtype=np.uint8)
    for m in (1, 3):
        b = (z, f, z, f, np.zeros(m + 1, dtype=np.uint32), np.ones(m, dtype=np.uint8))
        gt = _run(gpu, b, one_gt, "k=0, m=%d" % m)
        assert (gt == one_gt[None, :]).all()
        assert (gpu.pairing_gt_bw6(z, None, z, None, b[4], miller_only=True) == one_gt[None, :]).all()
    assert gpu.pairing_product_is_one_bw6(z, None, z, None)
    assert gpu.pairing_product_is_one_batch_bw6(z, None, z, None, np.zeros(1, dtype=np.uint32)).size == 0


# ------------------------------------------------------------------------------------------------ ragged batches on the per-pair path
def _ragged_counts(m, seed):
    """pair counts 0 ... 9; empty products at the start, in the middle and at the end; product 3 covers pairs 18 ... 26 (m >= 21): it
    straddles the boundary between the first two blocks of k_miller_lanes"""
    c = np.random.default_rng(seed).integers(0, pc.MAX_PAIRS + 1, size=m)
    if m >= 21:
        c[:4] = [0, 9, 9, 9]
        c[m // 2] = 0
        c[m - 1] = 0
        c[m - 2] = 9
    return [int(x) for x in c]


@pytest.mark.parametrize("m", [2, 21, 22, 300])
def test_ragged_batches_on_the_per_pair_path(gpu, big, one_gt, m):
    """1 < m < 16384: k_miller_lanes per pair, k_gt_product_lanes per product (offsets ragged, empty products, flags inside the batch),
    k_final_exp_lanes writing is_one for m > 1.  m = 21 / 22: one block of products and one more.  Every verdict against construction,
    EVERY GT value against the oracle, Miller values too for m <= 22."""
    if m == 2:        # nine pairs (four couples and a pair flagged through inf2) accepting, four pairs with half a couple flagged through inf1
        counts = [9, 4]
        batch = pc.layout(big, [pc.product(big, 9, "accept", 2002, which=2), pc.product(big, 4, "half_off", 2020, which=1)])
    else:
        counts = _ragged_counts(m, 100 + m)
        batch = pc.ragged_batch(big, counts, seed=200 + m, first=1000 * (m % 7))
    g1, i1, g2, i2, offs, expect = batch
    if m >= 21:
        assert counts[0] == 0 and counts[m // 2] == 0 and counts[-1] == 0 and offs[3] < GROUPS < offs[4]
    assert i1.any() and i2.any() and 0 < int(expect.sum()) < m
    gt = _run(gpu, batch, one_gt, "ragged m=%d" % m)
    ml = gpu.pairing_gt_bw6(g1, i1, g2, i2, offs, miller_only=True) if m <= 22 else None
    _against_oracle(batch, gt, range(m), "ragged m=%d" % m, ml)


@pytest.mark.parametrize("m,c", [(1, 8), (2, 2), (22, 2), (43, 3)])
def test_last_product_is_written_over_stale_rows(gpu, big, one_gt, m, c):
    """Calls of the SAME shape one after the other, so that the arena rows of the earlier call sit exactly where the later call writes
    (same k, same m: same layout).  First every product accepts, then the same call with a LAST product that does not (a foreign Q, or a
    live odd pair out), then all accepting again: a kernel that leaves the last product of a call unwritten returns the stale row of the
    call before - one where it must not be, not one where it must be - whatever the arena held at the start.  m = 1, k = 8 and m = 2 ... 43
    on the per-pair path (k_miller_lanes, k_gt_product_lanes, k_final_exp_lanes; 22 and 43 end in a block's first group)."""
    first = 50000 + 500 * m
    accept = [pc.product(big, c, "accept", first + 10 * p, which=1 + (p & 1)) for p in range(m)]
    reject = list(accept)
    reject[-1] = pc.product(big, c, "extra_live" if c % 2 else "mismatch", first + 10 * (m - 1))
    assert reject[-1].expect == 0 and all(s.expect == 1 for s in accept) and len(reject[-1]) == len(accept[-1]) == c
    for what, specs in (("all accept", accept), ("last product rejects", reject), ("all accept again", accept)):
        batch = pc.layout(big, specs)
        gt = _run(gpu, batch, one_gt, "m=%d, %s" % (m, what))
        ml = gpu.pairing_gt_bw6(*batch[:5], miller_only=True)
        _against_oracle(batch, gt, sorted({0, m - 1}), "m=%d, %s" % (m, what), ml)


def _sample(m, seed, fixed, budget):
    rnd = np.random.default_rng(seed).choice(m, size=min(64, m), replace=False).tolist()
    pick = list(dict.fromkeys([int(p) for p in list(fixed) + rnd if 0 <= p < m]))
    assert len(pick) <= budget, (len(pick), budget)
    return pick


def test_chain_of_1000_groth16_checks(gpu, big, one_gt, golden):
    """m = 1000 products of four pairs, what a light client walking a chain of epoch proofs asks: the reference vector at every tenth
    place among DISTINCT constructed accepting products, every 97th product tampered (a foreign Q; for a reference slot its two tampered
    forms).  Every verdict is checked; GT against the oracle on 64 seeded products plus the first, the last, groups 20 / 21 / 22, every
    tampered product and a reference slot: about 8 % of the call, the other 92 % are covered by their verdicts (an accepting product's
    GT row IS the packed one, so for the accepting 99 % the verdict from the GT row is a comparison of the whole value)."""
    rp = pc.reference_products(golden)
    pts, at = big.with_rows(np.concatenate([r[0] for r in rp]), np.concatenate([r[1] for r in rp]))      # a copy: the fixture stays as it is
    ref = [pc.fixed_product((at[0] + 4 * t, at[1] + 4 * t), 4, want, name) for t, (_, _, want, name) in enumerate(rp)]
    specs, tampered = [], []
    for p in range(1000):
        bad = p % 97 == 0
        if p % 10 == 5:
            specs.append(ref[1 + (p // 10) % 2] if bad else ref[0])
        else:
            specs.append(pc.product(pts, 4, "mismatch" if bad else "accept", 5 * p))
        if bad:
            tampered.append(p)
    batch = pc.layout(pts, specs)
    assert len(tampered) == 11 and 485 in tampered and specs[485].kind.startswith("reference_bad") and int(batch[5].sum()) == 989
    assert not batch[1].any() and (np.diff(batch[4].astype(np.int64)) == 4).all()
    gt = _run(gpu, batch, one_gt, "chain of 1000")
    pick = _sample(1000, 31, [0, 999, 20, 21, 22, 5, 15] + tampered, 90)
    assert len(pick) >= 64 + 11
    _against_oracle(batch, gt, pick, "chain of 1000")


# ------------------------------------------------------------------------------------------------ the 16384 threshold
M_BIG = SHARED_MIN + 37          # 16384 = 21 * 780 + 4; 16421 = 21 * 781 + 20: another remainder, a last block with one group idle
THRESHOLD_BUDGET = 1000          # products of the threshold call that go to the oracle: 6.1 % of 16421


@pytest.fixture(scope="module")
def threshold_batch(big):
    """16421 distinct products of 0 ... 4 pairs: accepts, rejects, unrelated points, flags through inf1 and inf2.  About 4 % of the
    products carry a flag (flag_share: 8 % of those the draw flags are kept): few enough for ALL of them to go to the oracle."""
    counts = np.random.default_rng(16384).integers(0, 5, size=M_BIG)
    counts[[0, 1, 2, 3, 4]] = [4, 0, 3, 2, 1]
    counts[[SHARED_MIN - 1, SHARED_MIN, M_BIG - 1]] = [4, 3, 4]
    specs = pc.ragged_specs(big, [int(c) for c in counts], seed=16385, flag_share=0.08)
    return specs, pc.layout(big, specs)


@pytest.fixture(scope="module")
def per_pair_rows(gpu, threshold_batch, one_gt):
    """GT rows of all 16421 products from the per-pair path: the first 16383 in one call (the largest below the threshold), the rest in
    a second"""
    _, batch = threshold_batch
    a = _run(gpu, _sub(batch, 0, SHARED_MIN - 1), one_gt, "m=16383 (per-pair path)")
    b = _run(gpu, _sub(batch, SHARED_MIN - 1, M_BIG), one_gt, "m=38 (per-pair path)")
    return np.concatenate([a, b])


def test_threshold_inputs_cover_every_class(threshold_batch):
    specs, batch = threshold_batch
    kinds = {(len(s), s.kind) for s in specs}
    assert {c for c, _ in kinds} == {0, 1, 2, 3, 4} and {k for _, k in kinds} >= set(pc.VARIANTS) | {"empty"}
    flagged = [s for s in specs if pc.has_flag(s)]
    assert 400 < len(flagged) < THRESHOLD_BUDGET - 200 and batch[1].sum() > 150 and batch[3].sum() > 150
    assert {(len(s), s.kind) for s in flagged} >= {(c, k) for c in (1, 2, 3, 4) for k in ("all_off",)} | {(2, "half_off"), (4, "half_off"), (1, "accept"), (3, "accept"), (3, "mismatch")}
    assert 4000 < int(batch[5].sum()) < 12000
    assert max(len(s) for s in specs) == 4


def test_threshold_per_pair_rows_against_oracle(gpu, threshold_batch, per_pair_rows):
    """m = 16383, the per-pair path (746 blocks of pairs and more): anchored to the oracle on the sample below"""
    specs, batch = threshold_batch
    _against_oracle(batch, per_pair_rows, _threshold_sample(specs), "m=16383 + 38 (per-pair path)")


def _threshold_sample(specs):
    """64 seeded products; the first, the last, groups 20 / 21 / 22 of the first block, both sides of 16384, the last block; one product
    per (pair count, class); EVERY product with a flag (613 of them); then products the construction expects to accept (two pairs and more,
    no flag), in order, until the budget of 1000 is full: 6.1 % of the call.  The other 93.9 % - none of them with a flag - are covered by
    their construction verdicts and by the row-for-row comparison of the two independent paths."""
    fixed = [0, M_BIG - 1, 20, 21, 22, SHARED_MIN - 2, SHARED_MIN - 1, SHARED_MIN, M_BIG - 21, M_BIG - 20]
    seen = {}
    for p, s in enumerate(specs):
        seen.setdefault((len(s), s.kind), p)
    fixed += sorted(seen.values())
    fixed += [p for p, s in enumerate(specs) if pc.has_flag(s)]
    base = _sample(M_BIG, 16386, fixed, THRESHOLD_BUDGET)
    have = set(base)
    accepts = [p for p, s in enumerate(specs) if s.expect == 1 and len(s) >= 2 and not pc.has_flag(s) and p not in have]
    pick = base + accepts[:THRESHOLD_BUDGET - len(base)]
    assert len(pick) == THRESHOLD_BUDGET and all(p in set(pick) for p, s in enumerate(specs) if pc.has_flag(s))
    return pick


@pytest.mark.parametrize("m", [SHARED_MIN, M_BIG])
def test_threshold_shared_accumulator_rows_equal_per_pair_rows(gpu, threshold_batch, per_pair_rows, one_gt, m):
    """m >= 16384, every product <= 4 pairs: k_miller_product_lanes<LP761> (miller_multi<4>), one lane group per product.  Every verdict
    against construction; EVERY GT row equal, bit for bit, to the row the per-pair kernels gave for the same product in calls below the
    threshold; the Miller rows as well on the sample; and the sample - every product with a flag is in it - against the oracle."""
    specs, batch = threshold_batch
    sub = _sub(batch, 0, m)
    gt = _run(gpu, sub, one_gt, "m=%d (shared accumulator)" % m)
    diff = np.nonzero((gt != per_pair_rows[:m]).any(axis=1))[0]
    assert diff.size == 0, "shared-accumulator rows differ from per-pair rows at products %s (blocks %s, groups %s; %d in all)" % (
        diff[:8], diff[:8] // GROUPS, diff[:8] % GROUPS, diff.size)
    pick = [p for p in _threshold_sample(specs) if p < m]
    ml = gpu.pairing_gt_bw6(sub[0], sub[1], sub[2], sub[3], sub[4], miller_only=True)
    _against_oracle(sub, gt, pick, "m=%d (shared accumulator)" % m, ml)


def test_threshold_one_product_of_five_pairs_falls_back(gpu, big, threshold_batch, per_pair_rows, one_gt):
    """a batch of 16421 in which ONE product has five pairs leaves the shared-accumulator path: same rows for all the others, the
    five-pair product against the oracle"""
    specs, _ = threshold_batch
    at = 8000
    mixed = list(specs)
    mixed[at] = pc.product(big, 5, "extra_live", 5 * M_BIG + 10)
    batch = pc.layout(big, mixed)
    gt = _run(gpu, batch, one_gt, "m=16421 with a five-pair product")
    keep = np.arange(M_BIG) != at
    assert np.array_equal(gt[keep], per_pair_rows[keep])
    _against_oracle(batch, gt, [at - 1, at, at + 1], "m=16421 with a five-pair product")


# ------------------------------------------------------------------------------------------------ call sequences on the engine arena
def test_call_sequences_reuse_the_arena(gpu, small, big, one_gt):
    """large -> small -> large, throughput -> latency -> throughput, flags then NULL flag pointers (stale flag bytes of the earlier call
    sit in the arena and must not be read), an interleaved BLS12-377 call, and the same call twice: identical bytes every time."""
    large = pc.ragged_batch(big, _ragged_counts(300, 7), seed=8, first=20000)
    tiny = pc.layout(small, [pc.product(small, 3, "unrelated", 40)])
    first = _run(gpu, large, one_gt, "large")
    _against_oracle(large, first, [0, 1, 3, 150, 298, 299], "large")
    _single(gpu, tiny, one_gt, "latency call after a large one")
    assert np.array_equal(_run(gpu, large, one_gt, "large again"), first)
    # flags, then none: every product is half a couple switched off (not 1) whose rows are valid, so without flags every product is 1
    specs = [pc.product(big, 2, "half_off", 30000 + 5 * p) for p in range(30)]
    off = pc.layout(big, specs)
    _run(gpu, off, one_gt, "30 half couples")
    g1, _, g2, _, offs, _ = off
    assert (gpu.pairing_gt_bw6(g1, None, g2, None, offs) == one_gt[None, :]).all(), "stale flag bytes were read"
    assert gpu.pairing_product_is_one_batch_bw6(g1, None, g2, None, offs).all()
    assert not gpu.pairing_product_is_one_batch_bw6(g1, off[1], g2, None, offs)[np.array([any(s.f1) for s in specs])].any()
    # a BLS12-377 call in between (another engine pool, the same device)
    sk = 0x1234567
    Hm = ecc.E1_377.mul(ecc.G1_377, 99)
    a1, _ = co.pack_g1_377([ecc.E1_377.mul(Hm, sk), Hm])
    a2, _ = co.pack_g2_377([ecc.E2_377.neg(ecc.G2_377), ecc.E2_377.mul(ecc.G2_377, sk)])
    assert gpu.pairing_product_is_one(a1, None, a2, None)
    assert np.array_equal(_run(gpu, large, one_gt, "large after a BLS12-377 call"), first)
    assert np.array_equal(gpu.pairing_gt_bw6(*large[:5]), first)


def test_four_concurrent_callers(gpu, big, one_gt):
    """four threads, each with a batch of its own shape (the engine pool leases an engine each): every caller's rows against ITS expected
    rows, which the oracle gives"""
    shapes = ([3], [9, 0, 4, 2], _ragged_counts(21, 1), _ragged_counts(22, 2))
    batches = [pc.ragged_batch(big, c, seed=50 + t, first=40000 + 1000 * t) for t, c in enumerate(shapes)]
    want = [np.stack([pc.oracle_gt(b, p)[0] for p in range(len(b[5]))]) for b in batches]
    got, errs = [[] for _ in batches], []

    def work(t):
        try:
            for _ in range(3):
                b = batches[t]
                got[t].append((gpu.pairing_gt_bw6(*b[:5]), gpu.pairing_product_is_one_batch_bw6(*b[:5])))
        except Exception as e:  # noqa: BLE001
            errs.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errs, errs
    for t, b in enumerate(batches):
        assert len(got[t]) == 3
        for gt, ok in got[t]:
            assert np.array_equal(gt, want[t]), "caller %d" % t
            assert ok.tolist() == b[5].tolist(), "caller %d" % t
