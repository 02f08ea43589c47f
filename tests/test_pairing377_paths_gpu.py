"""GPU (-m gpu): the BLS12-377 pairing on every dispatch path of PairingEngine<PP377>::run_staged (csrc/pairing.h), whole batches against
the oracle.  Every comparison is bit for bit on arkworks Montgomery limbs: GT values against co.pairing_product_377, Miller values against
co.miller_loop_377; verdicts are read twice, from pairing_gt (GT row == the packed one) and from pairing_product_is_one_batch, and compared
with the verdict each product has BY CONSTRUCTION (tests/pairing377_cases.py, whose inputs tests/test_pairing377_cases.py checks on the CPU
without the library).  m = products, k = pairs, c_p = pairs of product p.

  #    condition                                            Miller / product / final exp                              tests
  W    m <= 768, every c_p <= 3, k >= 1                     k377_wide_miller, k377_wide_final                         test_wide_*, test_768_769, test_stale (W), sequences, callers
  P1   m = 1, 4 <= k <= 8                                   k_miller_slots, k_gt_product_lanes, w3                    test_single_product_* (4, 5, 8), test_stale (P1), callers
  P2   m = 1, k > 8                                         k_miller_slots, k_gt_tree_lanes levels, w3                test_single_product_* (9 ... 64)
  P3   1 < m < 16384, not W, not S                          k_miller_slots, k_gt_product_lanes, final exp by m        test_ragged_*, test_768_769, test_final_exp_by_m, per_pair_rows,
                                                                                                                      verify_reference_rows, the fall-backs of test_split_*
  S    769 <= m <= 5120, every c_p == 2, same first G2 row  k_prepare_lines, k_miller_prepared_split_slots,           test_split_*, test_prepared_lines_cache, test_stale (S),
                                                            k_gt_product_lanes, w3 / w2                               sequences, callers
  A2p  m >= 16384, c_p <= 2, same first row, c_0 > 0        k_miller_prepared_slots, slots                            test_threshold_verify_shaped_*, test_prepared_lines_cache
  A2   m >= 16384, c_p <= 2, otherwise                      k_miller_product_slots<., 2>, slots                       test_threshold_verify_shaped_* (swapped; product 0 empty)
  A4   m >= 16384, max c_p 3 or 4                           k_miller_product_slots<., 4>, slots                       test_threshold_ragged_*
  P3'  m >= 16384, some c_p > 4                             k_miller_slots, k_gt_product_lanes, slots                 test_threshold_one_product_of_five_pairs_falls_back
  k = 0, m >= 1: the throughput row, not W                                                                            test_empty_call_shapes

  final exponentiation by m: <= 3072 k377_w3_final_products, 3073 ... 5120 k377_w2_final_products, above k_final_exp_slots; miller_only:
  k_final_exp_slots (pass-through) at every m.

  thresholds, each reached from both sides with the SAME products:
    768 | 769       test_768_769 (W against P3 + w3; and a four-pair product inside 768)
    3072 | 3073     test_final_exp_by_m (P3: w3 | w2), test_split_* (S: w3 | w2)
    5120 | 5121     test_final_exp_by_m (P3: w2 | slots), test_split_* (S | P3, w2 | slots)
    16383 | 16384   test_threshold_ragged_* (P3 | A4), test_threshold_verify_shaped_* (P3 | A2p, A2)

How much goes to the oracle.  Every product of every call has its verdict checked against construction, twice; where a second path computes
the same products every row is compared bit for bit; the oracle comparison of rows is total for m <= 300.  Above, pairing377_cases.sample
picks at most 400 products per large call: 64 seeded ones, the first, the last, 9 / 10 / 11, both sides of every threshold, the last block,
one per (pair count, class), EVERY product with a flag, then flagless accepting products up to the cap.  Measured: the C oracle takes about
13 ms for a four-pair product (5 ms for one pair), so a sample costs up to about 5 s and is 2.4 % of a call of 16421, 7.8 % of one of 5121
and 52 % of one of 768.

Left out on purpose: malformed offsets (the library does not validate them and a test must not provoke a fault); more than 64 pairs in one
product; the device-staged caller batch_verify_dev (tests/test_batch_gpu.py and tests/test_configs_gpu.py cover it)."""
import threading
import numpy as np
import pytest
import torch  # noqa: F401  (before the library: torch brings its own HIP runtime; loaded after the library's, it finds no device)
from oracle import cpu_oracle as co
from tests import pairing377_cases as pc

pytestmark = pytest.mark.gpu

SEED_SMALL, SEED_BIG = 0x377A11E, 0x377B16
N_BIG = pc.N_BIG
GROUPS = 10                      # LPH377::GROUPS: six-lane groups per 64-thread block
SHARED_MIN, M_BIG = pc.SHARED_MIN, pc.M_BIG
WIDE_MAX, W3_MAX, SPLIT_MAX = pc.WIDE_MAX, 3072, pc.SPLIT_MAX
FE_THRESHOLDS = (WIDE_MAX, W3_MAX, SPLIT_MAX)


@pytest.fixture(scope="module")
def small():
    return pc.python_points(160, SEED_SMALL)


@pytest.fixture(scope="module")
def big(gpu):
    return pc.device_points(N_BIG, SEED_BIG)


@pytest.fixture(scope="module")
def one_gt():
    gt, one = co.pairing_product_377(np.zeros((0, 12), dtype=np.uint64), None, np.zeros((0, 24), dtype=np.uint64), None)
    assert one
    return gt


def _where(p):
    p = np.asarray(p)
    return "products %s (slot kernels: block %s, group %s; w3 block %s; w2 block %s)" % (p, p // GROUPS, p % GROUPS, p // 3, p // 5)


def _sub(batch, a, b):
    """products a ... b - 1 of a batch as a batch of their own"""
    g1, i1, g2, i2, offs, expect = batch
    lo, hi = int(offs[a]), int(offs[b])
    return g1[lo:hi], i1[lo:hi], g2[lo:hi], i2[lo:hi], (offs[a:b + 1] - offs[a]).astype(np.uint32), expect[a:b]


def _run(gpu, batch, one_gt, what):
    """GT rows and both verdict vectors of one batch; the verdicts must agree with each other and with construction"""
    g1, i1, g2, i2, offs, expect = batch
    gt = gpu.pairing_gt(g1, i1, g2, i2, offs)
    by_gt = (gt == one_gt[None, :]).all(axis=1)
    by_entry = gpu.pairing_product_is_one_batch(g1, i1, g2, i2, offs)
    bad = np.nonzero(by_gt != expect.astype(bool))[0]
    assert bad.size == 0, "%s: GT verdict differs from construction at %s, %d in all" % (what, _where(bad[:8]), bad.size)
    bad = np.nonzero(by_entry.astype(bool) != expect.astype(bool))[0]
    assert bad.size == 0 and set(np.unique(by_entry)) <= {0, 1}, "%s: is_one differs from construction at %s, %d in all" % (what, _where(bad[:8]), bad.size)
    return gt


def _miller(gpu, batch):
    return gpu.pairing_gt(*batch[:5], miller_only=True)


def _against_oracle(batch, gt, products, what, ml=None):
    for p in products:
        p = int(p)
        want, one = pc.oracle_gt(batch, p)
        assert bool(one) == bool(batch[5][p]), "%s: oracle verdict of product %d differs from construction" % (what, p)
        assert np.array_equal(gt[p], want), "%s: GT value of %s, %d pairs" % (what, _where(p), int(batch[4][p + 1] - batch[4][p]))
        if ml is not None:
            assert np.array_equal(ml[p], pc.oracle_miller(batch, p)), "%s: Miller value of %s" % (what, _where(p))


def _same_rows(got, want, what, skip=()):
    keep = np.ones(got.shape[0], dtype=bool)
    keep[list(skip)] = False
    diff = np.nonzero((got != want).any(axis=1) & keep)[0]
    assert diff.size == 0, "%s: rows differ at %s, %d in all" % (what, _where(diff[:8]), diff.size)


def _single(gpu, batch, one_gt, what):
    """one product: Miller value, GT value, verdict (both batched entries and the single-product entry) against the oracle"""
    g1, i1, g2, i2, offs, expect = batch
    ml = _miller(gpu, batch)
    gt = _run(gpu, batch, one_gt, what)
    _against_oracle(batch, gt, [0], what, ml)
    assert bool(gpu.pairing_product_is_one(g1, i1, g2, i2)) == bool(expect[0]), what
    return gt


def test_device_generated_points_are_the_oracles(big):
    """the large cases rely on rows k_i A, k_i B from the generator kernel: a sample of them, bit for bit, against the Python oracle's"""
    idx = sorted({0, 1, 9, 10, 11, 4095, 16383, 16384, 65535, N_BIG - 1} | set(np.random.default_rng(1).integers(0, N_BIG, size=22).tolist()))
    g1, g2 = pc.python_rows(SEED_BIG, idx)
    assert big.P.shape == (N_BIG, 12) and big.Q.shape == (N_BIG, 24)
    assert np.array_equal(big.P[idx], g1) and np.array_equal(big.Q[idx], g2)


# ------------------------------------------------------------------------------------------------ W: the latency path
@pytest.mark.parametrize("k", [1, 2, 3])
def test_wide_single_product_every_k(gpu, small, one_gt, k):
    """csrc/unit_pairing377_wide.hip, m = 1: k unrelated pairs; then the infinity flag in every position, once through inf1 and once through
    inf2, a zero row or a stale valid row behind it; all pairs flagged; NULL flag pointers after calls that had them; accept and mismatch at
    k = 2.  Miller (a product of partial values on this path) and GT against the oracle, all three verdict entries."""
    live = pc.layout(small, [pc.product(small, k, "unrelated", 7 * k)])
    _single(gpu, live, one_gt, "W k=%d" % k)
    g1, _, g2, _, offs, _ = live
    for pos in range(k):
        for which in (1, 2):
            i1 = np.zeros(k, dtype=np.uint8); i2 = np.zeros(k, dtype=np.uint8)
            (i1 if which == 1 else i2)[pos] = 1
            a1, a2 = g1.copy(), g2.copy()
            if (pos + which) & 1:
                (a1 if which == 1 else a2)[pos] = 0              # what the packers write for a point at infinity; otherwise a stale valid row
            _single(gpu, (a1, i1, a2, i2, offs, np.array([1 if k == 1 else 0], dtype=np.uint8)), one_gt, "W k=%d inf%d[%d]" % (k, which, pos))
    off = pc.layout(small, [pc.product(small, k, "all_off", 5 * k)])
    gt = _single(gpu, off, one_gt, "W k=%d all pairs flagged" % k)
    assert np.array_equal(gt[0], one_gt)
    gt = gpu.pairing_gt(g1, None, g2, None, offs)                # no flag arrays at all (NULL pointers), after calls that had them
    assert np.array_equal(gt[0], co.pairing_product_377(g1, None, g2, None)[0])
    assert np.array_equal(gpu.pairing_gt(g1, None, g2, None, offs, miller_only=True)[0], co.miller_loop_377(g1, None, g2, None))
    if k >= 2:
        for variant in ("accept", "mismatch", "first_off", "half_off"):
            s = pc.product(small, k, variant, 3 * k + 20, flag_pos=k - 1 if k % 2 else 1)
            gt = _single(gpu, pc.layout(small, [s]), one_gt, "W k=%d %s" % (k, variant))
            assert np.array_equal(gt[0], one_gt) == (variant == "accept")


@pytest.mark.parametrize("m", [40, 768])
def test_wide_ragged_batches(gpu, big, one_gt, m):
    """W, a block per product: counts 0 ... 3, empty products at the start, in the middle and at the end, flags inside.  m = 40: every GT and
    Miller row against the oracle; m = 768 (the largest): every verdict, and the sample."""
    specs = pc.wide_specs(big, m, first=5 * m)
    batch = pc.layout(big, specs)
    assert batch[1].any() and batch[3].any() and 0 < int(batch[5].sum()) < m and max(len(s) for s in specs) == 3
    gt = _run(gpu, batch, one_gt, "W m=%d" % m)
    pick = range(m) if m <= 300 else pc.sample(specs, 320 + m, thresholds=(WIDE_MAX,))
    if m > 300:
        pc.check_sample(specs, pick, 320 + m, thresholds=(WIDE_MAX,))
    _against_oracle(batch, gt, pick, "W m=%d" % m, _miller(gpu, batch))


def test_wide_two_products(gpu, big, one_gt):
    """W, m = 2: an empty product first and three pairs (a couple and a pair flagged through inf2); then three unrelated pairs and half a couple"""
    for specs in ([pc.product(big, 0, "accept", 0), pc.product(big, 3, "accept", 700, which=2)],
                  [pc.product(big, 3, "unrelated", 710), pc.product(big, 2, "half_off", 720, which=1)],
                  [pc.product(big, 1, "unrelated", 730), pc.product(big, 0, "accept", 0)]):
        batch = pc.layout(big, specs)
        gt = _run(gpu, batch, one_gt, "W m=2")
        _against_oracle(batch, gt, [0, 1], "W m=2", _miller(gpu, batch))


def test_empty_call_shapes(gpu, one_gt):
    """k = 0 leaves W (it needs k >= 1): one empty product is 1 and its GT value is one; so are three, miller_only too; m = 0 is accepted"""
    z1, z2, f = np.zeros((0, 12), dtype=np.uint64), np.zeros((0, 24), dtype=np.uint64), np.zeros(0, dtype=np.uint8)
    for m in (1, 3):
        b = (z1, f, z2, f, np.zeros(m + 1, dtype=np.uint32), np.ones(m, dtype=np.uint8))
        gt = _run(gpu, b, one_gt, "k=0, m=%d" % m)
        assert (gt == one_gt[None, :]).all()
        assert (gpu.pairing_gt(z1, None, z2, None, b[4], miller_only=True) == one_gt[None, :]).all()
    assert gpu.pairing_product_is_one(z1, None, z2, None)
    assert gpu.pairing_product_is_one_batch(z1, None, z2, None, np.zeros(1, dtype=np.uint32)).size == 0
    assert gpu.pairing_gt(z1, None, z2, None, np.zeros(1, dtype=np.uint32)).shape == (0, 72)


def test_768_769(gpu, big, one_gt):
    """The same 769 distinct ragged products (counts 0 ... 3): the first 768 in one call (W) and all 769 in one (P3 + w3).  Rows 0 ... 767
    equal bit for bit, the Miller rows too (W's product of partial values against k_final_exp_slots' pass-through).  Then 768 products of
    which ONE has four pairs (leaves W): all other rows unchanged."""
    counts = pc.wide_counts(769)
    counts[768] = 3
    specs = pc.ragged_specs(big, counts, seed=769, first=9000)
    batch = pc.layout(big, specs)
    wide, both = _sub(batch, 0, WIDE_MAX), batch
    gt_w, gt_p = _run(gpu, wide, one_gt, "m=768 (W)"), _run(gpu, both, one_gt, "m=769 (P3 + w3)")
    _same_rows(gt_p[:WIDE_MAX], gt_w, "GT, m=769 against m=768")
    _same_rows(_miller(gpu, both)[:WIDE_MAX], _miller(gpu, wide), "Miller, m=769 against m=768")
    _against_oracle(both, gt_p, [0, 1, 766, 767, 768], "m=769 (P3 + w3)")
    at = 400
    mixed = specs[:WIDE_MAX]
    mixed[at] = pc.product(big, 4, "mismatch", 9000 + 4 * 770)
    b4 = pc.layout(big, mixed)
    gt_4 = _run(gpu, b4, one_gt, "m=768 with a four-pair product (P3)")
    _same_rows(gt_4, gt_w, "GT, m=768 with a four-pair product against W", skip=[at])
    _against_oracle(b4, gt_4, [at - 1, at, at + 1], "m=768 with a four-pair product", _miller(gpu, b4))


# ------------------------------------------------------------------------------------------------ P1, P2: one product on the per-pair kernels
@pytest.mark.parametrize("k", [4, 5, 8, 9, 10, 11, 20, 21, 43, 64])
def test_single_product_on_the_per_pair_kernels(gpu, small, one_gt, k):
    """m = 1, k >= 4: k_miller_slots<LPH377> (ten groups per block: k = 10 | 11 and 20 | 21 are a full block and one more), then
    k_gt_product_lanes (k <= 8) or the product tree k_gt_tree_lanes (k > 8; 9 -> 5 -> 3 -> 2 -> 1, 11 -> 6 -> 3 -> 2 -> 1 and
    43 -> 22 -> 11 -> 6 -> 3 -> 2 -> 1 have levels with an odd count), then k377_w3_final_products with a single product."""
    path = "P1" if k <= 8 else "P2"
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


# ------------------------------------------------------------------------------------------------ P3: ragged batches on the per-pair kernels
def _ragged_counts(m, seed):
    """pair counts 0 ... 9; empty products at the start, in the middle and at the end; product 2 covers pairs 9 ... 17 (m >= 10): it
    straddles the boundary between the first two blocks of k_miller_slots (ten pairs each)"""
    c = np.random.default_rng(seed).integers(0, pc.MAX_PAIRS + 1, size=m)
    if m >= 10:
        c[:3] = [0, 9, 9]
        c[m // 2] = 0
        c[m - 1] = 0
        c[m - 2] = 9
    return [int(x) for x in c]


@pytest.mark.parametrize("m", [2, 10, 11, 300])
def test_ragged_batches_on_the_per_pair_path(gpu, big, one_gt, m):
    """1 < m < 16384 with products of more than three pairs: k_miller_slots per pair, k_gt_product_lanes per product (offsets ragged, empty
    products, flags inside), k377_w3_final_products (m = 300 = 3 * 100: whole super-groups; 10 and 11: a surplus one).  m = 10 / 11: one
    block of products and one more.  Every verdict against construction, EVERY GT row against the oracle, Miller rows too for m <= 11."""
    if m == 2:        # nine pairs (four couples and a pair flagged through inf2) accepting, four pairs with the first pair flagged through inf1
        specs = [pc.product(big, 9, "accept", 2002, which=2), pc.product(big, 4, "first_off", 2020, which=1)]
    else:
        specs = pc.ragged_specs(big, _ragged_counts(m, 100 + m), seed=200 + m, first=1000 * (m % 7))
    batch = pc.layout(big, specs)
    g1, i1, g2, i2, offs, expect = batch
    if m >= 10:
        assert offs[1] == 0 and offs[2] < GROUPS < offs[3] and offs[m // 2] == offs[m // 2 + 1] and offs[m - 1] == offs[m]
    assert i1.any() and i2.any() and 0 < int(expect.sum()) < m
    gt = _run(gpu, batch, one_gt, "P3 m=%d" % m)
    _against_oracle(batch, gt, range(m), "P3 m=%d" % m, _miller(gpu, batch) if m <= 11 else None)


def test_ragged_batch_ending_in_a_surplus_super_group(gpu, big, one_gt):
    """m = 301 = 3 * 100 + 1: k377_w3_final_products ends in a super-group with one product"""
    specs = pc.ragged_specs(big, _ragged_counts(301, 401), seed=501, first=12000)
    batch = pc.layout(big, specs)
    gt = _run(gpu, batch, one_gt, "P3 m=301")
    _against_oracle(batch, gt, [0, 1, 2, 297, 298, 299, 300], "P3 m=301")


# ------------------------------------------------------------------------------------------------ final exponentiation by m on P3
@pytest.fixture(scope="module")
def final_exp_batch(big):
    specs = pc.final_exp_specs(big)
    return specs, pc.layout(big, specs)


@pytest.fixture(scope="module")
def final_exp_rows(gpu, final_exp_batch, one_gt):
    """GT rows of the prefixes 3072 (w3), 3073 (w2), 5120 (w2), 5121 (slots) of one set of 5121 distinct ragged products, every verdict checked"""
    _, batch = final_exp_batch
    return {m: _run(gpu, _sub(batch, 0, m), one_gt, "P3 m=%d" % m) for m in (W3_MAX, W3_MAX + 1, SPLIT_MAX, SPLIT_MAX + 1)}


def test_final_exp_by_m_rows_equal_across_the_thresholds(gpu, final_exp_batch, final_exp_rows):
    """3072 | 3073 and 5120 | 5121 with the same products: rows of the common prefix equal bit for bit across the four calls (three final
    exponentiation kernels); miller_only (k_final_exp_slots at every m) rows at 3073 equal those at 5121"""
    specs, batch = final_exp_batch
    assert max(len(s) for s in specs) == 4 and any(len(s) == 4 for s in specs[:769]) and batch[1].any() and batch[3].any()
    full = final_exp_rows[SPLIT_MAX + 1]
    for m in (W3_MAX, W3_MAX + 1, SPLIT_MAX):
        _same_rows(final_exp_rows[m], full[:m], "GT, P3 m=%d against m=5121" % m)
    _same_rows(_miller(gpu, _sub(batch, 0, W3_MAX + 1)), _miller(gpu, batch)[:W3_MAX + 1], "Miller, P3 m=3073 against m=5121")


def test_final_exp_by_m_sample_against_oracle(final_exp_batch, final_exp_rows):
    specs, batch = final_exp_batch
    pick = pc.sample(specs, 5123, thresholds=FE_THRESHOLDS)
    pc.check_sample(specs, pick, 5123, thresholds=FE_THRESHOLDS)
    _against_oracle(batch, final_exp_rows[SPLIT_MAX + 1], pick, "P3 m=5121")


# ------------------------------------------------------------------------------------------------ S: verify-shaped products cut in two
@pytest.fixture(scope="module")
def split_batch(big):
    specs = pc.split_threshold_specs(big)
    return specs, pc.layout(big, specs)


@pytest.fixture(scope="module")
def split_rows_5121(gpu, split_batch, one_gt):
    """the 5121 verify-shaped products in ONE call: past SPLIT_MAX_PRODUCTS, so P3 + k_final_exp_slots"""
    return _run(gpu, split_batch[1], one_gt, "verify-shaped m=5121 (P3)")


@pytest.mark.parametrize("m", [769, 3072, 3073, 5120])
def test_split_path(gpu, big, split_batch, split_rows_5121, one_gt, m):
    """769 <= m <= 5120 distinct verify-shaped products of exactly two pairs: k_prepare_lines + k_miller_prepared_split_slots (two blocks
    per ten products; 769 = 10 * 76 + 9: the last block pair has an idle group), k_gt_product_lanes, then w3 (m <= 3072) or w2 (3073 is
    1 mod 3 and 3 mod 5).  Kinds: accept, mismatch, second pair flagged, FIRST pair flagged (live_a and live_b are separate code), both,
    each through inf1 and inf2.  Every verdict; Miller and GT rows of the sample against the oracle; EVERY GT row equal to the row of the
    same call with one product swapped (which sends the call to P3), to the row of the m = 5121 call, and to the row of the same call with
    one product cut to one pair (k != 2 m: P3)."""
    specs = split_batch[0][:m]
    batch = _sub(split_batch[1], 0, m)
    assert pc.first_rows_shared(big, specs) and (np.diff(batch[4].astype(np.int64)) == 2).all()
    what = "S m=%d" % m
    gt = _run(gpu, batch, one_gt, what)
    pick = pc.sample(specs, 7100 + m, thresholds=FE_THRESHOLDS)
    pc.check_sample(specs, pick, 7100 + m, thresholds=FE_THRESHOLDS)
    _against_oracle(batch, gt, pick, what, _miller(gpu, batch))
    _same_rows(gt, split_rows_5121[:m], "GT, %s against m=5121 (P3)" % what)
    at = (2 * m) // 3
    swapped = list(specs)
    swapped[at] = pc.swapped(specs[at])
    bs = pc.layout(big, swapped)
    assert not pc.first_rows_shared(big, swapped) and np.array_equal(bs[4], batch[4])
    gt_s = _run(gpu, bs, one_gt, what + " with product %d swapped (P3)" % at)
    _same_rows(gt, gt_s, "GT, %s against the same call with product %d swapped" % (what, at), skip=[at])
    _against_oracle(bs, gt_s, [at], what + " swapped", _miller(gpu, bs))
    at = m // 3
    cut = list(specs)
    cut[at] = pc.verify_product(big, 1, "live", 2 * at)
    bc = pc.layout(big, cut)
    assert pc.first_rows_shared(big, cut) and bc[4][-1] == 2 * m - 1
    gt_c = _run(gpu, bc, one_gt, what + " with product %d of one pair (P3)" % at)
    _same_rows(gt, gt_c, "GT, %s against the same call with a one-pair product" % what, skip=[at])
    _against_oracle(bc, gt_c, [at], what + " one-pair product")


# ------------------------------------------------------------------------------------------------ the 16384 threshold: A4, P3'
@pytest.fixture(scope="module")
def threshold_batch(big):
    """16421 distinct products of 0 ... 4 pairs: accepts, rejects, unrelated points, flags through inf1 and inf2 (about 1.5 % carry one)"""
    specs = pc.threshold_specs(big)
    return specs, pc.layout(big, specs)


@pytest.fixture(scope="module")
def per_pair_rows(gpu, threshold_batch, one_gt):
    """GT rows of all 16421 products from P3: the first 16383 in one call (the largest below the threshold), the rest in a second"""
    _, batch = threshold_batch
    a = _run(gpu, _sub(batch, 0, SHARED_MIN - 1), one_gt, "m=16383 (P3)")
    b = _run(gpu, _sub(batch, SHARED_MIN - 1, M_BIG), one_gt, "m=38 (P3)")
    return np.concatenate([a, b])


@pytest.mark.parametrize("m", [SHARED_MIN, M_BIG])
def test_threshold_ragged_shared_accumulator_rows_equal_per_pair_rows(gpu, threshold_batch, per_pair_rows, one_gt, m):
    """m >= 16384, every product <= 4 pairs, some of three or four: k_miller_product_slots<LPH377, 4>, one group per product, and
    k_final_exp_slots (16384 = 10 * 1638 + 4, 16421 = 10 * 1642 + 1).  Every verdict against construction; EVERY GT row equal, bit for
    bit, to the row P3 gave for the same product in calls below the threshold; Miller and GT rows of the sample against the oracle."""
    specs, batch = threshold_batch
    assert max(len(s) for s in specs[SHARED_MIN - 1:]) == 4          # (so the call of 38 is not W)
    sub = _sub(batch, 0, m)
    gt = _run(gpu, sub, one_gt, "m=%d (A4)" % m)
    _same_rows(gt, per_pair_rows[:m], "GT, m=%d (A4) against P3" % m)
    pick = pc.sample(specs[:m], 16386, thresholds=(SHARED_MIN,))
    pc.check_sample(specs[:m], pick, 16386, thresholds=(SHARED_MIN,))
    _against_oracle(sub, gt, pick, "m=%d (A4)" % m, _miller(gpu, sub))


def test_threshold_one_product_of_five_pairs_falls_back(gpu, big, threshold_batch, per_pair_rows, one_gt):
    """P3': a batch of 16421 in which ONE product has five pairs leaves A4 (k_miller_slots + k_gt_product_lanes + k_final_exp_slots): the
    same rows for all the others, the five-pair product against the oracle"""
    specs, _ = threshold_batch
    at = 8000
    mixed = list(specs)
    mixed[at] = pc.product(big, 5, "extra_live", 5 * M_BIG + 10)
    batch = pc.layout(big, mixed)
    gt = _run(gpu, batch, one_gt, "m=16421 with a five-pair product (P3')")
    _same_rows(gt, per_pair_rows, "GT, P3' against P3", skip=[at])
    _against_oracle(batch, gt, [at - 1, at, at + 1], "m=16421 with a five-pair product (P3')")


# ------------------------------------------------------------------------------------------------ the 16384 threshold: A2p, A2
@pytest.fixture(scope="module")
def verify_batch(big):
    """16421 distinct verify-shaped products of 0 ... 2 pairs: one-pair products (P_i, B), empties (not at index 0), flags on the first
    and on the second pair through inf1 and inf2"""
    specs = pc.verify_threshold_specs(big)
    return specs, pc.layout(big, specs)


@pytest.fixture(scope="module")
def verify_reference_rows(gpu, big, verify_batch, one_gt):
    """GT rows of the 16421 verify-shaped products from P3, in two calls below 16384: the first 16383 (ragged counts: neither W nor S) and
    the other 38 with a four-pair product appended (38 products of <= 2 pairs alone would be W)"""
    specs, batch = verify_batch
    assert {len(s) for s in specs[:SHARED_MIN - 1]} == {0, 1, 2}
    a = _run(gpu, _sub(batch, 0, SHARED_MIN - 1), one_gt, "verify-shaped m=16383 (P3)")
    tail = pc.layout(big, specs[SHARED_MIN - 1:] + [pc.product(big, 4, "mismatch", 2 * M_BIG + 10)])
    b = _run(gpu, tail, one_gt, "verify-shaped m=38 + 1 (P3)")
    return np.concatenate([a, b[:-1]])


def test_threshold_verify_shaped_prepared_rows_equal_per_pair_rows(gpu, big, verify_batch, verify_reference_rows, one_gt):
    """A2p: m = 16421, every product <= 2 pairs, every first pair on B, product 0 non-empty: k_miller_prepared_slots (pair 0 on the prepared
    lines, one-pair products walk a dead second pair).  EVERY row equal to P3's; Miller and GT rows of the sample against the oracle."""
    specs, batch = verify_batch
    assert pc.first_rows_shared(big, specs) and len(specs[0]) == 2 and max(len(s) for s in specs) == 2
    gt = _run(gpu, batch, one_gt, "m=16421 (A2p)")
    _same_rows(gt, verify_reference_rows, "GT, A2p against P3")
    pick = pc.sample(specs, 16392, thresholds=(SHARED_MIN,))
    pc.check_sample(specs, pick, 16392, thresholds=(SHARED_MIN,))
    _against_oracle(batch, gt, pick, "m=16421 (A2p)", _miller(gpu, batch))


def test_threshold_verify_shaped_fall_backs(gpu, big, verify_batch, verify_reference_rows, one_gt):
    """A2: the same batch with ONE product swapped (another first G2 row: k_first_q_same clears the flag, k_miller_product_slots<., 2> runs)
    gives every row again; so does the batch with product 0 EMPTY (k_first_q_same refuses: there is no first row to compare with)"""
    specs, _ = verify_batch
    at = next(p for p in range(12000, M_BIG) if specs[p].kind == "accept")
    sw = list(specs)
    sw[at] = pc.swapped(specs[at])
    assert not pc.first_rows_shared(big, sw)
    gt = _run(gpu, pc.layout(big, sw), one_gt, "m=16421 with product %d swapped (A2)" % at)
    _same_rows(gt, verify_reference_rows, "GT, A2 (one product swapped) against P3")
    first_empty = [pc.verify_product(big, 0, "empty", 0)] + list(specs[1:])
    be = pc.layout(big, first_empty)
    gt = _run(gpu, be, one_gt, "m=16421 with product 0 empty (A2)")
    assert np.array_equal(gt[0], one_gt)
    _same_rows(gt, verify_reference_rows, "GT, A2 (product 0 empty) against P3", skip=[0])
    _against_oracle(be, gt, [0, 1, 2, 3, M_BIG - 1], "m=16421 with product 0 empty (A2)")


# ------------------------------------------------------------------------------------------------ the prepared-lines cache
def test_prepared_lines_cache_follows_the_shared_point(gpu, big, one_gt):
    """lines_valid / lines_at / lines_q0 (csrc/pairing.h): the engine keeps the 69 line triples of the shared G2 row between calls.  One
    caller, so one engine: S at m = 1003 over B; the SAME (k, m), offsets and flags over Q_J; B again; A2p at 16421 over Q_J, then over B;
    S at 1003 over B (another layout in between: the lines are recomputed at the new place).  Every call: all verdicts against construction
    (lines of the other point turn every accepting product into a reject, so the verdicts alone check the whole batch) and 16 GT rows
    against the oracle."""
    ptsj, fam = pc.family_over(big, N_BIG - 1)
    s_b = pc.split_specs(ptsj, 1003, seed=1003, first=40000)
    s_j = pc.split_specs(ptsj, 1003, seed=1003, first=40000, family=fam)
    a_b = pc.verify_threshold_specs(ptsj)
    a_j = pc.verify_threshold_specs(ptsj, family=fam)
    lb, lj = pc.layout(ptsj, s_b), pc.layout(ptsj, s_j)
    assert np.array_equal(lb[4], lj[4]) and np.array_equal(lb[5], lj[5]) and not np.array_equal(lb[2][0], lj[2][0]) and pc.first_rows_shared(ptsj, s_j, fam)
    assert 300 < int(lb[5].sum()) < 700
    rows = {}
    for step, (name, specs, f) in enumerate((("S over B", s_b, None), ("S over Q_J", s_j, fam), ("S over B", s_b, None), ("A2p over Q_J", a_j, fam),
                                             ("A2p over B", a_b, None), ("S over B", s_b, None))):
        batch = pc.layout(ptsj, specs)
        what = "cache step %d, %s" % (step, name)
        gt = _run(gpu, batch, one_gt, what)
        m = len(specs)
        pick = [0, m - 1] + np.random.default_rng(90 + step).choice(m, size=14, replace=False).tolist()
        _against_oracle(batch, gt, pick, what)
        if name in rows:
            _same_rows(gt, rows[name], what + " against its earlier call")
        rows[name] = gt


# ------------------------------------------------------------------------------------------------ stale rows
def _stale_specs(pts, path, m, first):
    """-> (all accepting, the same with a last product that rejects), the products shaped so that the call takes `path`"""
    if path == "W3":                       # m = 1, k = 3: a couple and a flagged pair | a couple and a live unrelated pair
        return [pc.product(pts, 3, "accept", first)], [pc.product(pts, 3, "extra_live", first)]
    if path == "P1":
        return [pc.product(pts, 8, "accept", first)], [pc.product(pts, 8, "mismatch", first)]
    if path == "W":
        accept = [pc.product(pts, 2 + (p & 1), "accept", first + 10 * p, which=1 + (p & 1)) for p in range(m)]
        last = pc.product(pts, len(accept[-1]), "extra_live" if len(accept[-1]) % 2 else "mismatch", first + 10 * (m - 1))
    elif path == "P3":                     # c = 2 with a four-pair product in front
        accept = [pc.product(pts, 4, "accept", first)] + [pc.verify_product(pts, 2, "accept", first + 10 * p) for p in range(1, m)]
        last = pc.verify_product(pts, 2, "mismatch", first + 10 * (m - 1), first + 10 * (m - 1) + 1)
    else:                                  # S
        accept = [pc.verify_product(pts, 2, "accept", first + 2 * p) for p in range(m)]
        last = pc.verify_product(pts, 2, "mismatch", first + 2 * (m - 1), first + 2 * (m - 1) + 1)
    return accept, accept[:-1] + [last]


@pytest.mark.parametrize("path,m", [("W3", 1), ("W", 4), ("P1", 1), ("P3", 11), ("P3", 21), ("S", 769), ("P3", 3073)])
def test_last_product_is_written_over_stale_rows(gpu, big, one_gt, path, m):
    """Three calls of the SAME shape one after the other, so that the arena rows of the earlier call sit exactly where the later call
    writes: all accept, then the same call with a LAST product that does not, then all accept again.  A kernel that leaves the last product
    of a call unwritten returns the stale row of the call before - one where it must not be, not one where it must be.  W (m = 1, k = 3 and
    m = 4), P1 (k = 8), P3 + w3 (m = 11: a block's first group; m = 21), S + w3 (m = 769), P3 + w2 (m = 3073: a surplus block of w2).
    Miller and GT of the first and the last product against the oracle each time."""
    accept, reject = _stale_specs(big, path, m, 50000)
    assert reject[-1].expect == 0 and all(s.expect == 1 for s in accept) and [len(s) for s in accept] == [len(s) for s in reject]
    for what, specs in (("all accept", accept), ("last product rejects", reject), ("all accept again", accept)):
        batch = pc.layout(big, specs)
        what = "%s m=%d, %s" % (path, m, what)
        gt = _run(gpu, batch, one_gt, what)
        _against_oracle(batch, gt, sorted({0, m - 1}), what, _miller(gpu, batch))


# ------------------------------------------------------------------------------------------------ call sequences on the engine arena
def test_call_sequences_reuse_the_arena(gpu, small, big, one_gt):
    """large P3 -> W -> the same large P3; S -> W -> S; flags then NULL flag pointers on the same shape (stale flag bytes of the earlier
    call sit in the arena and must not be read); a BW6-761 call in between: identical bytes every time."""
    from oracle.py import ecc
    large = pc.layout(big, pc.ragged_specs(big, _ragged_counts(300, 7), seed=8, first=20000))
    tiny = pc.layout(small, [pc.product(small, 3, "unrelated", 40)])
    split = pc.layout(big, pc.split_specs(big, 769, seed=11, first=60000))
    first = _run(gpu, large, one_gt, "large P3")
    _against_oracle(large, first, [0, 1, 2, 150, 298, 299], "large P3")
    _single(gpu, tiny, one_gt, "W after a large P3")
    _same_rows(_run(gpu, large, one_gt, "large P3 again"), first, "large P3 after W")
    s_first = _run(gpu, split, one_gt, "S")
    _against_oracle(split, s_first, [0, 1, 400, 767, 768], "S")
    _single(gpu, tiny, one_gt, "W after S")
    _same_rows(_run(gpu, split, one_gt, "S again"), s_first, "S after W")
    # flags, then none: every product is half a couple switched off (not 1) whose rows are valid, so without flags every product is 1;
    # 30 products on W, and 769 on S (first and second pairs flagged in turn, through inf1 and inf2)
    for m, what in ((30, "W"), (769, "S")):
        specs = [pc.verify_product(big, 2, ("second_off", "first_off")[p & 1], 30000 + 2 * p, which=1 + ((p >> 1) & 1)) for p in range(m)]
        off = pc.layout(big, specs)
        _run(gpu, off, one_gt, "%d half couples (%s)" % (m, what))
        g1, i1, g2, i2, offs, _ = off
        assert i1.any() and i2.any() and g1.any(axis=1).all() and g2.any(axis=1).all()
        assert (gpu.pairing_gt(g1, None, g2, None, offs) == one_gt[None, :]).all(), "%s: stale flag bytes were read" % what
        assert gpu.pairing_product_is_one_batch(g1, None, g2, None, offs).all(), what
        by1 = gpu.pairing_product_is_one_batch(g1, i1, g2, None, offs)
        assert by1.tolist() == [0 if (any(s.f1)) else 1 for s in specs], what
    # a BW6-761 call in between (another engine pool, the same device)
    from tests import pairing761_cases as pc761
    A, B = pc761.generators()
    a1, _ = co.pack_761([ecc.E1_761.mul(A, 77), ecc.E1_761.neg(A)])
    a2, _ = co.pack_761([B, ecc.E2_761.mul(B, 77)])
    assert gpu.pairing_product_is_one_bw6(a1, None, a2, None)
    _same_rows(_run(gpu, large, one_gt, "large P3 after a BW6-761 call"), first, "large P3 after a BW6-761 call")
    _same_rows(gpu.pairing_gt(*split[:5]), s_first, "S after a BW6-761 call")


def test_four_concurrent_callers(gpu, small, big, one_gt):
    """four threads, each with a batch of its own shape (the engine pool leases an engine each): W (m = 3), P1 (k = 8), P3 (m = 11, ragged)
    and S (m = 769), three rounds each.  Every caller's verdicts against construction; GT rows against oracle rows computed beforehand:
    all rows of the three small shapes, 16 sampled rows of S."""
    batches = [pc.layout(big, pc.ragged_specs(big, [3, 0, 2], seed=50, first=70000)),
               pc.layout(big, [pc.product(big, 8, "mismatch", 70100)]),
               pc.layout(big, pc.ragged_specs(big, _ragged_counts(11, 1), seed=51, first=70200)),
               pc.layout(big, pc.split_specs(big, 769, seed=52, first=71000))]
    picks = [list(range(len(b[5]))) for b in batches[:3]] + [[0, 768] + np.random.default_rng(53).choice(769, size=14, replace=False).tolist()]
    want = [{p: pc.oracle_gt(b, p)[0] for p in pick} for b, pick in zip(batches, picks)]
    got, errs = [[] for _ in batches], []

    def work(t):
        try:
            for _ in range(3):
                b = batches[t]
                got[t].append((gpu.pairing_gt(*b[:5]), gpu.pairing_product_is_one_batch(*b[:5])))
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
            assert ok.tolist() == b[5].tolist(), "caller %d" % t
            assert ((gt == one_gt[None, :]).all(axis=1) == b[5].astype(bool)).all(), "caller %d" % t
            for p, row in want[t].items():
                assert np.array_equal(gt[p], row), "caller %d, %s" % (t, _where(p))
