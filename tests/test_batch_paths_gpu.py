"""GPU (-m gpu): the batched small MSMs (msm_batch_*: csrc/msm_batch.h, MsmEngine::run_batch) on every dispatch path, every instance of
every call against the C++ oracle's MSM of the same slice - affine points, bit for bit - and the dispatch the call took
(celo_amd_msm_last_timings: window bits, windows, buckets) against tests/batch_cases.py's restatement of the rule.  The inputs are proved
on the CPU in tests/test_batch_cases.py.

  size borders      [1, n, 0, n - 1, 7] for n on both sides of every window threshold (128, 256, 512, 1024) and of the points-per-thread
                    steps of k_batch_sort (256, 512), full-length scalars: the seven automatic (c, PT) pairs, all four groups
  forced windows    c = 3..7 at 40, 300 and 600 points (PT = 1, 2, 4)
  scalar length     BW6-761: the longest scalar in every 16-byte group of k_scalar_or<12> and on both sides of the 32-bit limb borders
  instance count    m on both sides of the block borders of k_batch_horner_lanes (21), k_batch_horner_hex (10) and k_batch_reduce (128 lanes)
  Horner branches   doubling, a chain through the identity, window sums empty by cancellation, an identity from live windows
  GLS gates         nd * max_n <= 1024 at its three edges on the G2 subgroup entry
  k_scalar_or       a longest scalar that only the second pass of the grid-stride loop sees
  side path         the host form with an instance above 1024 points, with empty instances only, with no instance
  container bits    bits from SCALAR_BITS up are ignored, as on the single-MSM entry points and on the side path
Points come from the library's generator kernel (synthetic.device_points); a sample is compared with the Python oracle first."""
import numpy as np
import pytest
import torch  # noqa: F401  (before the library: torch brings its own HIP runtime; loaded after the library's, it finds no device)
from oracle import cpu_oracle as co
from tests import batch_cases as bc
from tests import helpers as H

pytestmark = pytest.mark.gpu

G1, G2, W1, W2 = "bls12_377_g1", "bls12_377_g2", "bw6_761_g1", "bw6_761_g2"
TABLE_N = 2112                     # the largest call but one: 1 + 1024 + 0 + 1023 + 7 points
SEEDS = {G1: 0xBA7C0001, G2: 0xBA7C0002, W1: 0xBA7C0003, W2: 0xBA7C0004}
STRIDE_POINTS = 2048 * 256 * 4 // 8      # scalars of 8 words that one pass of k_scalar_or's 2048 x 256 lanes of 16 bytes covers


def entry_id(e):
    return e[0] + ("_subgroup" if e[1] else "")


def device_table(group, n, seed):
    from celo_bls_snark_rs_amd import synthetic as syn
    return syn.device_points(group, n, seed).view(n, bc.GROUPS[group].rows).cpu().numpy().view(np.uint64)


@pytest.fixture(scope="module")
def tables(gpu):
    return {g: device_table(g, TABLE_N, s) for g, s in SEEDS.items()}


@pytest.fixture(scope="module")
def hand_points():
    """a few Python-oracle multiples of each generator for the hand-built instances: (P, R, P2)"""
    return {g: bc.GROUPS[g].multiples([0x51DE, 0xC0FFEE77, 0x900D5EED]) for g in (G1, G2, W1)}


def oracle_points(call, scalars=None):
    """the expected affine point of every instance (None: the identity), from the C++ oracle on the instance's own slice"""
    g = bc.GROUPS[call.group]
    sc = call.scalars if scalars is None else scalars
    out = []
    for lo, hi in zip(call.offsets[:-1], call.offsets[1:]):
        lo, hi = int(lo), int(hi)
        out.append(co.jac_to_affine(co.msm(call.group, call.rows[lo:hi], call.inf[lo:hi], sc[lo:hi], threads=4), g.kind) if hi > lo else None)
    return out


def check(gpu, call, subgroup=False, forced_c=0, oracle_scalars=None, want=None):
    """runs the call; every instance == the oracle (on oracle_scalars where the call's own carry bits the library must ignore) and the
    dispatch == expected_dispatch for the longest scalar present.  -> (affine results, the dispatch record)"""
    g = bc.GROUPS[call.group]
    got = gpu.msm_batch(call.group, call.rows, call.inf, call.scalars, call.offsets, subgroup=subgroup)
    t = gpu.msm_timings(call.group)
    assert got.shape == (len(call.sizes), 3 * g.rows // 2)
    got = [co.jac_to_affine(r, g.kind) for r in got]
    exp = oracle_points(call, oracle_scalars)
    wrong = [(i, k) for i, k in enumerate(call.sizes) if got[i] != exp[i]]
    assert not wrong, "instances (index, size) that differ from the oracle: %s" % wrong[:8]
    if want is not None:
        for i, P in want.items():
            assert got[i] == P, i
    d = bc.expected_dispatch(call.group, call.sizes, bc.longest(call.scalars if oracle_scalars is None else oracle_scalars), subgroup, forced_c)
    if d != "side":
        assert (t["window_bits"], t["windows"], t["buckets"]) == d[:3], (t, d)
    return got, t, d


def test_device_tables_are_the_generator_multiples(tables):
    for group, rows in tables.items():
        g = bc.GROUPS[group]
        for i in (0, 1, TABLE_N - 1):
            assert np.array_equal(rows[i], g.pack(g.multiples([H.splitmix64_at(SEEDS[group], i) | 1]))[0][0]), (group, i)
        assert len({r.tobytes() for r in rows}) == TABLE_N


# ---- size borders ---------------------------------------------------------------------------------------------------------------------
BORDERS_377 = [1, 127, 128, 255, 256, 257, 511, 512, 513, 1023, 1024]
BORDERS_761 = [127, 128, 256, 257, 512, 513, 1024]
AUTO_C = {1: 3, 127: 3, 128: 4, 255: 4, 256: 5, 257: 5, 511: 5, 512: 6, 513: 6, 1023: 6, 1024: 7}


@pytest.mark.parametrize("group,max_n", [(g, n) for g in (G1, G2) for n in BORDERS_377] + [(g, n) for g in (W1, W2) for n in BORDERS_761])
def test_size_borders(gpu, tables, group, max_n):
    """every automatic (c, PT) pair of k_batch_sort - (3,1) (4,1) (5,1) (5,2) (6,2) (6,4) (7,4) - on both sides of each border, with
    full-length scalars (252 / 376 bits): at 1024 points B = 64 counters fill the whole first wave of the LDS scan"""
    g = bc.GROUPS[group]
    sizes = [1, max_n, 0] + ([max_n - 1] if max_n > 1 else []) + [7]
    call = bc.mixed_call(group, tables[group], sizes, g.scalar_bits - 1, 0x5129 + max_n)
    _, t, d = check(gpu, call)
    assert d[0] == AUTO_C[max_n] == t["window_bits"] and t["windows"] == (g.scalar_bits - 1 + d[0]) // d[0]


# ---- forced windows --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group,c,max_n", [(g, c, n) for g in (G1, W1) for c in (3, 4, 5, 6, 7) for n in (40, 300, 600)] +
                         [(g, c, n) for g in (G2, W2) for c in (3, 7) for n in (40, 300, 600)])
def test_forced_windows(gpu, tables, group, c, max_n):
    """celo_amd_msm_set_window_bits: every window at every points-per-thread count (40, 300, 600 points: PT = 1, 2, 4)"""
    g = bc.GROUPS[group]
    call = bc.mixed_call(group, tables[group], [max_n, 9, 1], g.scalar_bits - 1, 0xF0C + 8 * max_n + c)
    gpu.set_window_bits(group, c)
    try:
        _, t, _ = check(gpu, call, forced_c=c)
    finally:
        gpu.set_window_bits(group, 0)
    assert t["window_bits"] == c and t["windows"] == (g.scalar_bits - 1 + c) // c and t["buckets"] == 3 * t["windows"] << (c - 1)


# ---- scalar length, BW6-761 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("place", ["first", "last"])
@pytest.mark.parametrize("bits", [1, 31, 32, 33, 95, 96, 97, 191, 192, 193, 319, 320, 321, 352, 353, 376])
@pytest.mark.parametrize("group", [W1, W2])
def test_scalar_length_bw6_761(gpu, tables, group, bits, place):
    """k_scalar_or<12> (three 16-byte groups per scalar) and the window count: one scalar of exactly 2^bits - 1, the first of the call or
    the last, among scalars at least 3 bits shorter"""
    sizes = [9, 40, 1, 130, 5]
    call = bc.mixed_call(group, tables[group], sizes, max(1, bits - 3), 0x761B + bits)
    at = 0 if place == "first" else sum(sizes) - 1
    bc.set_scalar(call.scalars, at, (1 << bits) - 1)
    assert call.bits() == bits and bc.longest(np.delete(call.scalars, at, axis=0)) <= max(1, bits - 3)
    _, t, _ = check(gpu, call)
    assert t["window_bits"] == 4 and t["windows"] == (bits + 4) // 4


# ---- instance count -----------------------------------------------------------------------------------------------------------------------
def count_call(group, table, hand, m, seed):
    """m instances of 1..4 points with 136-bit scalars (all of them: c = 3); at the last slot of every Horner block and the first of the
    next (slots 20 / 21 of the three-lane kernel, 9 / 10 of the hex kernel, and their multiples) a cancel-and-go-on instance whose result
    is a point of its own (R = a row no other instance holds): a result written to the wrong slot cannot equal its neighbour's"""
    g = bc.GROUPS[group]
    P = hand[group][0]
    head = g.pack([P, g.curve.neg(g.curve.mul(P, 8))])[0]
    head_sc = co.ints_to_limbs([1 << 6, 1 << 3, 1], g.limbs)
    sizes = [1 + (7 * p + p // 4) % 4 for p in range(m)]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    sc = bc.random_scalars(int(offs[-1]), g.limbs, 136, seed)
    bc.set_scalar(sc, 0, (1 << 136) - 1)                    # instance 0 is never a special one
    inst, special = [], []
    for p in range(m):
        lo, hi = int(offs[p]), int(offs[p + 1])
        if p > 0 and (p % 21 in (20, 0) or p % 10 in (9, 0)):
            inst.append((np.concatenate([head, table[lo:lo + 1]]), np.zeros(3, dtype=np.uint8), head_sc))
            special.append(p)
        else:
            inst.append((table[lo:hi], np.zeros(hi - lo, dtype=np.uint8), sc[lo:hi]))
    return bc.concat_call(group, inst), special


@pytest.mark.parametrize("m", [1, 9, 10, 11, 20, 21, 22, 41, 42, 43, 127, 128, 129, 257])
@pytest.mark.parametrize("entry", [(G1, False), (G2, False), (G2, True), (W1, False)], ids=entry_id)
def test_instance_count(gpu, tables, hand_points, entry, m):
    """the block borders of k_batch_horner_lanes (21 instances per block), k_batch_horner_hex (10) and k_batch_reduce (m * windows lanes
    in blocks of 128); on the subgroup entry the 136-bit scalars split into three digits"""
    group, subgroup = entry
    g = bc.GROUPS[group]
    call, special = count_call(group, tables[group], hand_points, m, 0xC0 + m)
    assert call.bits() == 136 and len(call.sizes) == m and max(call.sizes) <= 4
    want = {p: co.jac_to_affine(np.concatenate([call.rows[int(call.offsets[p]) + 2], co.to_mont([1] + [0] * (g.coords // 2 - 1), g.q).reshape(-1)]), g.kind)
            for p in special}
    _, t, d = check(gpu, call, subgroup=subgroup, want=want)
    assert d[3] == (3 if subgroup else 1) and t["window_bits"] == 3 and t["windows"] == ((64 if subgroup else 136) + 3) // 3


# ---- Horner branches ----------------------------------------------------------------------------------------------------------------------
def builder_instance(name, group, c, hand, seed):
    P, R, _ = hand[group]
    pts, sc, exp = bc.build(name, group, c, P, R, bc.full_scalar(group, seed))
    return bc.pack_instance(group, pts, sc), exp


@pytest.mark.parametrize("name", bc.BUILDERS)
@pytest.mark.parametrize("group", [G1, G2, W1])
def test_horner_branches(gpu, tables, hand_points, group, name):
    """each branch in each Horner kernel (three lanes over Fq, six over Fq2, three over the 12-word field): the instance alone, inside a
    batch of ordinary instances (both c = 3), and inside a 300-point instance (c = 5, the scalars built for that window) whose other points
    cancel bucket by bucket, so that the window sums are the builder's"""
    g = bc.GROUPS[group]
    table = tables[group]
    inst3, exp = builder_instance(name, group, 3, hand_points, 0xB3)
    _, t, _ = check(gpu, bc.concat_call(group, [inst3]), want={0: exp})
    assert t["window_bits"] == 3
    ordinary = bc.mixed_call(group, table, [9, 20, 5], g.scalar_bits - 1, 0xB4)
    parts = [(ordinary.rows[int(a):int(b)], ordinary.inf[int(a):int(b)], ordinary.scalars[int(a):int(b)]) for a, b in zip(ordinary.offsets[:-1], ordinary.offsets[1:])]
    _, t, _ = check(gpu, bc.concat_call(group, [parts[0], inst3, parts[1], inst3, parts[2]]), want={1: exp, 3: exp})
    assert t["window_bits"] == 3
    inst5, exp5 = builder_instance(name, group, 5, hand_points, 0xB5)
    filler = bc.cancelling_filler(group, table, 298, g.scalar_bits - 1, 0xB6)
    big = tuple(np.concatenate([a, b]) for a, b in zip(inst5, filler))
    _, t, _ = check(gpu, bc.concat_call(group, [parts[0], big, parts[2]]), want={1: exp5})
    assert t["window_bits"] == 5 and 300 <= big[0].shape[0] <= 301


def test_horner_branches_on_the_split_path(gpu, tables, hand_points):
    """the G2 subgroup entry: 136-bit scalars split into three 64-bit digits over P, psi(P), psi^2(P) - a cancelling pair cancels in every
    image, and [P, P, -P] x [a, b, a + b] is the identity although no image's share vanishes (the digits of a + b carry)"""
    P = hand_points[G2][0]
    k = bc.scalar_of_bits(136, 0xB7)
    cancel = bc.pack_instance(G2, *bc.all_cancel(G2, 3, P, k)[:2])
    short = bc.pack_instance(G2, *bc.live_identity_short(G2, P, bc.scalar_of_bits(135, 1), bc.scalar_of_bits(135, 2))[:2])
    ordinary = bc.mixed_call(G2, tables[G2], [9], 136, 0xB8)
    one = (ordinary.rows, ordinary.inf, ordinary.scalars)
    for call in (bc.concat_call(G2, [cancel]), bc.concat_call(G2, [short]), bc.concat_call(G2, [one, cancel, short, one])):
        got, t, d = check(gpu, call, subgroup=True)
        assert d[3] == 3 and t["windows"] == (64 + 3) // 3
        assert [p for p, k_ in zip(got, call.sizes) if k_ < 9] == [None] * (len(call.sizes) - call.sizes.count(9))


# ---- GLS gates ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,max_n,split", [(136, 341, True), (136, 342, False), (252, 256, True), (252, 257, False), (100, 512, True), (100, 513, False)])
def test_gls_gates(gpu, tables, bits, max_n, split):
    """nd * max_n <= 1024 at its edge for nd = 3, 4 and 2: the last size that is split and the first that is not"""
    call = bc.mixed_call(G2, tables[G2], [max_n, 3], bits, 0x615 + max_n)
    _, t, d = check(gpu, call, subgroup=True)
    c = t["window_bits"]
    assert (d[3] > 1) == split and t["windows"] == ((64 + c) // c if split else (bits + c) // c)


# ---- k_scalar_or beyond one stride ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_g1(gpu):
    return device_table(G1, 257 * 1024, 0xBA7C0005)


@pytest.mark.parametrize("place", ["second_pass_first", "last"])
def test_scalar_or_beyond_one_stride(gpu, big_g1, place):
    """257 instances of 1024 points: k_scalar_or's 2048 x 256 lanes cover 262144 scalars per pass, so the one 136-bit scalar - the first of
    the second pass, or the very last - is seen by the loop's second iteration only; every other scalar has 20 bits"""
    m, n = 257, 1024
    tot = m * n
    assert STRIDE_POINTS == 262144 < tot
    sc = bc.random_scalars(tot, 4, 20, 0x50 + len(place))
    at = STRIDE_POINTS if place == "second_pass_first" else tot - 1
    bc.set_scalar(sc, at, (1 << 136) - 1)
    call = bc.Call(G1, big_g1, np.zeros(tot, dtype=np.uint8), sc, np.arange(0, tot + 1, n, dtype=np.uint32))
    assert bc.longest(sc[:STRIDE_POINTS]) <= 20 and call.bits() == 136
    _, t, _ = check(gpu, call)
    assert t["window_bits"] == 7 and t["windows"] == (136 + 7) // 7 and t["buckets"] == m * 20 * 64


# ---- the host form of the side path ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [G1, W1])
def test_host_form_side_path(gpu, tables, group):
    """an instance above 1024 points sends every instance of the call through the large pipeline; so does a call of empty instances; a
    call of no instance returns at once"""
    g = bc.GROUPS[group]
    call = bc.mixed_call(group, tables[group], [1025, 0, 3], g.scalar_bits - 1, 0x51DE)
    got, _, d = check(gpu, call)
    assert d == "side" and got[1] is None and got[0] is not None and got[2] is not None
    none = bc.concat_call(group, [bc.pack_instance(group, [], [])] * 3)
    got, _, d = check(gpu, none)
    assert d == "side" and got == [None, None, None]
    empty = bc.concat_call(group, [])
    out = gpu.msm_batch(group, empty.rows, empty.inf, empty.scalars, empty.offsets)
    assert out.shape == (0, 3 * g.rows // 2)


# ---- bits above the modulus -----------------------------------------------------------------------------------------------------------------
def stray_bits(group):
    return (253, 254, 255) if bc.GROUPS[group].scalar_bits == 253 else (377, 383)


def with_stray_bits(call, rows_at):
    """a copy of the call's scalars with one container bit from SCALAR_BITS up set in each of the scalars at rows_at (one bit per scalar,
    taking turns), and the same scalars with those bits cleared: what the library must compute with"""
    g = bc.GROUPS[call.group]
    clean = call.scalars.copy()
    dirty = clean.copy()
    for i, at in enumerate(rows_at):
        b = stray_bits(call.group)[i % len(stray_bits(call.group))]
        dirty[at, b // 64] |= np.uint64(1 << (b % 64))
    assert np.array_equal(bc.clear_from(dirty, g.scalar_bits), clean) and bc.longest(dirty) > g.scalar_bits >= bc.longest(clean)
    return dirty, clean


@pytest.mark.parametrize("n", [40, 130, 256, 600, 1024])
@pytest.mark.parametrize("entry", bc.ENTRIES, ids=entry_id)
def test_bits_above_the_modulus_are_ignored(gpu, tables, entry, n):
    """a scalar is read modulo 2^SCALAR_BITS, as msm_<group> and the side path of this very call read it: the container bits 253..255
    (BLS12-377) / 377..383 (BW6-761) of a few scalars are set, and the result is the oracle's on the scalars without them - one case per
    window c = 3..7 (on the subgroup entry the full-length scalars split into four digits up to 256 points)"""
    group, subgroup = entry
    g = bc.GROUPS[group]
    call = bc.mixed_call(group, tables[group], [n, 6], g.scalar_bits - 1, 0xAB0 + n)
    dirty, clean = with_stray_bits(call, [9, 10, 11, 12, n - 1, n + 2])
    _, t, d = check(gpu, bc.Call(group, call.rows, call.inf, dirty, call.offsets), subgroup=subgroup, oracle_scalars=clean)
    if not subgroup:
        assert t["window_bits"] == {40: 3, 130: 4, 256: 5, 600: 6, 1024: 7}[n]
    else:
        assert d[3] == (4 if n <= 256 else 1)


def test_stray_bit_does_not_switch_the_split_off(gpu, tables):
    """136-bit exponents with a container bit set above the modulus: the subgroup entry still splits them into three digits"""
    call = bc.mixed_call(G2, tables[G2], [40, 6], 136, 0xAB7)
    dirty, clean = with_stray_bits(call, [9, 10, 11, 45])
    _, t, d = check(gpu, bc.Call(G2, call.rows, call.inf, dirty, call.offsets), subgroup=True, oracle_scalars=clean)
    assert d[3] == 3 and t["windows"] == (64 + t["window_bits"]) // t["window_bits"]


@pytest.mark.parametrize("entry", bc.ENTRIES, ids=entry_id)
def test_batch_path_and_side_path_read_a_scalar_alike(gpu, tables, entry):
    """one call must not answer differently for an instance of 1024 points (the batched kernels) and the same instance with one
    zero-scalar point appended (1025 points: the large pipeline)"""
    group, subgroup = entry
    g = bc.GROUPS[group]
    call = bc.mixed_call(group, tables[group], [1024], g.scalar_bits - 1, 0xAB8)
    dirty, clean = with_stray_bits(call, [9, 10, 11, 1023])
    got, _, d = check(gpu, bc.Call(group, call.rows, call.inf, dirty, call.offsets), subgroup=subgroup, oracle_scalars=clean)
    longer = bc.Call(group, np.concatenate([call.rows, tables[group][1024:1025]]), np.append(call.inf, np.uint8(0)),
                     np.concatenate([dirty, np.zeros((1, g.limbs), dtype=np.uint64)]), np.array([0, 1025], dtype=np.uint32))
    side, _, d2 = check(gpu, longer, subgroup=subgroup, oracle_scalars=np.concatenate([clean, np.zeros((1, g.limbs), dtype=np.uint64)]))
    assert d != "side" and d2 == "side" and got == side and got[0] is not None
