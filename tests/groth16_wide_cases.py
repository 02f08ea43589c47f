"""Wide BLS12-377 verifying keys (up to 1024 public inputs) and the many-lane input sum: what tests/test_groth16_wide_host.py and
tests/test_groth16_wide_gpu.py share on top of tests/groth16_verify377_cases.py (no GPU import at module level).

The rules are RESTATED here, not read from the library: the window rule with its borders, the lane rule with its two constants, and the lane
that owns an input.  Lane l of L sums the inputs j = l, l + L, ..; lane 0 starts from gamma_abc[0]; the partials are folded in rounds of
stride L/2 .. 1, lane l < s taking the partial of lane l + s.  With the key's scalars u_j known (gamma_abc[j] = u_j G1) an input vector can
be chosen so that two partials are equal (the fold's doubling branch), opposite (cancelling) or the identity."""
import copy
from oracle.py import ecc
from tests import groth16_verify377_cases as gc

R = gc.R
WIDE_MAX = 1024
LANES = (1, 2, 4, 8, 16, 32, 64, 128, 256)
# the last input count of each window width, 10 .. 4 bits (128-byte entries, 64 MiB)
BORDERS = {10: 39, 9: 70, 8: 128, 7: 221, 6: 381, 5: 642, 4: 1024}
# csrc/groth16_verify.h g16_pick_lanes
NARROW_MAX, INPUTS_PER_LANE, FILL_LANES, MAX_LANES = 64, 1, 1 << 16, 256


def window_bits_wide(n_in):
    """the widest of 10 .. 4 bits whose tables fit 64 MiB, or None past the limit of the wide loaders"""
    return None if n_in > WIDE_MAX else gc.window_bits(n_in)


def pick_lanes(n_in, m):
    """min(256, smallest power of two >= n_in / INPUTS_PER_LANE, largest power of two <= FILL_LANES / m), at least 1; 1 up to 64 inputs"""
    if n_in <= NARROW_MAX:
        return 1
    work = 1
    while work < MAX_LANES and work * INPUTS_PER_LANE < n_in:
        work *= 2
    fill = MAX_LANES
    while fill > 1 and fill * m > FILL_LANES:
        fill //= 2
    return min(work, fill)


def sub_key(key, n_in):
    """the key of the first n_in inputs of `key`: the same alpha .. delta, a prefix of gamma_abc"""
    assert n_in <= key.n_in
    k = copy.copy(key)
    k.n_in, k.u, k.abc = n_in, key.u[:n_in + 1], key.abc[:n_in + 1]
    return k


def _div(a, b):
    return a * pow(b, -1, R) % R


def fold_branch_inputs(key, L):
    """{name: input vector} for a key of at least max(L, 3) inputs, every input not named zero.  u[j + 1] is the scalar of input j."""
    u, n, h = key.u, key.n_in, L // 2
    assert L >= 2 and n >= max(L, 3)
    out = {}

    def vec(**at):
        x = [0] * n
        for j, v in at.items():
            x[int(j[1:])] = v % R
        return x

    for sign, name in ((1, "double"), (-1, "cancel")):
        if L >= 4:
            # lanes 1 and 1 + L/2 meet in the first round: x_1 u_2 = +- x_(1+h) u_(2+h)
            out[name + "_first_round"] = vec(j1=1, **{"j%d" % (1 + h): sign * _div(u[2], u[2 + h])})
            # lane 0 (gamma_abc[0], and lane 2's partial from an earlier round) meets lane 1 in the last round
            out[name + "_last_round"] = vec(j2=1, j1=sign * _div(u[0] + u[3], u[2]))
        # lane 0's partial, gamma_abc[0] included, against its first partner, lane L/2 (at L = 2 the first round is the last)
        out[name + "_lane0"] = vec(**{"j%d" % h: sign * _div(u[0], u[1 + h])})
    out["only_lane0"] = vec()                                            # every partial but lane 0's is the identity
    out["only_last_lane"] = vec(j0=-_div(u[0], u[1]), **{"j%d" % (L - 1): 5})   # lane 0 cancels to the identity; lane L - 1 alone is not
    return out


def bad_input_rows(n_in, L, rng):
    """[(inputs, index of the input that is not below r)] : r, r + 1, 2^256 - 1 at the first input, the last, and one of another lane than 0"""
    spots = sorted({0, n_in - 1} | ({1} if n_in >= 2 and L >= 2 else set()))
    rows = []
    for j in spots:
        for v in (R, R + 1, (1 << 256) - 1):
            x = [ecc.random_scalar(rng, R) for _ in range(n_in)]
            x[j] = v
            rows.append((x, j))
    return rows
