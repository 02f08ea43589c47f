"""Test-side restatement of ark-groth16 0.1 parameter generation after synthesis (generator.rs generate_parameters, r1cs_to_qap.rs
instance_map_with_evaluation / witness_map), shared by tests/test_groth16_setup_host.py and the GPU setup tests.

The ark-groth16 0.1 source is not vendored with the reference; three parts below rest on its recalled structure, not on a reading of it:
  - instance_map_with_evaluation adds, for every instance variable i (the one included), L_(num_constraints + i)(tau) to a_i - the
    "input consistency" rows the witness map fills with a[num_constraints + i] = z_i;
  - the evaluation domain is the smallest power of two >= num_constraints + num_inputs;
  - h_query has domain size - 1 rows: zt delta^-1 tau^i for i < domain size - 1.
None of them can be pinned against a reference vector (the reference holds no proving key).  What a proof depends on is pinned instead by
the round trips: a key made from these scalars must make the prover's proofs pass the Groth16 pairing check, and reject a wrong input.

Circuits are R1CS given as three lists (one per matrix) of constraints, each a dict {variable index: coefficient}; variables are ordered as
ark-relations orders them: the instance variables first (index 0 is the constant one), then the witness."""
from oracle.py import ecc
from oracle.py import ntt as ontt
from oracle import cpu_oracle as co

FIELDS = {"bw6_761": ecc.Q377, "bls12_377": ecc.R377}      # the scalar field of each curve


def root_of_unity(curve, log_n):
    return ontt.root_of_unity(log_n) if curve == "bw6_761" else ontt.root_of_unity_fr377(log_n)


def coset_generator(p):
    g = 2
    while pow(g, (p - 1) // 2, p) != p - 1:
        g += 1
    return g


def domain_log(num_constraints, num_inputs):
    n, log_n = 1, 0
    while n < num_constraints + num_inputs:
        n, log_n = 2 * n, log_n + 1
    return log_n


def lagrange_at(tau, log_n, omega, p):
    """L_i(tau) for the domain {omega^i}: Z(tau) / n * omega^i / (tau - omega^i) (tau outside the domain)"""
    n = 1 << log_n
    zt = (pow(tau, n, p) - 1) % p
    c = zt * pow(n, -1, p) % p
    out, w = [], 1
    for _ in range(n):
        out.append(c * w % p * pow((tau - w) % p, -1, p) % p)
        w = w * omega % p
    return out


def qap_at(A, B, C, n_vars, num_inputs, tau, log_n, omega, p):
    """instance_map_with_evaluation: (a, b, c) lists of n_vars field elements and zt = Z(tau)"""
    L = lagrange_at(tau, log_n, omega, p)
    a, b, c = [0] * n_vars, [0] * n_vars, [0] * n_vars
    for M, out in ((A, a), (B, b), (C, c)):
        for j, row in enumerate(M):
            for v, k in row.items():
                out[v] = (out[v] + k * L[j]) % p
    m = len(A)
    for i in range(num_inputs):
        a[i] = (a[i] + L[m + i]) % p
    zt = (pow(tau, 1 << log_n, p) - 1) % p
    return a, b, c, zt


def setup_scalars(a, b, c, num_inputs, zt, tau, n_h, alpha, beta, gamma, delta, p):
    """the scalars of every key row (generate_parameters), as python ints: {section: scalar or list}"""
    gi, di = pow(gamma, -1, p), pow(delta, -1, p)
    lc = [(beta * x + alpha * y + z) % p for x, y, z in zip(a, b, c)]
    return {"alpha_g1": alpha, "beta_g1": beta, "delta_g1": delta, "beta_g2": beta, "gamma_g2": gamma, "delta_g2": delta,
            "gamma_abc_g1": [v * gi % p for v in lc[:num_inputs]], "l_query": [v * di % p for v in lc[num_inputs:]],
            "a_query": list(a), "b_g1_query": list(b), "b_g2_query": list(b),
            "h_query": [zt * di % p * pow(tau, i, p) % p for i in range(n_h)]}


def witness_rows(A, B, C, z, num_inputs, log_n, p):
    """the witness map's inputs: (A z), (B z), (C z) over the domain rows, the input-consistency rows a[m + i] = z_i"""
    n = 1 << log_n
    out = []
    for M in (A, B, C):
        v = [0] * n
        for j, row in enumerate(M):
            v[j] = sum(k * z[i] for i, k in row.items()) % p
        out.append(v)
    m = len(A)
    for i in range(num_inputs):
        out[0][m + i] = z[i] % p
    return out


# ---- circuits
def toy_circuit():
    """x^3 + x + 5 = out with one public input (out): variables [one, out | x, x^2, x^3, x^3 + x]"""
    A = [{2: 1}, {3: 1}, {4: 1, 2: 1}, {5: 1, 0: 5}]
    B = [{2: 1}, {2: 1}, {0: 1}, {0: 1}]
    C = [{3: 1}, {4: 1}, {5: 1}, {1: 1}]
    return A, B, C, 6, 2


def toy_witness(x, p):
    return [1, (x ** 3 + x + 5) % p, x % p, x * x % p, x ** 3 % p, (x ** 3 + x) % p]


def squaring_chain(m):
    """m constraints x_k * x_k = x_(k+1), the last one's output the public input: variables [one, out | x_0 .. x_(m-1)]"""
    A, B, C = [], [], []
    for k in range(m):
        v = 2 + k
        A.append({v: 1}); B.append({v: 1}); C.append({(v + 1) if k + 1 < m else 1: 1})
    return A, B, C, m + 2, 2


def squaring_witness(m, x0, p):
    xs = [x0 % p]
    for _ in range(m - 1):
        xs.append(xs[-1] * xs[-1] % p)
    return [1, xs[-1] * xs[-1] % p] + xs


def mont(vals, p):
    return co.to_mont(vals, p)


# ---- key rows and the pairing check
CURVES = {   # (scalar field, G1 curve, G2 curve, G1 coordinate field, u64 per scalar, u64 per G1 row)
    "bw6_761": (ecc.Q377, ecc.E1_761, ecc.E2_761, ecc.Q761, 6, 24),
    "bls12_377": (ecc.R377, ecc.E1_377, ecc.E2_377, ecc.Q377, 4, 12),
}


def generators(curve):
    """the G1 / G2 generators the tests hand to the setup: BW6-761 has none in the oracle, so the reference verifying key's alpha_g1 and
    beta_g2 serve (any element of a prime-order group other than the identity generates it)"""
    if curve == "bw6_761":
        import bw6_serial as bs
        vk = bs.reference_vk()
        return ecc.deser_point(ecc.E1_761, vk[0:96]), ecc.deser_point(ecc.E2_761, vk[96:192])
    return ecc.G1_377, ecc.G2_377


def pack(curve, group, pts):
    """python affine points -> (rows, inf); group 1 or 2"""
    if curve == "bw6_761":
        return co.pack_761(pts)
    return co.pack_g1_377(pts) if group == 1 else co.pack_g2_377(pts)


def ark_zero_fix(curve, rows, inf):
    """zero rows of the identity -> arkworks' GroupAffine::zero() coordinates (0, 1)"""
    rows = rows.copy()
    one = co.to_mont([1], ecc.Q761 if curve == "bw6_761" else ecc.Q377)[0]
    half = rows.shape[1] // 2
    for i in range(rows.shape[0]):
        if inf[i]:
            rows[i, :] = 0
            rows[i, half:half + one.size] = one
    return rows


def to_points(curve, group, rows):
    """affine rows (arkworks identity (0, 1) or zero rows -> None) -> python points"""
    import numpy as np
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    rows = rows.reshape(-1, rows.shape[-1])
    q = ecc.Q761 if curve == "bw6_761" else ecc.Q377
    out = []
    for r in rows:
        v = co.from_mont(r.reshape(-1, 12 if curve == "bw6_761" else 6), q)
        if curve == "bls12_377" and group == 2:
            P = ((v[0], v[1]), (v[2], v[3]))
            out.append(None if P[0] == (0, 0) and P[1] in ((0, 0), (1, 0)) else P)
        else:
            out.append(None if v[0] == 0 and v[1] in (0, 1) else (v[0], v[1]))
    return out


def split_rows(curve, g1, g2, n_vars, n_inputs, n_h):
    """the setup's two row lists (G1 [alpha, beta, delta, gamma_abc, a, b, h, l], G2 [beta, gamma, delta, b]) -> the layout of
    ffi.groth16_setup: {"vk": {...}, "rows": {...}}"""
    o = 3
    abc = g1[o:o + n_inputs]; o += n_inputs
    a = g1[o:o + n_vars]; o += n_vars
    b = g1[o:o + n_vars]; o += n_vars
    h = g1[o:o + n_h]; o += n_h
    l_ = g1[o:]
    vk = {"alpha_g1": g1[0], "beta_g2": g2[0], "gamma_g2": g2[1], "delta_g2": g2[2], "gamma_abc_g1": abc}
    rows = {"beta_g1": g1[1], "delta_g1": g1[2], "a_query": a, "b_g1_query": b, "b_g2_query": g2[3:], "h_query": h, "l_query": l_}
    return {"vk": vk, "rows": rows}


def scalar_lists(s, n_vars, n_inputs):
    """setup_scalars' dict -> the two lists in kernel order"""
    g1 = [s["alpha_g1"], s["beta_g1"], s["delta_g1"]] + s["gamma_abc_g1"] + s["a_query"] + s["b_g1_query"] + s["h_query"] + s["l_query"]
    g2 = [s["beta_g2"], s["gamma_g2"], s["delta_g2"]] + s["b_g2_query"]
    return g1, g2


def pairing_inputs(curve, vk, proof, public):
    """the four pairs (A, B), (-alpha, beta), (-vk_x, gamma), (-C, delta) of the Groth16 check e(A, B) = e(alpha, beta) e(vk_x, gamma)
    e(C, delta); vk: rows as in split_rows; proof: python affine points (A, B, C); public: z_0 .. z_(n_inputs - 1) (z_0 = 1).
    Returns (g1 rows, inf1, g2 rows, inf2)."""
    _, E1, _, _, _, _ = CURVES[curve]
    abc = to_points(curve, 1, vk["gamma_abc_g1"])
    vkx = None
    for z, P in zip(public, abc):
        vkx = E1.add(vkx, E1.mul(P, z) if P is not None and z else None)
    alpha = to_points(curve, 1, vk["alpha_g1"])[0]
    A, B, Cp = proof
    g1 = [A, E1.neg(alpha), E1.neg(vkx) if vkx else None, E1.neg(Cp) if Cp else None]
    g2 = [B] + [to_points(curve, 2, vk[k])[0] for k in ("beta_g2", "gamma_g2", "delta_g2")]
    x1, i1 = pack(curve, 1, g1)
    x2, i2 = pack(curve, 2, g2)
    return x1, i1, x2, i2


# ---- the fixed-base tests' groups and scalars
# (host twin group id, curve, G1 or G2, u64 per scalar, u64 per row)
GROUPS = {"bls12_377_g1": (0, "bls12_377", 1, 4, 12), "bls12_377_g2": (1, "bls12_377", 2, 4, 24),
          "bw6_761_g1": (2, "bw6_761", 1, 6, 24), "bw6_761_g2": (2, "bw6_761", 2, 6, 24)}


def edge_scalars(r, bits, c, rng):
    """0, 1, 2, r - 1, (r - 1) / 2, digits at every window boundary (2^(c w) and its neighbours, the largest positive digit 2^(c-1) and the
    first negative one 2^(c-1) + 1 in window w), random values"""
    s = [0, 1, 2, r - 1, (r - 1) // 2]
    for w in range(0, bits // c + 1):
        for v in (1 << (c * w), (1 << (c * w)) - 1, (1 << (c - 1)) << (c * w), ((1 << (c - 1)) + 1) << (c * w)):
            if v < r:
                s.append(v)
    s += [rng.randrange(r) for _ in range(6)]
    return s
