"""CPU (-m "not gpu"): the case list of tests/subgroup_cases.py is what it claims - every expected status is proved from the ROW with the
oracle (the canonical range, the curve equation, a full mul(P, r)) - and the number facts behind csrc/wire761.h w761_in_subgroup_endo."""
import re
import os
import numpy as np
import pytest
from oracle.py import ecc
import subgroup_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def proved_status(g, row, flag, level):
    if flag:
        return 1
    if any(v >= g.q for v in g.components(row)):
        return 2
    P = g.point_of(row)
    if not g.E.on_curve(P):
        return 2
    if level == 2 and g.E.mul(P, g.r) is not None:
        return 3
    return 0


@pytest.mark.parametrize("name", sc.GROUPS)
def test_every_expected_status_is_the_oracles(name):
    g, cs = sc.group(name), sc.cases(name)
    for level in (1, 2):
        got = [proved_status(g, cs.xy[i], cs.inf[i], level) for i in range(cs.n)]
        assert got == cs.want[level].tolist(), [(cs.labels[i], got[i], int(cs.want[level][i])) for i in range(cs.n) if got[i] != cs.want[level][i]]
    # every status occurs, and at level 2 both verdicts on finite curve points
    assert set(cs.want[1].tolist()) == {0, 1, 2} and set(cs.want[2].tolist()) == {0, 1, 2, 3}
    assert cs.first_bad(1) > 0 and cs.first_bad(2) > 0 and cs.first_bad(2) <= cs.first_bad(1) < cs.n


@pytest.mark.parametrize("name", ["bw6_761_g1", "bw6_761_g2"])
def test_mandatory_low_order_cases_are_present(name):
    labels = [label for label, _, _ in sc.on_curve_cases(name)]
    must = ["(1, 0) order 2", "(beta, 0) order 2", "(beta^2, 0) order 2", "G + (1, 0) order 2"] if name == "bw6_761_g1" else \
        ["(0, 2) order 3", "(0, -2) order 3", "G + (0, 2)", "G - (0, 2)", "order 13", "G + order 13"]
    for m in must:
        assert m in labels, m
    g = sc.group(name)
    for label, P, member in sc.on_curve_cases(name):
        assert g.E.on_curve(P) and (g.E.mul(P, g.r) is None) == member, label


def test_norm_and_eigenvalues():
    x, r, q = ecc.X, ecc.R761, ecc.Q761
    a, b = sc.ENDO_A, sc.ENDO_B
    assert 3 * a == 2 * x ** 3 - 2 * x ** 2 - x + 1 and 3 * b == x ** 3 - x ** 2 - 2 * x - 1
    assert a * a - a * b + b * b == r                                     # the endomorphism a + b phi has degree r exactly
    assert a.bit_length() == 189 and b.bit_length() == 188
    assert sc.SHORT_A ** 2 - sc.SHORT_A * sc.SHORT_B + sc.SHORT_B ** 2 == 3 * r
    b1, b2 = sc.betas()
    assert b1 != b2 and b1 != 1 and b2 != 1 and pow(b1, 3, q) == 1 and b2 == b1 * b1 % q
    lam = (-a * pow(b, -1, r)) % r                                        # the eigenvalue with a + b lambda = 0 (mod r)
    assert (lam * lam + lam + 1) % r == 0
    for name, beta, other in (("bw6_761_g1", b1, b2), ("bw6_761_g2", b2, b1)):
        g = sc.group(name)
        G = sc.subgroup_points(name)[1]
        assert g.E.mul(G, lam) == sc.phi(beta, G)                         # this group's beta acts on the subgroup as lambda: a + b lambda = 0
        assert g.E.mul(G, lam) != sc.phi(other, G)                        # ... and the other root does not: the two groups need different betas
        assert sc.endo_image(g.E, beta, G) is None and sc.endo_image(g.E, other, G) is not None


def test_betas_are_the_headers():
    """the two constants of csrc/wire761.h (canonical little-endian words) are g^((q-1)/3) and its square"""
    txt = open(os.path.join(ROOT, "celo-bls-snark-rs_amd", "csrc", "wire761.h")).read()
    for tag, want in zip(("BETA_G1", "BETA_G2"), sc.betas()):
        m = re.search(r"%s\[12\] = \{(.*?)\}" % tag, txt, re.S)
        words = [int(w, 16) for w in re.findall(r"0x[0-9a-fA-F]+", m.group(1))]
        assert len(words) == 12 and sum(w << (64 * i) for i, w in enumerate(words)) == want, tag


def test_cofactors():
    h1, h2 = sc.cofactor_761("bw6_761_g1"), sc.cofactor_761("bw6_761_g2")
    assert h1 % 3 != 0 and h1 % 2 == 0
    assert h2 % 3 == 0 and h2 % 13 == 0


def test_the_norm_3r_vector_accepts_points_outside_g2():
    """Why (x + 1, x^3 - x^2 + 1) is not used: T = (0, 2) has order 3 and phi(T) = T, and T, G + T, G - T all pass that test on G2; the
    norm-r vector rejects all three."""
    g = sc.group("bw6_761_g2")
    E, G, beta = g.E, g.gen, sc.betas()[1]
    T = (0, 2)
    assert E.on_curve(T) and E.mul(T, 3) is None and sc.phi(beta, T) == T
    assert sc.endo_image(E, beta, G, sc.SHORT_A, sc.SHORT_B) is None      # it does hold on the subgroup
    for P in (T, E.add(G, T), E.add(G, E.neg(T))):
        assert E.mul(P, g.r) is not None
        assert sc.endo_image(E, beta, P, sc.SHORT_A, sc.SHORT_B) is None   # accepted, wrongly
        assert sc.endo_image(E, beta, P) is not None                      # rejected by a + b phi


@pytest.mark.parametrize("name", ["bw6_761_g1", "bw6_761_g2"])
def test_endomorphism_test_equals_membership_on_the_case_list(name):
    g = sc.group(name)
    beta = sc.betas()[0 if name == "bw6_761_g1" else 1]
    for label, P, member in sc.on_curve_cases(name):
        assert (sc.endo_image(g.E, beta, P) is None) == member, label
