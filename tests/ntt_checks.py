"""Whole-output checks of a number-theoretic transform and of the Groth16 witness map that need no O(n log n) reference.

Plain Python integers modulo a prime p; nothing here imports the library under test or the C++ oracle.

Random-evaluation identity of a transform.  For X = NTT_w(x), X_j = sum_i x_i w^(i j), of size n (w^n = 1) and any r with r^n != 1:

    sum_j r^j X_j  =  sum_i x_i sum_j (r w^i)^j  =  (r^n - 1) * sum_i x_i / (r w^i - 1)        (mod p)

The left side is the polynomial with coefficients X evaluated at r, so two different output vectors agree on it for at most n - 1
values of r: a wrong output escapes a random r with probability below n / p.  Every input and every output takes part.  The variants
of the library's entry point are the same identity with other arguments:

    X_j = s * post^j * sum_i (x_i pre^i) w^(i j)    =>    sum_j r^j X_j = s * (rho^n - 1) * sum_i x_i pre^i / (rho w^i - 1),  rho = r * post

Both sides are linear in (x, X): the identity holds for Montgomery residues (x R, X R) exactly when it holds for the values, so callers
may pass the limbs of a Montgomery array as integers without converting them.

Quotient identity of the witness map.  For evaluations a, b, c over the domain {w^i} and h = witness_map(a, b, c) with c_i = a_i b_i:

    h(tau) * (tau^n - 1)  =  A(tau) B(tau) - C(tau),      A(tau) = (tau^n - 1) / n * sum_i a_i w^i / (tau - w^i)   (barycentric form)

and deg h <= n - 2, so h[n - 1] = 0.

Both checks are sums over the positions, so they split into ranges (`start`): a caller may compute the partial sums of ranges of a
large array in parallel and add them up."""


def batch_inverse(vals, p):
    """[1 / v mod p for v in vals] with one modular inversion (Montgomery's trick).  A zero among vals is an error."""
    n = len(vals)
    if n == 0:
        return []
    prefix = [0] * n
    acc = 1
    for i, v in enumerate(vals):
        if v % p == 0:
            raise ZeroDivisionError("batch_inverse: element %d is zero" % i)
        prefix[i] = acc
        acc = acc * v % p
    inv = pow(acc, -1, p)
    out = [0] * n
    for i in range(n - 1, -1, -1):
        out[i] = inv * prefix[i] % p
        inv = inv * vals[i] % p
    return out


def output_sum(X, r, p, start=0):
    """sum_j r^(start + j) X[j]  (Horner over the range, then the range's offset)."""
    acc = 0
    for v in reversed(X):
        acc = (acc * r + v) % p
    return acc * pow(r, start, p) % p


def input_sum(x, w, rho, p, pre=None, start=0):
    """sum_i x[i] pre^(start + i) / (rho w^(start + i) - 1) over the range (pre = None: no coset factor)."""
    n = len(x)
    d = [0] * n
    t = rho * pow(w, start, p) % p
    for i in range(n):
        d[i] = (t - 1) % p
        t = t * w % p
    inv = batch_inverse(d, p)
    if pre is None:
        return sum(a * b for a, b in zip(x, inv)) % p
    acc = 0
    g = pow(pre, start, p)
    for a, b in zip(x, inv):
        acc += a * g % p * b
        g = g * pre % p
    return acc % p


def identity_rhs(in_sum, n, r, p, post=None, scale=None):
    """the right-hand side from the (summed) input_sum of all ranges: s * (rho^n - 1) * in_sum"""
    rho = r * (post if post is not None else 1) % p
    return (pow(rho, n, p) - 1) * in_sum % p * (scale if scale is not None else 1) % p


def rho_of(r, p, post=None):
    return r * (post if post is not None else 1) % p


def ntt_identity_holds(x, X, w, p, r, pre=None, post=None, scale=None):
    """True iff X passes the random-evaluation identity at r as  X_j = scale * post^j * sum_i x_i pre^i w^(i j)."""
    n = len(x)
    if len(X) != n or pow(w, n, p) != 1:
        return False
    lhs = output_sum(X, r, p)
    rhs = identity_rhs(input_sum(x, w, rho_of(r, p, post), p, pre), n, r, p, post, scale)
    return lhs == rhs


def bary_sums(a, b, c, w, tau, p, start=0):
    """(sum_i a[i] w^i / (tau - w^i), the same for b, for c) over the range starting at position `start`."""
    n = len(a)
    assert len(b) == n and len(c) == n
    pw = [0] * n
    d = [0] * n
    t = pow(w, start, p)
    for i in range(n):
        pw[i] = t
        d[i] = (tau - t) % p
        t = t * w % p
    inv = batch_inverse(d, p)
    k = [u * v % p for u, v in zip(pw, inv)]
    return tuple(sum(u * v for u, v in zip(vec, k)) % p for vec in (a, b, c))


def quotient_identity_from_sums(h_at_tau, sums, n, tau, p, mont_radix=None):
    """h(tau) (tau^n - 1) == A(tau) B(tau) - C(tau) from h(tau) and the summed bary_sums.  With mont_radix = R all of a, b, c, h were
    Montgomery residues (value * R): the product of two residues carries one R too many, every other term is linear."""
    z = (pow(tau, n, p) - 1) % p
    f = z * pow(n, -1, p) % p
    A, B, C = (f * s % p for s in sums)
    ab = A * B % p
    if mont_radix is not None:
        ab = ab * pow(mont_radix, -1, p) % p
    return h_at_tau * z % p == (ab - C) % p


def quotient_identity_holds(a, b, c, h, w, p, tau, mont_radix=None):
    """True iff h passes the quotient identity at tau for the evaluations a, b, c over the domain generated by w, and h[n - 1] == 0."""
    n = len(a)
    if len(h) != n or pow(w, n, p) != 1 or h[n - 1] % p != 0:
        return False
    return quotient_identity_from_sums(output_sum(h, tau, p), bary_sums(a, b, c, w, tau, p), n, tau, p, mont_radix)
