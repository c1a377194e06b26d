"""Plain-Python oracle of the evaluation-form polynomial call and the KZG layer
(msm_fr_eval_quotient, msm_kzg_*): integers on fr_inputs (Fr), enc_inputs (curve
points and their bytes) and mult_inputs.smul (scalar multiplication).

The setup is INSECURE on purpose: tau is known, so a commitment is [f(tau)]G1 and a
proof [(f(tau) - y) / (tau - z)]G1 -- neither uses the evaluation-form quotient, so
the expected values do not rest on the formulas under test (eval_quot below, which
the CPU tests check against Horner and synthetic division).
tests/golden/kzg.json pins it to the reference.  Test infrastructure only."""
import enc_inputs as ei
import fr_inputs as fi
import mult_inputs as mi

R = fi.R
TAU = 0x1d2c3b4a59687766554433221100ffeeddccbbaa99887766554433221100f1e3 % R  # the golden's
SEED = 4844


def inv0(x):
    """the MSM_FR_INV convention: the inverse of zero is zero"""
    return pow(x % R, R - 2, R)


def brev(i, bits):
    return int(format(i, f"0{bits}b")[::-1], 2) if bits else 0


def domain(log_n, bitrev=False):
    w, n = fi.root(log_n), 1 << log_n
    nat = [1] * n
    for i in range(1, n):
        nat[i] = nat[i - 1] * w % R
    return [nat[brev(i, log_n)] for i in range(n)] if bitrev else nat


def eval_quot(f, z, log_n, bitrev=False, dom=None):
    """(y, q): y = f(z) and the values of (f - y) / (X - z) on the domain, by the formulas
    of include/msm_mi355x.h"""
    n = 1 << log_n
    D = dom if dom is not None else domain(log_n, bitrev)
    d = [inv0(z - x) for x in D]
    S = sum(a * x * di for a, x, di in zip(f, D, d)) % R
    T = sum(x * di for x, di in zip(D, d)) % R
    m = [i for i, x in enumerate(D) if x == z % R]
    y = f[m[0]] if m else (pow(z, n, R) - 1) * inv0(n) * S % R
    q = [(y - a) * di % R for a, di in zip(f, d)]
    if m:
        q[m[0]] = inv0(z) * (S - y * T) % R
    return y, q


def horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def synthetic_quotient(coeffs, z, y):
    """the coefficients of (p - y) / (X - z), and the remainder (0 when y = p(z))"""
    n = len(coeffs)
    c = list(coeffs)
    c[0] = (c[0] - y) % R
    q, carry = [0] * n, 0
    for k in range(n - 1, 0, -1):
        carry = (c[k] + carry * z) % R
        q[k - 1] = carry
    return q, (c[0] + carry * z) % R


def lagrange_at(tau, log_n, bitrev=False, dom=None):
    """l_i(tau) for the Lagrange basis of the domain: (tau^n - 1) x_i / (n (tau - x_i)); tau
    outside the domain"""
    n = 1 << log_n
    D = dom if dom is not None else domain(log_n, bitrev)
    k = (pow(tau, n, R) - 1) * inv0(n) % R
    assert k != 0, "tau lies in the domain"
    return [k * x % R * inv0(tau - x) % R for x in D]


def eval_at(f, lag):
    """f(tau) of an evaluation-form polynomial from the l_i(tau)"""
    return sum(a * l for a, l in zip(f, lag)) % R


# ---- the group side ----
def g1(k):
    return mi.smul(1, ei.GEN[1], k % R)


def g2(k):
    return mi.smul(2, ei.GEN[2], k % R)


def srs_scalars(tau, log_n, bitrev=False):
    return lagrange_at(tau, log_n, bitrev)


def srs_points(tau, log_n, bitrev=False):
    return [g1(l) for l in lagrange_at(tau, log_n, bitrev)]


def commit_scalar(f, lag):
    return eval_at(f, lag)


def proof_scalar(f, z, lag, tau, log_n, bitrev=False, dom=None):
    """(y, (f(tau) - y) / (tau - z)) with y from eval_quot's first half only (Horner-checked
    in the CPU tests)"""
    y, _ = eval_quot(f, z, log_n, bitrev, dom)
    return y, (eval_at(f, lag) - y) * inv0(tau - z) % R


def p1_bytes(pt):
    return ei.affine_bytes(1, pt)


def p2_bytes(pt):
    return ei.affine_bytes(2, pt)


def compressed(g, pt):
    return ei.encode_point(g, pt, True)


# ---- the golden's inputs (n = 16, natural order) ----
GOLDEN_LOG_N = 4


def golden_polys():
    n = 1 << GOLDEN_LOG_N
    vals = fi.rand_values(3 * n, SEED)
    return [vals[j * n:(j + 1) * n] for j in range(3)]


def golden_points():
    """per polynomial: random, 0, a domain point, the last domain point"""
    D = domain(GOLDEN_LOG_N)
    rnd = fi.rand_values(3, SEED + 1)
    return [[rnd[j], 0, D[5 + j], D[-1]] for j in range(3)]
