"""Inputs and a plain-integer model of the bulk pairings (tests/test_pairing_host.py,
tests/test_gpu_pairing.py, tests/golden/make_pairing_golden.py).

The model: the tower Fp2 = Fp[u]/(u^2 + 1), Fp6 = Fp2[v]/(v^3 - (1 + u)),
Fp12 = Fp6[w]/(w^2 - v); the Miller loop over |z| = 0xd201000000010000 with the
line functions of the reference (Jacobian doubling dbl-2009-alnr and mixed
addition madd-2007-bl with the lines of eprint 2010/354, the factors -2 x_P and
2 y_P applied to the line); the reference's final exponentiation chain; Fp12 to
and from blst's bytes.  An Fp12 value is a list of six Fp2 = (c0, c1), in blst's
order: [a00, a01, a02, a10, a11, a12] for (a00 + a01 v + a02 v^2) + (a10 + ..) w.

Inputs: 24 pairs ([a_i] g1, [b_i] g2) with seeded scalars, the generators, and
the pairs with infinity on either side and on both.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import enc_inputs as ei  # noqa: E402
import mult_inputs as mi  # noqa: E402
import pairing_constants as pc  # noqa: E402
from jac_inputs import fnv  # noqa: E402,F401

P = ei.P
R = ei.R
Z_ABS = 0xd201000000010000
FP12_BYTES = 576
XI = (1, 1)


# ------------------------------------------------------------------ Fp2 ----
def f2_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2_neg(a):
    return (-a[0] % P, -a[1] % P)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_sqr(a):
    return f2_mul(a, a)


def f2_scale(a, k):
    return (a[0] * k % P, a[1] * k % P)


def f2_conj(a):
    return (a[0], -a[1] % P)


def f2_inv(a):
    n = pow((a[0] * a[0] + a[1] * a[1]) % P, -1, P)
    return (a[0] * n % P, -a[1] * n % P)


def f2_xi(a):
    """a (1 + u)"""
    return ((a[0] - a[1]) % P, (a[0] + a[1]) % P)


F2_ZERO, F2_ONE = (0, 0), (1, 0)


# ------------------------------------------------------------------ Fp6 ----
def f6_add(a, b):
    return [f2_add(x, y) for x, y in zip(a, b)]


def f6_sub(a, b):
    return [f2_sub(x, y) for x, y in zip(a, b)]


def f6_neg(a):
    return [f2_neg(x) for x in a]


def f6_mul(a, b):
    c = [F2_ZERO] * 5
    for i in range(3):
        for j in range(3):
            c[i + j] = f2_add(c[i + j], f2_mul(a[i], b[j]))
    return [f2_add(c[0], f2_xi(c[3])), f2_add(c[1], f2_xi(c[4])), c[2]]


def f6_mul_v(a):
    return [f2_xi(a[2]), a[0], a[1]]


def f6_inv(a):
    c0 = f2_sub(f2_sqr(a[0]), f2_xi(f2_mul(a[1], a[2])))
    c1 = f2_sub(f2_xi(f2_sqr(a[2])), f2_mul(a[0], a[1]))
    c2 = f2_sub(f2_sqr(a[1]), f2_mul(a[0], a[2]))
    t = f2_add(f2_xi(f2_add(f2_mul(c1, a[2]), f2_mul(c2, a[1]))), f2_mul(c0, a[0]))
    ti = f2_inv(t)
    return [f2_mul(c0, ti), f2_mul(c1, ti), f2_mul(c2, ti)]


# ----------------------------------------------------------------- Fp12 ----
F12_ONE = [F2_ONE] + [F2_ZERO] * 5


def f12_mul(a, b):
    a0, a1, b0, b1 = a[:3], a[3:], b[:3], b[3:]
    t0, t1 = f6_mul(a0, b0), f6_mul(a1, b1)
    c1 = f6_sub(f6_sub(f6_mul(f6_add(a0, a1), f6_add(b0, b1)), t0), t1)
    return f6_add(t0, f6_mul_v(t1)) + c1


def f12_sqr(a):
    return f12_mul(a, a)


def f12_conj(a):
    return a[:3] + f6_neg(a[3:])


def f12_inv(a):
    a0, a1 = a[:3], a[3:]
    t = f6_inv(f6_sub(f6_mul(a0, a0), f6_mul_v(f6_mul(a1, a1))))
    return f6_mul(a0, t) + f6_neg(f6_mul(a1, t))


def f12_frob(a, k):
    return [f2_mul(f2_conj(c) if k & 1 else c, pc.FROB[k][j]) for j, c in enumerate(a)]


def f12_pow(a, e):
    r = F12_ONE
    for bit in bin(e)[2:]:
        r = f12_sqr(r)
        if bit == "1":
            r = f12_mul(r, a)
    return r


def f12_is_one(a):
    return [tuple(c) for c in a] == F12_ONE


def f12_mul_sparse(a, x, y, z):
    """a (x + y v + z v w): the line's three coefficients at positions 0, 1 and 4"""
    return f12_mul(a, [x, y, F2_ZERO, F2_ZERO, z, F2_ZERO])


def fp12_bytes(a):
    return b"".join(ei.mont_bytes(2, c) for c in a)


def fp12_from_bytes(raw):
    assert len(raw) == FP12_BYTES
    return [ei.from_mont(2, raw[96 * j:96 * (j + 1)]) for j in range(6)]


def fp12_one():
    return fp12_bytes(F12_ONE)


# ---------------------------------------------------------- Miller loop ----
def line_dbl(T):
    """T = (X, Y, Z) Jacobian over Fp2 -> (2T, line); the line is (l0, l1, l2) before the factors of P"""
    X, Y, Zc = T
    A, B, ZZ = f2_sqr(X), f2_sqr(Y), f2_sqr(Zc)
    C = f2_sqr(B)
    D = f2_sub(f2_sub(f2_sqr(f2_add(X, B)), A), C)
    D = f2_add(D, D)
    E = f2_scale(A, 3)
    F = f2_sqr(E)
    X3 = f2_sub(F, f2_add(D, D))
    Z3 = f2_sub(f2_sub(f2_sqr(f2_add(Y, Zc)), B), ZZ)
    Y3 = f2_sub(f2_mul(f2_sub(D, X3), E), f2_scale(C, 8))
    l0 = f2_sub(f2_sub(f2_sub(f2_sqr(f2_add(E, X)), A), F), f2_scale(B, 4))
    return (X3, Y3, Z3), (l0, f2_mul(E, ZZ), f2_mul(Z3, ZZ))


def line_add(T, Q):
    X1, Y1, Z1 = T
    Z1Z1 = f2_sqr(Z1)
    U2 = f2_mul(Q[0], Z1Z1)
    S2 = f2_mul(f2_mul(Q[1], Z1), Z1Z1)
    H = f2_sub(U2, X1)
    HH = f2_sqr(H)
    I = f2_scale(HH, 4)
    J = f2_mul(H, I)
    r = f2_sub(S2, Y1)
    r = f2_add(r, r)
    V = f2_mul(X1, I)
    X3 = f2_sub(f2_sub(f2_sqr(r), J), f2_add(V, V))
    JY = f2_mul(J, Y1)
    Y3 = f2_sub(f2_mul(f2_sub(V, X3), r), f2_add(JY, JY))
    Z3 = f2_sub(f2_sub(f2_sqr(f2_add(Z1, H)), Z1Z1), HH)
    l0 = f2_sub(f2_mul(r, Q[0]), f2_mul(Q[1], Z3))
    return (X3, Y3, Z3), (f2_add(l0, l0), r, Z3)


def miller_loop(pairs):
    """prod ml(P_i, Q_i) with the squarings shared; a pair with P or Q None contributes one"""
    live = [(p, q) for p, q in pairs if p is not None and q is not None]
    f = F12_ONE
    T = [(q[0], q[1], F2_ONE) for _, q in live]
    px = [(-2 * p[0] % P, 2 * p[1] % P) for p, _ in live]
    for b in range(62, -1, -1):
        if b != 62:
            f = f12_sqr(f)
        for i in range(len(live)):
            T[i], l = line_dbl(T[i])
            f = f12_mul_sparse(f, l[0], f2_scale(l[1], px[i][0]), f2_scale(l[2], px[i][1]))
        if (Z_ABS >> b) & 1:
            for i in range(len(live)):
                T[i], l = line_add(T[i], live[i][1])
                f = f12_mul_sparse(f, l[0], f2_scale(l[1], px[i][0]), f2_scale(l[2], px[i][1]))
    return f12_conj(f)


# --------------------------------------------------- final exponentiation ----
def _raise_z_half(a):
    r = f12_sqr(a)
    for n in (2, 3, 9, 32, 15):
        r = f12_mul(r, a)
        for _ in range(n):
            r = f12_sqr(r)
    return f12_conj(r)


def _raise_z(a):
    return f12_sqr(_raise_z_half(a))


def final_exp(f):
    """the reference's chain (easy part, then the hard part on the cyclotomic subgroup)"""
    ret = f12_mul(f12_conj(f), f12_inv(f))
    ret = f12_mul(ret, f12_frob(ret, 2))
    y0 = f12_sqr(ret)
    y1 = _raise_z(y0)
    y2 = _raise_z_half(y1)
    y1 = f12_mul(f12_conj(f12_mul(y1, f12_conj(ret))), y2)
    y2 = _raise_z(y1)
    y3 = _raise_z(y2)
    y3 = f12_mul(y3, f12_conj(y1))
    y1 = f12_mul(f12_frob(y1, 3), f12_frob(y2, 2))
    y2 = f12_mul(f12_mul(_raise_z(y3), y0), ret)
    y1 = f12_mul(y1, y2)
    return f12_mul(y1, f12_frob(y3, 1))


def pairing(p, q):
    return final_exp(miller_loop([(p, q)]))


def pairing_product(pairs):
    return final_exp(miller_loop(pairs))


# ---------------------------------------------------------------- inputs ----
G1, G2 = ei.GEN[1], ei.GEN[2]
NEG_G1 = (G1[0], -G1[1] % P)
N_RANDOM = 24


def neg_g1():
    return ei.affine_bytes(1, NEG_G1)


_PAIRS = []


def pairs():
    """[(P, Q)]: 24 seeded pairs, the generators, then (inf, Q), (P, inf), (inf, inf)"""
    if not _PAIRS:
        ks = mi.gen_scalars(2 * N_RANDOM, 0x9a1712)
        out = [(mi.smul(1, G1, ks[2 * i]), mi.smul(2, G2, ks[2 * i + 1])) for i in range(N_RANDOM)]
        out.append((G1, G2))
        out += [(None, out[1][1]), (out[2][0], None), (None, None)]
        _PAIRS.extend(out)
    return _PAIRS


N_PAIRS = N_RANDOM + 4
INF_PAIRS = (N_RANDOM + 1, N_RANDOM + 2, N_RANDOM + 3)


def pair_bytes(idx):
    """(P bytes, Q bytes) of the pairs idx, flat blst affine arrays"""
    ps = pairs()
    return (b"".join(ei.affine_bytes(1, ps[i][0]) for i in idx), b"".join(ei.affine_bytes(2, ps[i][1]) for i in idx))


def cyclic(n):
    return [i % N_PAIRS for i in range(n)]


# segment layouts of the fixture: name -> list of segments, each a list of pair indices
def _layout(lengths):
    out, k = [], 0
    for ln in lengths:
        out.append([(k + i) % N_RANDOM for i in range(ln)])
        k += ln
    return out


def layout_lengths(L):
    return [0, 1, 2, L, L + 1, 2 * L + 1, 0]


# (at these sizes the default piece length is 1: pair_piece_len() of pairing.hpp)
SEGMENTS = {
    "L1": _layout(layout_lengths(1)),
    "L3": _layout(layout_lengths(3)),
    "span100": [[i % N_RANDOM for i in range(100)]],
    "inf_ends": [[INF_PAIRS[0], 3, 4, INF_PAIRS[1], 5, 6, INF_PAIRS[2]]],
    "inf_only": [list(INF_PAIRS)],
}
