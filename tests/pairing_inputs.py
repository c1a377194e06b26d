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


# ----------------------------------------- Fp12 values for the tower tests ----
# (tests/test_fp12_bounds.py, tests/test_gpu_fp12_tower.py, tests/test_gpu_pairing.py,
# tests/test_pairing_host.py and tests/golden/make_pairing_golden.py share them)
SPECIAL_NAMES = ("one", "minus_one", "fp", "fp2", "fp6", "w_only", "w", "v", "line", "pm1", "half", "mont_max", "rand")
# the final exponentiation of these is one, by its easy part (p^6 - 1)(p^2 + 1): a value
# a0 in Fp6 has a0^(p^6) = a0, and a1 w with a1 in Fp6 has (a1 w)^(p^6 - 1) = -1, whose
# p^2 + 1 power (an even one) is one
SPECIAL_FE_ONE = ("one", "minus_one", "fp", "fp2", "fp6", "w_only", "w", "v")
_SPECIAL = {}


def random_fp12(n, seed):
    import random
    rnd = random.Random(seed)
    return [[(rnd.randrange(P), rnd.randrange(P)) for _ in range(6)] for _ in range(n)]


def special_fp12():
    """{name: Fp12 value}, in the order of SPECIAL_NAMES (seeded)"""
    if not _SPECIAL:
        import random
        rnd = random.Random(0xf12e)
        f2 = lambda: (rnd.randrange(P), rnd.randrange(P))  # noqa: E731
        z = F2_ZERO
        mm = (P - 1) * ei.RINV % P  # the element whose blst Montgomery limbs are p - 1
        v = {
            "one": list(F12_ONE),
            "minus_one": [(P - 1, 0)] + [z] * 5,
            "fp": [(rnd.randrange(P), 0)] + [z] * 5,
            "fp2": [f2()] + [z] * 5,
            "fp6": [f2(), f2(), f2(), z, z, z],
            "w_only": [z, z, z, f2(), f2(), f2()],
            "w": [z, z, z, F2_ONE, z, z],
            "v": [z, F2_ONE, z, z, z, z],
            "line": [f2(), f2(), z, z, f2(), z],
            "pm1": [(P - 1, P - 1)] * 6,
            "half": [((P - 1) // 2, (P + 1) // 2)] * 6,
            "mont_max": [(mm, mm)] * 6,
            "rand": [f2() for _ in range(6)],
        }
        assert tuple(v) == SPECIAL_NAMES
        _SPECIAL.update(v)
    return _SPECIAL


def special_list():
    sp = special_fp12()
    return [sp[k] for k in SPECIAL_NAMES]


def unitary(f):
    """an element of the cyclotomic subgroup: u = conj(f) / f, then u frob2(u)"""
    u = f12_mul(f12_conj(f), f12_inv(f))
    return f12_mul(u, f12_frob(u, 2))


def f12_cyc_sqr(a, k=1):
    for _ in range(k):
        a = f12_sqr(a)
    return a


# the stored form of the engine (csrc/fp12l.hpp Fp12S): per coordinate value 2^392 mod p
# in 14 little-endian 28-bit limbs (uint32); six Fp2, c0 | c1 each: 168 words, 672 bytes
NL, R392 = 14, 1 << 392
R392_INV = pow(R392, -1, P)
FP12S_WORDS = 12 * NL


def limbs28(v):
    return [(v >> (28 * i)) & 0xfffffff for i in range(NL - 1)] + [v >> (28 * (NL - 1))]


def stored_words(a, plus_p=False):
    """Fp12 value -> 168 words: the canonical representative of every coordinate, or that plus p"""
    out = []
    for c in a:
        for x in c:
            out += limbs28(x * R392 % P + (P if plus_p else 0))
    return out


def stored_coords(words):
    """168 words -> the twelve stored integers (not reduced)"""
    assert len(words) == FP12S_WORDS
    return [sum(int(w) << (28 * i) for i, w in enumerate(words[k * NL:(k + 1) * NL])) for k in range(12)]


def stored_value(words):
    """168 words -> the Fp12 value they hold"""
    cs = [x * R392_INV % P for x in stored_coords(words)]
    return [(cs[2 * j], cs[2 * j + 1]) for j in range(6)]


def check_stored_S(words):
    """class S: limbs 0 .. 12 below 2^28, every coordinate below 2p"""
    for k in range(12):
        assert all(w < (1 << 28) for w in words[k * NL:(k + 1) * NL - 1]), ("limb", k)
    assert all(x < 2 * P for x in stored_coords(words)), "coordinate not below 2p"


# the ten reference calls the fixture's "tower" key records per special value
# (tests/golden/make_pairing_golden.py), and the model's value of each
TOWER_OPS = ("mul", "sqr", "inverse", "conjugate", "frobenius1", "frobenius2", "frobenius3", "mul_by_xy00z0",
             "cyclotomic_sqr", "final_exp")


def tower_model(a, b):
    """in the order of TOWER_OPS: binary ops with b, the sparse one with b's coefficients
    0, 1, 4, the cyclotomic squaring on fe(a)"""
    fe = final_exp(a)
    return [f12_mul(a, b), f12_sqr(a), f12_inv(a), f12_conj(a), f12_frob(a, 1), f12_frob(a, 2), f12_frob(a, 3),
            f12_mul_sparse(a, b[0], b[1], b[4]), f12_sqr(fe), fe]


def miller_line_cases(pair_idx=(0, 1), steps=3):
    """[(kind, T, Q)]: the running point at every line evaluation of the first `steps` steps
    of miller_loop for the pairs pair_idx; the first of each pair is the doubling of T = Q, Z = 1"""
    out = []
    for i in pair_idx:
        q = pairs()[i][1]
        T = (q[0], q[1], F2_ONE)
        for b in range(62, 62 - steps, -1):
            out.append(("dbl", T, q))
            T = line_dbl(T)[0]
            if (Z_ABS >> b) & 1:
                out.append(("add", T, q))
                T = line_add(T, q)[0]
    return out
