#!/usr/bin/env python3
"""The Frobenius coefficients of the Fp12 tower of BLS12-381, computed as plain
integers from p alone:

    Fp2 = Fp[u] / (u^2 + 1),  Fp6 = Fp2[v] / (v^3 - xi),  Fp12 = Fp6[w] / (w^2 - v),  xi = 1 + u

so w^6 = xi, and the p^k-power Frobenius sends w^i to gamma_k^i w^i with
gamma_k = xi^((p^k - 1) / 6) (an element of Fp2), after conjugating every Fp2
coefficient when k is odd.  In the tower's order an Fp12 value is
c[0] + c[1] v + c[2] v^2 + (c[3] + c[4] v + c[5] v^2) w, and coefficient j
carries w^(E[j]) with E = (0, 2, 4, 1, 3, 5).

FROB[k][j] = gamma_k^E[j] for k = 1, 2, 3.  Nothing here is copied from a table.
"""
P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
XI = (1, 1)
E = (0, 2, 4, 1, 3, 5)  # the power of w under coefficient j


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_pow(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = f2_mul(r, a)
        a = f2_mul(a, a)
        e >>= 1
    return r


def gamma(k):
    assert (P ** k - 1) % 6 == 0
    return f2_pow(XI, (P ** k - 1) // 6)


FROB = {k: [f2_pow(gamma(k), e) for e in E] for k in (1, 2, 3)}

for _k in (1, 2, 3):
    assert f2_pow(gamma(_k), 6) == f2_pow(XI, P ** _k - 1)
    assert FROB[_k][0] == (1, 0)
# the p^2 map is linear over Fp2 and its coefficients lie in Fp
assert all(c[1] == 0 for c in FROB[2])

if __name__ == "__main__":
    for k in (1, 2, 3):
        for j, c in enumerate(FROB[k]):
            print(k, j, hex(c[0]), hex(c[1]))
