"""Single-chain Montgomery columns (fp.hpp MulChain) against the split form
(MulSplit, the untagged functions), on the host with every MSM_CHECK enabled
(tests/host/single_chain_shim.cpp; no GPU needed).

The single-chain form adds the same terms of every column in another order
(the previous column's carry first), so each product must equal the split
form's limb for limb, and no range check may fire in either: fp_mul, fp_mul2,
fp_sqr and fp_mul4 on random operands, on the largest lazy operands each is
documented for, and on 0, 1 and p - 1; then xyzz_madd (generic, a bucket's
first add, P = +-bucket, infinity), xyzz_add and xyzz_dbl through both forms.
"""
import ctypes
import os
import random
import subprocess

import pytest

import fp_bounds as fb
from test_fp_bounds import NL, P, RINV, _F, _arr, _dec, _elem, _limbs, _ref_add, _ref_dbl, _ref_madd, _val

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM_SRC = os.path.join(HERE, "host", "single_chain_shim.cpp")
SHIM_SO = os.path.join(HERE, "host", "_build", "single_chain_shim.so")
M28 = (1 << 28) - 1
ONE = fb.R % P  # Montgomery one
NARGS = {0: 2, 1: 1, 2: 4, 3: 8, 4: 4}  # fp_mul, fp_sqr, fp_mul2, fp_mul4, f_mul_sub


@pytest.fixture(scope="module")
def shim():
    deps = [SHIM_SRC] + [os.path.join(os.path.dirname(HERE), "msm_blst_amd", "csrc", f) for f in ("fp.hpp", "ec.hpp")]
    if not os.path.exists(SHIM_SO) or any(os.path.getmtime(d) > os.path.getmtime(SHIM_SO) for d in deps):
        os.makedirs(os.path.dirname(SHIM_SO), exist_ok=True)
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas",
                        "-Wl,-Bsymbolic", "-o", SHIM_SO, SHIM_SRC], check=True)
    L = ctypes.CDLL(SHIM_SO)
    vp = ctypes.c_void_p
    L.h_sc_fp.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp]
    L.h_sc_xyzz.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_int]
    L.h_overflow.argtypes = [ctypes.c_int]
    return L


def _fp(shim, form, op, args):
    assert len(args) == NARGS[op]
    keep = [_arr(a) for a in args]
    ptrs = (ctypes.c_void_p * 8)(*[ctypes.addressof(k) for k in keep] + [None] * (8 - len(keep)))
    r = (ctypes.c_uint32 * NL)()
    shim.h_overflow(1)
    shim.h_sc_fp(form, op, r, ptrs)
    assert shim.h_overflow(1) == 0, (form, op, args)
    return list(r)


def _both_fp(shim, op, args):
    split, chain = _fp(shim, 0, op, args), _fp(shim, 1, op, args)
    assert split == chain, (op, args)
    return chain


def _flat(limb, top):
    """every low limb at `limb`, the top limb `top`"""
    return [limb] * (NL - 1) + [top]


def _rand_lazy(rnd, bits, top_bits):
    return [rnd.randrange(1 << bits) for _ in range(NL - 1)] + [rnd.randrange(1 << top_bits)]


def _mont(*pairs):
    return sum(_val(a) * _val(b) for a, b in pairs) * RINV % P


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_products_random_operands(shim, seed):
    rnd = random.Random(seed)
    for _ in range(16):
        a, b = _rand_lazy(rnd, 30, 22), _rand_lazy(rnd, 30, 22)           # limbs < 2^30, value < 2^386
        assert _val(_both_fp(shim, 0, [a, b])) % P == _mont((a, b))
        assert _val(_both_fp(shim, 1, [a])) % P == _mont((a, a))
        x = [_rand_lazy(rnd, 28, 17) for _ in range(8)]                   # normalized, < 2p
        assert _val(_both_fp(shim, 2, x[:4])) % P == _mont((x[0], x[1]), (x[2], x[3]))
        assert _val(_both_fp(shim, 3, x)) % P == _mont(*[(x[2 * j], x[2 * j + 1]) for j in range(4)])
        want = (_val(x[0]) * _val(x[1]) - _val(x[2]) * _val(x[3])) * RINV % P
        assert _val(_both_fp(shim, 4, x[:4])) % P == want


def test_products_largest_lazy_operands(shim):
    """fp_mul / fp_sqr: limbs just below 2^30, values just below 2^386 (a column
    reaches 14 2^60 + 14 m p + carry < 2^64).  fp_mul2: a, b limbs below 2^29.6,
    c below 2^28.6, d below 2^29 (its documented column bound).  fp_mul4: the
    ranges of the Fp2 f_mul_sub that calls it (a lazy below 2^29.6 against
    normalized and 8p - b operands below 2^29, c and d in S)."""
    top386 = (1 << 22) - 5  # 13 limbs of 2^30 - 1 are ~ 2^366; top limb weighs 2^364
    big = _flat((1 << 30) - 1, top386)
    assert _val(big) < 1 << 386
    r = _both_fp(shim, 0, [big, big])
    assert all(x <= M28 for x in r[:NL - 1]) and _val(r) < 2 * P and _val(r) % P == _mont((big, big))
    r = _both_fp(shim, 1, [big])
    assert _val(r) < 2 * P and _val(r) % P == _mont((big, big))
    l296 = int(2 ** 29.6) - 1
    a = _flat(l296, (1 << 20) - 1)
    c = _flat(int(2 ** 28.6) - 1, (1 << 18) - 1)
    d = _flat((1 << 29) - 1, (1 << 18) - 1)
    r = _both_fp(shim, 2, [a, a, c, d])
    assert _val(r) % P == _mont((a, a), (c, d))
    s = _flat(M28, (1 << 17) - 1)
    r = _both_fp(shim, 3, [a, s, a, d, s, d, s, s])
    assert _val(r) % P == _mont((a, s), (a, d), (s, d), (s, s))


@pytest.mark.parametrize("op", [0, 1, 2, 3, 4])
def test_products_of_zero_one_and_p_minus_one(shim, op):
    vals = [_limbs(0), _limbs(1), _limbs(P - 1), _limbs(ONE)]
    n = NARGS[op]
    rnd = random.Random(50 + op)
    combos = [[v] * n for v in vals] + [[rnd.choice(vals) for _ in range(n)] for _ in range(24)]
    for args in combos:
        r = _both_fp(shim, op, args)
        v = [_val(a) for a in args]
        if op == 1:
            want = v[0] * v[0]
        elif op == 4:
            want = v[0] * v[1] - v[2] * v[3]
        else:
            want = sum(v[2 * j] * v[2 * j + 1] for j in range(n // 2))
        assert _val(r) % P == want * RINV % P, (op, args)


# ------------------------------------------------------------ xyzz (G1) ----
def _xyzz(shim, form, op, acc, other, flags=0):
    a = _arr(sum(acc, []))
    o = _arr(sum(other, [])) if other is not None else None
    shim.h_overflow(1)
    shim.h_sc_xyzz(form, op, a, o, flags)
    assert shim.h_overflow(1) == 0, (form, op, flags)
    out = list(a)
    return [out[k * NL:(k + 1) * NL] for k in range(4)]


def _both_xyzz(shim, op, acc, other, flags=0):
    split, chain = _xyzz(shim, 0, op, acc, other, flags), _xyzz(shim, 1, op, acc, other, flags)
    assert split == chain, (op, flags)
    return chain


def _dec4(c):
    return tuple(_dec(1, w) for w in c)


@pytest.mark.parametrize("seed", [None, 61, 62])
def test_madd_generic_and_first_add(shim, seed):
    rnd = random.Random(seed) if seed is not None else None
    r2 = rnd or random.Random(97)
    F = _F(1)
    acc = [_elem(1, rnd, fb.Xc())] + [_elem(1, r2, fb.S()) for _ in range(3)]
    pt = [_elem(1, r2, fb.canonical()) for _ in range(2)]
    for neg in (0, 1):
        out = _both_xyzz(shim, 0, acc, pt, neg)
        assert _dec4(out) == _ref_madd(F, _dec4(acc), _dec4(pt)[:2], neg)
    # a bucket's first add: acc is xyzz_from_aff of a row (ZZ = ZZZ = 1)
    row = [_elem(1, r2, fb.canonical()) for _ in range(2)]
    first = [row[0], row[1], _limbs(ONE), _limbs(ONE)]
    for neg in (0, 1):
        want = _ref_madd(F, _dec4(first), _dec4(pt)[:2], neg)
        for affine in (0, 2):
            assert _dec4(_both_xyzz(shim, 0, first, pt, neg | affine)) == want, (neg, affine)


def test_madd_equal_opposite_and_infinity(shim):
    rnd = random.Random(63)
    F = _F(1)
    row = [_elem(1, rnd, fb.canonical()) for _ in range(2)]
    first = [row[0], row[1], _limbs(ONE), _limbs(ONE)]
    for affine in (0, 2):
        # P == bucket: the doubling branch; P == -bucket: infinity (all zero)
        assert _dec4(_both_xyzz(shim, 0, first, row, affine)) == _ref_dbl(F, _dec4(first))
        out = _both_xyzz(shim, 0, first, row, 1 | affine)
        assert all(w == 0 for c in out for w in c)
    # bucket at infinity: xyzz_from_aff of the row, negated or not
    inf = [_limbs(0)] * 4
    out = _both_xyzz(shim, 0, inf, row, 0)
    assert out == first
    out = _both_xyzz(shim, 0, inf, row, 1)
    assert _dec4(out) == (_val(row[0]), (P - _val(row[1])) % P, ONE, ONE)


@pytest.mark.parametrize("seed", [None, 71, 72])
def test_add_and_dbl(shim, seed):
    rnd = random.Random(seed) if seed is not None else None
    r2, r3 = rnd or random.Random(98), rnd or random.Random(99)
    F = _F(1)
    a = [_elem(1, rnd, fb.Xc())] + [_elem(1, r2, fb.S()) for _ in range(3)]
    b = [_elem(1, r3, fb.Xc())] + [_elem(1, r3, fb.S()) for _ in range(3)]
    assert _dec4(_both_xyzz(shim, 1, a, b)) == _ref_add(F, _dec4(a), _dec4(b))
    assert _dec4(_both_xyzz(shim, 2, a, None)) == _ref_dbl(F, _dec4(a))
    inf = [_limbs(0)] * 4
    assert _both_xyzz(shim, 1, a, inf) == a
    assert _both_xyzz(shim, 1, inf, b) == b
    # equal operands double, opposite ones (y negated mod p) give infinity
    s = [_elem(1, r2, fb.S()) for _ in range(4)]
    assert _dec4(_both_xyzz(shim, 1, s, s)) == _ref_dbl(F, _dec4(s))
    opp = [s[0], _limbs((P - _val(s[1]) % P) % P), s[2], s[3]]
    out = _both_xyzz(shim, 1, s, opp)
    assert all(w == 0 for c in out for w in c)
