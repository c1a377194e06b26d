"""Range proof and host runs of a bucket's first add (ec.hpp xyzz_madd with
acc_affine set; no GPU needed).

A bucket starts as xyzz_from_aff of its first row (ZZ = ZZZ = 1) and its second
row enters through xyzz_madd(acc, p, neg, acc_affine = true), which skips the
four products by one:

    U2 := X2            S2 := +-Y2 (a negated Y2 reduced: f_neg4 + f_nred)
    P = U2 - X1         R = S2 - Y1        PP = P^2
    PPP = P PP          Q = X1 PP
    X3 = R^2 - PPP - 2Q                    Y3 = R (Q - X3) - Y1 PPP
    ZZ3 := PP           ZZZ3 := PPP

1. The interval model of tests/fp_bounds.py (same transfer functions, same
   classes) over this sequence, for Fp, the one-lane Fp2 and the lane-pair Fp2
   forms: X1, Y1 as xyzz_from_aff leaves them (canonical, or f_nred of a
   negation), X2, Y2 canonical rows.  Every f_sub subtrahend is in class S, R
   stays below the 6p that f_sqr / f_mul_sub are proven for, the stored
   coordinates are in S (x in X), and the PP == 0 branch doubles the untouched
   affine bucket.  The model also shows why the negated Y2 must be reduced: left
   lazy (< 4p) it puts R at 8p.
2. The same header text compiled for the host with every range check enabled
   (tests/host/first_pair_shim.cpp) runs from_aff + first add on max-limb and
   random canonical rows, with the flag set and clear: no check fires, every
   stored coordinate is in its class, and both give the coordinates the plain
   algebra mod p gives (X3, Y3, ZZZ1 PPP, ZZ1 PP with ZZ1 = ZZZ1 = 1).
"""
import ctypes
import os
import random
import subprocess

import pytest

import fp_bounds as fb
from test_fp_bounds import NL, P, _F, _arr, _check_S, _dec, _elem, _ref_dbl, _ref_madd

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM_SRC = os.path.join(HERE, "host", "first_pair_shim.cpp")
SHIM_SO = os.path.join(HERE, "host", "_build", "first_pair_shim.so")
ONE = fb.R % P  # Montgomery one


def one_iv():
    """ZZ = ZZZ = 1 exactly (f_one: the limbs of ONE28)"""
    return fb.Iv(fb.C["ONE28"], ONE)


def from_aff_y():
    """Y1 as xyzz_from_aff leaves it: the canonical row's y, or f_nred(f_neg4(y))"""
    return fb.union(fb.canonical(), fb.nred(fb.neg(fb.canonical())))


def trace_first_pair(group, negate, reduce_neg=True):
    """xyzz_madd(acc, p, neg, acc_affine = true), acc = xyzz_from_aff of a canonical row"""
    F = fb.Field(group)
    x, y = fb.canonical(), from_aff_y()
    fb.need(y.is_S(), "first pair: Y1 must be S")
    px, py = fb.canonical(), fb.canonical()
    if negate:
        y2 = fb.neg(py)
        if reduce_neg:
            y2 = fb.nred(y2)
    else:
        y2 = py
    Pd = fb.sub(px, x, 16)            # U2 := X2
    Rd = fb.sub(y2, y)                # S2 := +-Y2
    PP = F.sqr(Pd)
    fb.need(PP.is_S(), "first pair: PP must be S for f_is_zero_S")
    PPP = F.mul_bs(Pd, PP)
    Q = F.mul_bs(x, PP)
    X3 = fb._x3(F, Rd, PPP, Q)
    t = fb.sub(Q, X3, 16)
    Y3 = F.mul_sub(t, Rd, y, PPP)
    # PP == 0: the untouched affine bucket (X1, Y1, 1, 1) is doubled
    dbl = fb.trace_dbl(group, (x, y, one_iv(), one_iv()))
    return (X3, Y3, PPP, PP), dbl, Rd


@pytest.mark.parametrize("group", [1, 2, 3])
@pytest.mark.parametrize("negate", [False, True])
def test_first_pair_interval_proof(group, negate):
    main, dbl, Rd = trace_first_pair(group, negate)
    # R within what the generic formula feeds f_sqr / f_mul_sub (S - S + 4p < 6p)
    generic_R = fb.sub(fb.S(), fb.S())
    assert Rd.vmax <= generic_R.vmax < 6 * P
    assert all(a <= b for a, b in zip(Rd.lim, generic_R.lim))
    for outs in (main, dbl):
        assert outs[0].is_X(), outs[0]
        assert all(o.is_S() for o in outs[1:]), outs


def test_lazy_negated_y2_would_leave_the_proven_range():
    """f_neg4 alone gives 4p - Y2 with limbs up to 2^29: R = S2 + 4p - Y1 reaches
    8p, past the < 6p of every proven caller of f_sqr / f_mul_sub."""
    _, _, Rd = trace_first_pair(1, True, reduce_neg=False)
    assert Rd.vmax >= 6 * P
    _, _, Rd = trace_first_pair(1, True)
    assert Rd.vmax < 6 * P


# ----------------------------------------------------------- host runs ----
@pytest.fixture(scope="module")
def shim():
    deps = [SHIM_SRC, os.path.join(HERE, "host", "fp_host_shim.cpp")] + [
        os.path.join(os.path.dirname(HERE), "msm_blst_amd", "csrc", f) for f in ("fp.hpp", "ec.hpp", "fp2l.hpp")]
    if not os.path.exists(SHIM_SO) or any(os.path.getmtime(d) > os.path.getmtime(SHIM_SO) for d in deps):
        os.makedirs(os.path.dirname(SHIM_SO), exist_ok=True)
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wall", "-Wno-unknown-pragmas",
                        "-Wl,-Bsymbolic", "-o", SHIM_SO, SHIM_SRC], check=True)
    L = ctypes.CDLL(SHIM_SO)
    vp = ctypes.c_void_p
    L.h_first_pair.argtypes = [ctypes.c_int, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.h_overflow.argtypes = [ctypes.c_int]
    return L


def _first_pair(shim, group, rows, neg1, neg2, affine):
    g = 1 if group == 1 else 2
    W = NL * g
    out = (ctypes.c_uint32 * (4 * W))()
    shim.h_overflow(1)
    shim.h_first_pair(group, out, _arr(sum(rows, [])), neg1, neg2, affine)
    assert shim.h_overflow(1) == 0, (group, neg1, neg2, affine)
    out = list(out)
    return [out[k * W:(k + 1) * W] for k in range(4)]


def _one(F):
    return ONE if F.g == 1 else (ONE, 0)


@pytest.mark.parametrize("group", [1, 2, 3])
@pytest.mark.parametrize("seed", [None, 31, 32])
def test_first_pair_host_run(shim, group, seed):
    g = 1 if group == 1 else 2
    F = _F(g)
    rnd = random.Random(seed) if seed is not None else None
    r2 = rnd or random.Random(95)
    # seed None: the first row at the canonical maximum, the second near it
    rows = [_elem(g, rnd, fb.canonical()), _elem(g, rnd, fb.canonical()),
            _elem(g, r2, fb.canonical()), _elem(g, r2, fb.canonical())]
    dec = lambda ws: tuple(_dec(g, w) for w in ws)  # noqa: E731
    x1, y1, x2, y2 = dec(rows)
    for neg1 in (0, 1):
        for neg2 in (0, 1):
            acc = (x1, F.neg(y1) if neg1 else y1, _one(F), _one(F))
            want = _ref_madd(F, acc, (x2, y2), neg2)
            for affine in (0, 1):
                coords = _first_pair(shim, group, rows, neg1, neg2, affine)
                _check_S(g, coords[0], 10)
                for c in coords[1:]:
                    _check_S(g, c)
                assert dec(coords) == want, (neg1, neg2, affine)


@pytest.mark.parametrize("group", [1, 2, 3])
def test_first_pair_equal_and_opposite_rows(shim, group):
    """PP == 0 from the affine state: equal rows double the untouched bucket,
    opposite rows leave infinity (ZZ == 0 exactly)."""
    g = 1 if group == 1 else 2
    F = _F(g)
    rnd = random.Random(41)
    row = [_elem(g, rnd, fb.canonical()), _elem(g, rnd, fb.canonical())]
    dec = lambda ws: tuple(_dec(g, w) for w in ws)  # noqa: E731
    x, y = dec(row)
    for neg in (0, 1):
        coords = _first_pair(shim, group, row + row, neg, neg, 1)
        acc = (x, F.neg(y) if neg else y, _one(F), _one(F))
        assert dec(coords) == _ref_dbl(F, acc), neg
        coords = _first_pair(shim, group, row + row, neg, 1 - neg, 1)
        assert all(w == 0 for c in coords for w in c), neg
