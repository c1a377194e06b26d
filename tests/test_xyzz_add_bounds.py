"""Range proof and host runs of the regrouped general add (ec.hpp xyzz_add; no
GPU needed).

xyzz_add computes 12 products and 2 squares with 11 Montgomery reductions:

    P = X2 ZZ1 - X1 ZZ2      R = Y2 ZZZ1 - Y1 ZZZ2     (one f_mul_sub each)
    PP = P^2                 PPP = P PP
    V = ZZ2 PP               ZZ3 = ZZ1 V               Q = X1 V
    W = ZZZ2 PPP             ZZZ3 = ZZZ1 W
    X3 = R^2 - PPP - 2Q      Y3 = R (Q - X3) - Y1 W    (f_mul_sub)

instead of reducing U1 = X1 ZZ2 and S1 = Y1 ZZZ2 on their own (13 reductions:
the formula kept below as _old_add, which tests/fp_bounds.py trace_add models).

The one-lane Fp2 keeps the old form (ec.hpp AddRegrouped: two of its kernels,
already at 512 registers, spilled with the four-product sums); its bounds close
like the others', so group 2 stays in the proof and its host runs check the form
it keeps against the same references.

1. The interval model of tests/fp_bounds.py over this sequence, for Fp, the
   one-lane Fp2 and the lane-pair Fp2L forms.  The two new f_mul_sub calls take
   X1 and X2 in class X (normalized, < 10p), not the "< 6p lazy" the Y3 line
   feeds it: the bound that has to hold is a b + c (4p - d) < 63 p^2 with every
   FIPS column below 2^64.  P and R come out in class S (they were < 6p lazy),
   so every later range is the old form's or smaller; the PP == 0 branch
   doubles the untouched acc (x in class X, the rest in S).
2. The same header text compiled for the host with every range check enabled
   (tests/host/fp_host_shim.cpp) runs xyzz_add on random points, on coordinates
   at the class limits, on P + P (another representative of the same point, and
   the same coordinates), P + (-P), infinity on either side and a negated Y: no
   check fires, every stored coordinate is in its class, and the result is what
   the old formula gives mod p (the same point in the doubling branch, which
   now doubles another representative) and what the oracle's xyzz add gives.
"""
import ctypes
import random

import pytest

import fp_bounds as fb
import oracle_ffi as of
from test_fp_bounds import NL, P, RINV, _F, _arr, _check_S, _dec, _elem, _limbs, _maxlimb, _ref_dbl, _val
from test_fp_bounds import shim  # noqa: F401  (the checked host build of fp.hpp / ec.hpp / fp2l.hpp)

GROUPS = [1, 2, 3]  # Fp, Fp2 on one lane, Fp2 on a lane pair


# ------------------------------------------------------ interval proof ----
def trace_add_regrouped(group):
    """xyzz_add (ec.hpp): acc (x in X, rest S) += b (x in X, rest S)"""
    F = fb.Field(group)
    x, y, zzz, zz = fb.Xc(), fb.S(), fb.S(), fb.S()
    bx, by, bzzz, bzz = fb.Xc(), fb.S(), fb.S(), fb.S()
    Pd = F.mul_sub(bx, zz, x, bzz)
    Rd = F.mul_sub(by, zzz, y, bzzz)
    PP = F.sqr(Pd)
    fb.need(PP.is_S(), "add: PP must be S for f_is_zero_S")
    V = F.mul_bs(bzz, PP)
    zz3 = F.mul_bs(zz, V)
    Q = F.mul_bs(x, V)
    PPP = F.mul_bs(Pd, PP)
    W = F.mul_bs(bzzz, PPP)
    zzz3 = F.mul_bs(zzz, W)
    X3 = fb._x3(F, Rd, PPP, Q)
    t = fb.sub(Q, X3, 16)
    Y3 = F.mul_sub(t, Rd, y, W)
    dbl = fb.trace_dbl(group, (x, y, zzz, zz))   # PP == 0: the untouched acc is doubled
    return (X3, Y3, zzz3, zz3), dbl, (Pd, Rd, V, W, Q, PPP)


@pytest.mark.parametrize("group", GROUPS)
def test_regrouped_add_interval_proof(group):
    main, dbl, (Pd, Rd, V, W, Q, PPP) = trace_add_regrouped(group)   # raises RangeError if a column wraps
    # P and R are products now: class S, below the < 6p lazy of the old form
    old_PR = fb.sub(fb.S(), fb.S())
    for d in (Pd, Rd):
        assert d.is_S(), d
        assert d.vmax < old_PR.vmax and all(a <= b for a, b in zip(d.lim, old_PR.lim))
    assert all(v.is_S() for v in (V, W, Q, PPP))   # every f_sub / f_sub_2x subtrahend is S
    for outs in (main, dbl):
        assert outs[0].is_X(), outs[0]
        assert all(o.is_S() for o in outs[1:]), outs
    # X3 and Y3 are bounded by the old form's bounds or less (R shrank); ZZ3 and
    # ZZZ3 are products with one input-class factor (ZZ1 V, < 2p 1.002p / R + p)
    # where the old form multiplied two product outputs, so their bound moves in
    # the fourth decimal and stays a product output's (< 1.1p)
    old_main, _ = fb.trace_add(group)
    for new, old in zip(main[:2], old_main[:2]):
        assert new.vmax <= old.vmax and all(a <= b for a, b in zip(new.lim, old.lim)), (new, old)
    for new in main[2:]:
        assert new.vmax < 11 * P // 10, new


def test_mul_sub_value_bound_with_class_X_operands():
    """f_mul_sub(Fp) = fp_mul2(a, b, c, 4p - d) with a, c in class X and b, d in S:
    a b + c (4p - d) < 63 p^2 (the bound fp_mul2 is documented for), and its
    output is far inside S."""
    a, b = fb.Xc(), fb.S()
    nd = fb.neg(fb.S(), 4)
    assert a.vmax * b.vmax + a.vmax * nd.vmax < 63 * P * P
    assert fb.mul2(a, b, a, nd).vmax < 11 * P // 10
    # the Fp2 forms: four products, 8p-adjusted negations (fp_mul4)
    assert fb.mul_sub_fp2(a, b, a, b).vmax < 11 * P // 10


def test_model_rejects_a_lazy_first_operand_pair():
    """Not vacuous: with X1, X2 left as the unnormalized X3 chain (limbs < 2^31)
    the two-product sum overflows a column."""
    lazyx = fb.sub2x(fb.S(), fb.S(), fb.S())
    with pytest.raises(fb.RangeError):
        fb.Field(1).mul_sub(lazyx, fb.sub(fb.S(), fb.S()), lazyx, fb.S())


# ----------------------------------------------------------- host runs ----
def _rep(g, res, k):
    """the representative res + k p of a residue (per component), normalized limbs"""
    if g == 1:
        return _limbs(res + k * P)
    return _limbs(res[0] + k * P) + _limbs(res[1] + k * P)


def _words(g, pt, kx, ks):
    """xyzz words of residues (X, Y, ZZZ, ZZ): x as X + kx p (class X), the rest + ks p (class S)"""
    return [_rep(g, pt[0], kx)] + [_rep(g, c, ks) for c in pt[1:]]


def _rand_el(F, rnd):
    return rnd.randrange(1, P) if F.g == 1 else (rnd.randrange(1, P), rnd.randrange(P))


def _rand_point(F, rnd):
    """a consistent xyzz representative (x l^2, y l^3, l^3, l^2) in the Montgomery domain"""
    x, y, l = _rand_el(F, rnd), _rand_el(F, rnd), _rand_el(F, rnd)
    l2 = F.mul(l, l)
    l3 = F.mul(l2, l)
    return (F.mul(x, l2), F.mul(y, l3), l3, l2), (x, y)


def _scaled(F, aff, l):
    l2 = F.mul(l, l)
    l3 = F.mul(l2, l)
    return (F.mul(aff[0], l2), F.mul(aff[1], l3), l3, l2)


def _old_add(F, a, b):
    """the 13-reduction form this add replaces, mod p; returns (coords, branch)"""
    X1, Y1, ZZZ1, ZZ1 = a
    X2, Y2, ZZZ2, ZZ2 = b
    U1, S1 = F.mul(X1, ZZ2), F.mul(Y1, ZZZ2)
    Pd, Rd = F.sub(F.mul(X2, ZZ1), U1), F.sub(F.mul(Y2, ZZZ1), S1)
    zz12, zzz12 = F.mul(ZZ1, ZZ2), F.mul(ZZZ1, ZZZ2)
    if Pd == F.zero():
        if Rd == F.zero():   # acc rewritten as (U1, S1, ZZZ1 ZZZ2, ZZ1 ZZ2), then doubled
            return _ref_dbl(F, (U1, S1, zzz12, zz12)), "dbl"
        return None, "inf"
    PP = F.mul(Pd, Pd)
    PPP = F.mul(Pd, PP)
    Q = F.mul(U1, PP)
    X3 = F.sub(F.sub(F.mul(Rd, Rd), PPP), F.add(Q, Q))
    Y3 = F.sub(F.mul(Rd, F.sub(Q, X3)), F.mul(S1, PPP))
    return (X3, Y3, F.mul(zzz12, PPP), F.mul(zz12, PP)), "add"


def _same_point(F, a, b):
    return F.mul(a[0], b[3]) == F.mul(b[0], a[3]) and F.mul(a[1], b[2]) == F.mul(b[1], a[2])


# the oracle's xyzz add (Montgomery R = 2^384, 6 x 64-bit limbs, canonical values)
def _or_fp(L, fn, v):
    a = (ctypes.c_uint64 * 6)(*[(v >> (64 * i)) & (2**64 - 1) for i in range(6)])
    r = (ctypes.c_uint64 * 6)()
    getattr(L, fn)(r, a)
    return sum(int(w) << (64 * i) for i, w in enumerate(r))


def _oracle_add(F, a, b):
    """a, b: residues in the engine's Montgomery domain (R = 2^392); the same
    field elements go through or_p{1,2}xyzz_dadd and come back in that domain"""
    L = of.lib()
    comps = (lambda c: [c]) if F.g == 1 else (lambda c: list(c))

    def pack(pt):
        ws = []
        for c in pt:
            for v in comps(c):
                m = _or_fp(L, "or_fp_to_mont", v * RINV % P)
                ws += [(m >> (64 * i)) & (2**64 - 1) for i in range(6)]
        return (ctypes.c_uint64 * len(ws))(*ws)

    A, B = pack(a), pack(b)
    r = (ctypes.c_uint64 * len(A))()
    getattr(L, f"or_p{F.g}xyzz_dadd")(r, A, B)
    vals = [_or_fp(L, "or_fp_from_mont", sum(int(r[6 * k + i]) << (64 * i) for i in range(6))) * fb.R % P
            for k in range(len(A) // 6)]
    if F.g == 1:
        return tuple(vals)
    return tuple((vals[2 * k], vals[2 * k + 1]) for k in range(4))


def _run_add(shim, group, acc, oth):  # noqa: F811
    g = 1 if group == 1 else 2
    W = NL * g
    a = _arr(sum(acc, []))
    shim.h_overflow(1)
    if group == 3:
        shim.h_xyzz_l(1, a, _arr(sum(oth, [])), 0)
    else:
        shim.h_xyzz(group, 1, a, _arr(sum(oth, [])), 0)
    assert shim.h_overflow(1) == 0, "a range check fired"
    out = list(a)
    return [out[k * W:(k + 1) * W] for k in range(4)]


def _check(shim, group, acc, oth, branch):  # noqa: F811
    """run acc += oth on the checked host build; compare with the old formula
    and the oracle; returns the decoded result (None: infinity)"""
    g = 1 if group == 1 else 2
    F = _F(g)
    dec = lambda ws: tuple(_dec(g, w) for w in ws)  # noqa: E731
    coords = _run_add(shim, group, acc, oth)
    want, got_branch = _old_add(F, dec(acc), dec(oth))
    assert got_branch == branch
    orc = _oracle_add(F, dec(acc), dec(oth))
    if branch == "inf":
        assert all(w == 0 for c in coords for w in c)      # ZZ == 0 exactly (all four, as xyzz_set_inf)
        assert orc[2] == F.zero() and orc[3] == F.zero()
        return None
    _check_S(g, coords[0], 10)
    for c in coords[1:]:
        _check_S(g, c)
    got = dec(coords)
    if branch == "add":
        assert got == want        # coordinate by coordinate: the regrouping keeps every value mod p
        assert got == orc
    elif group == 2:              # the one-lane Fp2 keeps the old form and its doubled representative
        assert got == want
        assert _same_point(F, got, orc)
    else:
        assert _same_point(F, got, want)   # the doubled representative differs (acc itself, not (U1, S1, ..))
        assert got == _ref_dbl(F, dec(acc))
        assert got == orc         # the oracle doubles the untouched first operand as well
    return got


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("seed", [51, 52])
def test_random_points_and_negated_y(shim, group, seed):  # noqa: F811
    g = 1 if group == 1 else 2
    F = _F(g)
    rnd = random.Random(seed)
    for _ in range(3):
        a, _ = _rand_point(F, rnd)
        b, _ = _rand_point(F, rnd)
        kxa, kxb = rnd.randrange(10), rnd.randrange(10)
        _check(shim, group, _words(g, a, kxa, rnd.randrange(2)), _words(g, b, kxb, rnd.randrange(2)), "add")
        # a + (-b): the negated Y as its upper representative (2p - y)
        nb = (b[0], F.neg(b[1]), b[2], b[3])
        r1 = _check(shim, group, _words(g, a, kxa, 1), _words(g, nb, kxb, 1), "add")
        # -(a + (-b)) == (-a) + b
        na = (a[0], F.neg(a[1]), a[2], a[3])
        r2 = _check(shim, group, _words(g, na, 0, 0), _words(g, b, 0, 0), "add")
        assert _same_point(F, r1, (r2[0], F.neg(r2[1]), r2[2], r2[3]))


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("seed", [None, 61, 62])
def test_coordinates_at_the_class_limits(shim, group, seed):  # noqa: F811
    """X at its largest normalized value (every low limb 2^28 - 1, < 10p), the S
    coordinates just below 2p: the widest operands the two f_mul_sub calls, V, W
    and the Y3 line see."""
    g = 1 if group == 1 else 2
    rnd = random.Random(seed) if seed is not None else None
    # (seed None: equal coordinates on both sides would be P + P; the second
    # operand's S coordinates are drawn just below their maxima instead)
    r2 = rnd or random.Random(63)
    acc = [_elem(g, rnd, fb.Xc())] + [_elem(g, rnd, fb.S()) for _ in range(3)]
    oth = [_elem(g, rnd, fb.Xc())] + [_elem(g, r2, fb.S()) for _ in range(3)]
    assert _val(acc[0][:NL]) >= 9 * P and _val(acc[1][:NL]) >= P
    _check(shim, group, acc, oth, "add")
    _check(shim, group, oth, acc, "add")


@pytest.mark.parametrize("group", GROUPS)
def test_mul_sub_primitive_with_class_X_operands(shim, group):  # noqa: F811
    """f_mul_sub(a, b, c, d) alone with a, c at the class X maximum, b, d at the S maximum"""
    g = 1 if group == 1 else 2
    F = _F(g)
    X = _elem(g, None, fb.Xc())
    S = _elem(g, None, fb.S())
    S2 = _elem(g, random.Random(64), fb.S())
    r = (ctypes.c_uint32 * (NL * g))()
    shim.h_overflow(1)
    if group == 1:
        shim.h_fp_op(9, r, _arr(X), _arr(S), _arr(X), _arr(S2), None, None, None, None)
    elif group == 2:
        shim.h_fp2_op(3, r, _arr(X), _arr(S), _arr(X), _arr(S2))
    else:
        shim.h_fp2l_op(3, r, _arr(X), _arr(S), _arr(X), _arr(S2))
    assert shim.h_overflow(1) == 0
    _check_S(g, list(r))
    x, s, s2 = _dec(g, X), _dec(g, S), _dec(g, S2)
    assert _dec(g, list(r)) == F.sub(F.mul(x, s), F.mul(x, s2))


@pytest.mark.parametrize("group", GROUPS)
def test_doubling_infinity_and_opposite_points(shim, group):  # noqa: F811
    g = 1 if group == 1 else 2
    F = _F(g)
    rnd = random.Random(71)
    a, aff = _rand_point(F, rnd)
    # P + P, the same coordinates in other representatives (P == p, not 0, inside)
    _check(shim, group, _words(g, a, 0, 0), _words(g, a, 9, 1), "dbl")
    _check(shim, group, _words(g, a, 9, 1), _words(g, a, 9, 1), "dbl")
    # P + P, another xyzz representative of the same point
    b = _scaled(F, aff, _rand_el(F, rnd))
    r1 = _check(shim, group, _words(g, a, 3, 1), _words(g, b, 5, 0), "dbl")
    r2 = _check(shim, group, _words(g, b, 0, 0), _words(g, a, 0, 1), "dbl")
    assert _same_point(F, r1, r2)
    # P + (-P)
    nb = (b[0], F.neg(b[1]), b[2], b[3])
    _check(shim, group, _words(g, a, 2, 1), _words(g, nb, 7, 1), "inf")
    _check(shim, group, _words(g, nb, 0, 0), _words(g, a, 0, 0), "inf")
    # infinity on either side: the other operand comes back word for word
    inf = [[0] * (NL * g) for _ in range(4)]
    wa = _words(g, a, 9, 1)
    assert _run_add(shim, group, inf, wa) == wa
    assert _run_add(shim, group, wa, inf) == wa
    assert _run_add(shim, group, inf, inf) == inf
