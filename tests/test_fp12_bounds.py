"""Range proof and host runs of the Fp12 tower and the Miller loop's line functions
(msm_blst_amd/csrc/fp12l.hpp on fp2l.hpp / fp2l_mem.hpp; no GPU needed).

fp12l.hpp keeps every value between two products in class S (limbs 0..12 below 2^28,
value below 2p): t_add / t_sub / t_neg / t_conj / t_xi reduce after every sum.

1. The interval model of tests/fp_bounds.py walks every primitive and every composite
   of the header (prove_tower): each maps S to S, no product is ever handed anything
   but S, the norm of f_inv(Fp2L) is a legal fp_inv input and the factors -2 x_P and
   2 y_P of k_pair_init land in S.  DESIGN.md section 21 records the table.
2. The SAME header text compiled for the host with every range check armed
   (tests/host/fp12_host_shim.cpp, on the two-thread lane-pair harness of
   fp_host_shim.cpp) runs each Fp12 operation and both line functions, aliased and
   not, on stored values in four operand forms: (a) canonical, (b) every coordinate
   plus p, (c) every coordinate the class-S max-limb element (exact, and random below
   it) and (d) the special values of pairing_inputs.special_fp12().  For every case:
   no check fires, every stored output limb 0..12 is at most 2^28 - 1, every output
   coordinate is below 2p, and the value mod p is the plain-integer model's
   (tests/pairing_inputs.py, itself pinned to the reference by tests/golden/pairing.json).
3. Negative controls: an operand outside the documented class trips a check in the
   model and in the shim, so neither is vacuous.
"""
import ctypes
import os
import random
import subprocess

import pytest

import fp_bounds as fb
import pairing_inputs as pi
from test_fp_bounds import NL, P, _arr, _maxlimb, _val

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "msm_blst_amd", "csrc")
SHIM_SRC = os.path.join(HERE, "host", "fp12_host_shim.cpp")
SHIM_SO = os.path.join(HERE, "host", "_build", "fp12_host_shim.so")
MUL, SQR, SPARSE, CONJ, FROB, INV, CSQR, LINE_DBL, LINE_ADD = range(9)
W = pi.FP12S_WORDS
CSQR_RUNS = (1, 2, 3, 9, 15, 32)  # the run lengths of the final exponentiation's program


# ------------------------------------------------------------ interval model ----
@pytest.fixture(scope="module")
def rows():
    return fb.prove_tower()


def test_tower_primitives_map_S_to_S(rows):
    for name in ("t_add", "t_sub", "t_dbl", "t_neg", "t_conj", "t_xi"):
        assert all(o.is_S() for o in rows[name]), name
    # t_xi lane by lane: the odd lane's sum a1 + a0 and the even lane's fp_sub<4> a0 + 4p - a1
    s = fb.S()
    odd, even = fb.add(s, s), fb.sub(s, s, 4)
    assert odd.vmax < 4 * P and even.vmax < 6 * P
    assert fb.nred(odd).is_S() and fb.nred(even).is_S()


def test_products_accept_S_and_return_S(rows):
    s = fb.S()
    assert fb.mul_bs_fp2(s, s).is_S()      # f_mul_bs, a in S and b in S
    assert fb.sqr_fp2l(s).is_S()           # f_sqr of S
    assert fb.mul(s, s).is_S()             # t_scale: fp_mul of S by S
    for name in ("t_mul (f_mul_bs, S x S)", "t_sqr (f_sqr, S)", "t_scale"):
        assert all(o.is_S() for o in rows[name]), name


def test_inversion_norm_and_pair_init_factors(rows):
    norm, inv = fb.f_inv_fp2l(fb.S())
    assert norm.vmax < 4 * P and inv.is_S()          # sq + psq: below 4p lazy, a legal fp_inv input
    assert fb.fp_inv_iv(norm).is_S()
    px, py = fb.pair_init_factors()                  # fp_add / fp_neg<4> / fp_nred of k_pair_init
    assert px.is_S() and py.is_S()


def test_composites_never_hand_a_product_anything_but_S(rows):
    """every t_mul / t_sqr of a trace demands S (fb.RangeError otherwise): the traces completed"""
    want = {"t_mul6": 3, "t_mul6_xy0": 3, "t_mul6_0y0": 3, "t_cof6": 4, "t_sqr4": 2, "t_cyc_lo / t_cyc_hi": 2,
            "t_mul12": 6, "t_sqr12": 6, "t_mul12_sparse": 6, "t_frob12": 6, "t_inv12": 6, "t_cyc_sqr12": 6,
            "pair_line_dbl": 6, "pair_line_add": 6}
    for name, n in want.items():
        assert len(rows[name]) == n and all(o.is_S() for o in rows[name]), name
    assert len(rows) == 25


def test_model_rejects_an_operand_outside_class_S():
    """not vacuous: a class-X value (normalized, below 10p) as the b operand of t_mul has a
    top limb above 8p's, so f_mul_bs's 8p - b would go negative; and a sum left lazy (t_sub
    without its f_nred) is refused by the next product"""
    with pytest.raises(fb.RangeError):
        fb.t_mul(fb.S(), fb.Xc())
    with pytest.raises(fb.RangeError):
        fb.mul_bs_fp2(fb.S(), fb.Xc())
    lazy = fb.sub(fb.S(), fb.S(), 4)
    with pytest.raises(fb.RangeError):
        fb.t_mul(lazy, fb.S())
    with pytest.raises(fb.RangeError):
        fb.mul_bs_fp2(fb.S(), lazy)


# ----------------------------------------------------------------- host runs ----
@pytest.fixture(scope="module")
def shim():
    deps = [SHIM_SRC, os.path.join(HERE, "host", "fp_host_shim.cpp")] + [
        os.path.join(CSRC, f) for f in ("fp.hpp", "ec.hpp", "fp2l.hpp", "fp2l_mem.hpp", "fp12l.hpp", "pairing_consts.hpp")]
    if not os.path.exists(SHIM_SO) or any(os.path.getmtime(d) > os.path.getmtime(SHIM_SO) for d in deps):
        os.makedirs(os.path.dirname(SHIM_SO), exist_ok=True)
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wall", "-Wno-unknown-pragmas",
                        "-Wl,-Bsymbolic", "-o", SHIM_SO, SHIM_SRC], check=True)
    L = ctypes.CDLL(SHIM_SO)
    vp = ctypes.c_void_p
    L.h_fp12_op.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp]
    L.h_tower_fp2.argtypes = [ctypes.c_int, vp, vp, vp]
    L.h_overflow.argtypes = [ctypes.c_int]
    return L


def run(shim, op, a, b=None, k=0, alias=0, expect_overflow=False):
    """one operation on stored words; returns the stored result after the three class checks"""
    out = (ctypes.c_uint32 * W)()
    shim.h_overflow(1)
    assert shim.h_fp12_op(op, k, alias, out, _arr(a), _arr(b) if b is not None else None) == 0
    over = shim.h_overflow(1)
    if expect_overflow:
        return over
    assert over == 0, ("a range check fired", op, k, alias)
    out = list(out)
    pi.check_stored_S(out)  # limbs 0..12 at most 2^28 - 1, every coordinate below 2p
    return out


def model(op, a, b=None, k=0):
    return {MUL: lambda: pi.f12_mul(a, b), SQR: lambda: pi.f12_sqr(a),
            SPARSE: lambda: pi.f12_mul_sparse(a, b[0], b[1], b[4]), CONJ: lambda: pi.f12_conj(a),
            FROB: lambda: pi.f12_frob(a, k), INV: lambda: pi.f12_inv(a), CSQR: lambda: pi.f12_cyc_sqr(a, k)}[op]()


# (op, k, the aliases its comment in fp12l.hpp allows: 0 separate, 1 d == a, 2 d == b)
UNARY = [(SQR, 0, (0, 1)), (CONJ, 0, (0, 1)), (FROB, 1, (0, 1)), (FROB, 2, (0, 1)), (FROB, 3, (0, 1)), (INV, 0, (0,))]
BINARY = [(MUL, 0, (0, 1, 2)), (SPARSE, 0, (0, 1))]


def check_all_ops(shim, a_words, b_words, what):
    a, b = pi.stored_value(a_words), pi.stored_value(b_words)
    for op, k, aliases in UNARY:
        want = model(op, a, k=k)
        for alias in aliases:
            got = run(shim, op, a_words, k=k, alias=alias)
            assert pi.stored_value(got) == want, (what, op, k, alias)
    for op, k, aliases in BINARY:
        want = model(op, a, b)
        for alias in aliases:
            got = run(shim, op, a_words, b_words, alias=alias)
            assert pi.stored_value(got) == want, (what, op, alias)


@pytest.mark.parametrize("plus_p", [False, True], ids=["canonical", "plus_p"])
def test_special_values_every_op(shim, plus_p):
    """forms (a), (b) and (d): the 13 special values, each against "rand" and against its neighbour"""
    sp = pi.special_list()
    for i, a in enumerate(sp):
        for b in (pi.special_fp12()["rand"], sp[(i + 1) % len(sp)]):
            check_all_ops(shim, pi.stored_words(a, plus_p), pi.stored_words(b, plus_p), (pi.SPECIAL_NAMES[i], plus_p))


@pytest.mark.parametrize("plus_p", [False, True], ids=["canonical", "plus_p"])
def test_random_values_every_op(shim, plus_p):
    vs = pi.random_fp12(4, 0x12a)
    for i in range(0, 4, 2):
        check_all_ops(shim, pi.stored_words(vs[i], plus_p), pi.stored_words(vs[i + 1], not plus_p), (i, plus_p))


def maxlimb_value(seed):
    """form (c): all twelve coordinates the class-S max-limb element (seed None), or random below it"""
    rnd = random.Random(seed) if seed is not None else None
    return sum((_maxlimb(fb.S(), rnd) for _ in range(12)), [])


@pytest.mark.parametrize("seed", [None, 41, 42])
def test_max_limb_coordinates_every_op(shim, seed):
    a = maxlimb_value(seed)
    b = a if seed is None else maxlimb_value(seed + 100)
    assert all(x >= P for x in pi.stored_coords(a))  # above p: no canonical value looks like this
    if seed is None:
        assert all(w == (1 << 28) - 1 for k in range(12) for w in a[k * NL:(k + 1) * NL - 1])
        assert all(x == pi.stored_coords(a)[0] and x + (1 << 364) >= 2 * P for x in pi.stored_coords(a))
    check_all_ops(shim, a, b, ("maxlimb", seed))


@pytest.mark.parametrize("plus_p", [False, True], ids=["canonical", "plus_p"])
def test_cyclotomic_squarings_on_unitary_values(shim, plus_p):
    fs = [pi.special_fp12()["rand"], pi.special_fp12()["line"]] + pi.random_fp12(1, 0xc7c)
    for j, f in enumerate(fs):
        u = pi.unitary(f)
        assert pi.f12_is_one(pi.f12_mul(u, pi.f12_conj(u))) and not pi.f12_is_one(u)
        words = pi.stored_words(u, plus_p)
        for k in CSQR_RUNS:
            want = pi.f12_cyc_sqr(u, k)
            for alias in (0, 1):
                assert pi.stored_value(run(shim, CSQR, words, k=k, alias=alias)) == want, (j, k, alias)


def line_words(T, Q, plus_p):
    return pi.stored_words([T[0], T[1], T[2], Q[0], Q[1], pi.F2_ZERO], plus_p)


def check_line(shim, kind, words, what):
    v = pi.stored_value(words)
    T, Q = tuple(v[:3]), (v[3], v[4])
    T3, l = pi.line_dbl(T) if kind == "dbl" else pi.line_add(T, Q)
    got = pi.stored_value(run(shim, LINE_DBL if kind == "dbl" else LINE_ADD, words))
    assert got == [T3[0], T3[1], T3[2], l[0], l[1], l[2]], what


@pytest.mark.parametrize("plus_p", [False, True], ids=["canonical", "plus_p"])
def test_line_functions_on_miller_points(shim, plus_p):
    cases = pi.miller_line_cases()
    assert [c[0] for c in cases[:5]] == ["dbl", "add", "dbl", "dbl", "add"] and cases[0][1][2] == pi.F2_ONE
    for j, (kind, T, Q) in enumerate(cases):
        check_line(shim, kind, line_words(T, Q, plus_p), (j, kind, plus_p))
    # the addition from an affine T (Z = 1) as well: T = Q_1, Q = Q_0
    q0, q1 = pi.pairs()[0][1], pi.pairs()[1][1]
    check_line(shim, "add", line_words((q1[0], q1[1], pi.F2_ONE), q0, plus_p), ("affine add", plus_p))


@pytest.mark.parametrize("seed", [None, 51, 52])
def test_line_functions_on_max_limb_coordinates(shim, seed):
    """the formulas are plain algebra: no curve point is needed to compare them with the model"""
    if seed is None:  # equal X and U2 would make the addition degenerate: only qx, qy at the exact maximum there
        dbl = maxlimb_value(None)
        add = maxlimb_value(53)
        add[6 * NL:10 * NL] = dbl[6 * NL:10 * NL]
    else:
        dbl = add = maxlimb_value(seed)
    check_line(shim, "dbl", dbl, ("maxlimb dbl", seed))
    check_line(shim, "add", add, ("maxlimb add", seed))


FP2_OPS = {0: pi.f2_add, 1: pi.f2_sub, 2: lambda a, b: pi.f2_add(a, a), 3: lambda a, b: pi.f2_neg(a),
           4: lambda a, b: pi.f2_conj(a), 5: lambda a, b: pi.f2_xi(a), 6: pi.f2_mul, 7: lambda a, b: pi.f2_sqr(a),
           8: lambda a, b: pi.f2_inv(a)}


@pytest.mark.parametrize("seed", [None, 61, 62])
def test_fp2_primitives_of_the_tower_at_class_bounds(shim, seed):
    rnd = random.Random(seed) if seed is not None else None
    r2 = rnd or random.Random(63)
    a = _maxlimb(fb.S(), rnd) + _maxlimb(fb.S(), rnd)
    b = _maxlimb(fb.S(), r2) + _maxlimb(fb.S(), r2)
    dec = lambda w: (_val(w[:NL]) * pi.R392_INV % P, _val(w[NL:]) * pi.R392_INV % P)  # noqa: E731
    shim.h_overflow(1)
    for op in range(10):
        r = (ctypes.c_uint32 * (2 * NL))()
        shim.h_tower_fp2(op, r, _arr(a), _arr(b))
        assert shim.h_overflow(1) == 0, op
        r = list(r)
        assert all(x < (1 << 28) for x in r[:NL - 1] + r[NL:2 * NL - 1]), op
        assert _val(r[:NL]) < 2 * P and _val(r[NL:]) < 2 * P, op
        want = FP2_OPS[op](dec(a), dec(b)) if op < 9 else pi.f2_scale(dec(a), dec(b)[0])
        assert dec(r) == want, op


def test_shim_trips_on_an_operand_outside_class_S(shim):
    """not vacuous: the same product with b in class X (normalized, below 10p: 8p - b goes negative
    in f_mul_bs) sets the overflow flag; with both operands in S it does not"""
    a = maxlimb_value(None)
    bad = sum((_maxlimb(fb.Xc()) for _ in range(12)), [])
    assert all(2 * P <= x < 10 * P for x in pi.stored_coords(bad))
    assert run(shim, MUL, a, bad, expect_overflow=True) != 0
    assert run(shim, SPARSE, a, bad, expect_overflow=True) != 0
    assert run(shim, MUL, a, a, expect_overflow=True) == 0
