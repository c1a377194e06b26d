"""GPU parity of the Fp12 tower and the Miller loop's line functions, one operation at a
time (msm_test_fp12 of the C ABI; csrc/fp12l.hpp, the test kernels of csrc/pairing.hip) on
an MI355X.

Oracle: the plain-integer model of tests/pairing_inputs.py, pinned op by op to the
reference by the "tower" key of tests/golden/pairing.json (tests/test_pairing_host.py).
Every comparison is exact.  raw = 0: blst Fp12 values in and out (in through the
arithmetic of msm_fp12_final_exp's load, out canonical), byte for byte.  raw = 1: the
672-byte stored form in and out untouched, so the test chooses the representative --
(a) canonical, (b) every coordinate plus p, (c) every coordinate the class-S max-limb
element -- and checks the class of what comes back: limbs 0..12 at most 2^28 - 1, every
coordinate below 2p, the value mod p.  The end-to-end pairing tests only ever put
generic values, in whatever representative the previous product left, through these
operations, and an error the final exponentiation absorbs is invisible to them.
"""
import ctypes
import random

import pytest

import fp_bounds as fb
import pairing_inputs as pi
from test_fp_bounds import NL, _maxlimb

pytestmark = pytest.mark.gpu

G, W = pi.FP12_BYTES, pi.FP12S_WORDS
MUL, SQR, SPARSE, CONJ, FROB, INV, CSQR, LINE_DBL, LINE_ADD = range(9)
CSQR_RUNS = (1, 2, 3, 9, 15, 32)  # the run lengths of the final exponentiation's program
# a 128-lane block holds 64 values: a lone pair, the last pair of a block, a full block,
# one pair into the second block, a partial third
COUNTS = [1, 63, 64, 65, 129]
# (op, k, aliases: 0 a destination of its own, 1 d == a, 2 d == b)
UNARY = [(SQR, 0, (0, 1)), (CONJ, 0, (0, 1)), (FROB, 1, (0, 1)), (FROB, 2, (0, 1)), (FROB, 3, (0, 1)), (INV, 0, (0,))]
BINARY = [(MUL, 0, (0, 1, 2)), (SPARSE, 0, (0, 1))]


@pytest.fixture(scope="module")
def L():
    import msm_blst_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible")
    return m.lib()


def model(op, a, b=None, k=0):
    return {MUL: lambda: pi.f12_mul(a, b), SQR: lambda: pi.f12_sqr(a),
            SPARSE: lambda: pi.f12_mul_sparse(a, b[0], b[1], b[4]), CONJ: lambda: pi.f12_conj(a),
            FROB: lambda: pi.f12_frob(a, k), INV: lambda: pi.f12_inv(a), CSQR: lambda: pi.f12_cyc_sqr(a, k)}[op]()


def call_blst(L, op, a, b=None, k=0, alias=0):
    """a, b: lists of Fp12 values -> the list of result values' canonical bytes"""
    n = len(a)
    out = (ctypes.c_uint8 * (n * G))(*([0xa5] * (n * G)))
    ab = b"".join(pi.fp12_bytes(v) for v in a)
    bb = b"".join(pi.fp12_bytes(v) for v in b) if b is not None else None
    assert L.msm_test_fp12(op, k, alias, 0, ab, bb, out, n) == 0, (op, k, alias)
    raw = bytes(out)
    return [raw[i * G:(i + 1) * G] for i in range(n)]


def call_raw(L, op, a, b=None, k=0, alias=0):
    """a, b: lists of 168-word stored values -> the list of stored results, each checked for class S"""
    n = len(a)
    out = (ctypes.c_uint32 * (n * W))(*([0xffffffff] * (n * W)))
    flat = lambda vs: (ctypes.c_uint32 * (n * W))(*[w for v in vs for w in v])  # noqa: E731
    assert L.msm_test_fp12(op, k, alias, 1, flat(a), flat(b) if b is not None else None, out, n) == 0, (op, k, alias)
    out = list(out)
    res = [out[i * W:(i + 1) * W] for i in range(n)]
    for i, r in enumerate(res):
        try:
            pi.check_stored_S(r)  # limbs 0..12 at most 2^28 - 1, every coordinate below 2p
        except AssertionError as e:
            raise AssertionError(f"op {op} k {k} alias {alias} slot {i} of {n}: result outside class S: {e}")
    return res


def differing(got, want):
    return [i for i, (g, w) in enumerate(zip(got, want)) if g != w]


def check_blst(L, a, b, what):
    """every op (the cyclotomic squaring and the lines apart) on the slots of a (and b), blst form"""
    for op, k, aliases in UNARY:
        want = [pi.fp12_bytes(model(op, x, k=k)) for x in a]
        for alias in aliases:
            bad = differing(call_blst(L, op, a, k=k, alias=alias), want)
            assert not bad, f"{what}: op {op} k {k} alias {alias}: slots {bad[:8]} of {len(a)} differ"
    for op, k, aliases in BINARY:
        want = [pi.fp12_bytes(model(op, x, y)) for x, y in zip(a, b)]
        for alias in aliases:
            bad = differing(call_blst(L, op, a, b, alias=alias), want)
            assert not bad, f"{what}: op {op} alias {alias}: slots {bad[:8]} of {len(a)} differ"


def check_raw(L, a, b, what):
    """the same on stored words: class S out (call_raw) and the value mod p"""
    va, vb = [pi.stored_value(x) for x in a], [pi.stored_value(y) for y in b]
    for op, k, aliases in UNARY:
        want = [model(op, x, k=k) for x in va]
        for alias in aliases:
            got = [pi.stored_value(r) for r in call_raw(L, op, a, k=k, alias=alias)]
            bad = differing(got, want)
            assert not bad, f"{what}: op {op} k {k} alias {alias}: slots {bad[:8]} of {len(a)} differ"
    for op, k, aliases in BINARY:
        want = [model(op, x, y) for x, y in zip(va, vb)]
        for alias in aliases:
            got = [pi.stored_value(r) for r in call_raw(L, op, a, b, alias=alias)]
            bad = differing(got, want)
            assert not bad, f"{what}: op {op} alias {alias}: slots {bad[:8]} of {len(a)} differ"


def maxlimb_value(seed):
    """form (c): all twelve coordinates the class-S max-limb element (seed None), or random below it"""
    rnd = random.Random(seed) if seed is not None else None
    return sum((_maxlimb(fb.S(), rnd) for _ in range(12)), [])


RANDOMS = pi.random_fp12(16, 0x70e5)


def test_special_and_random_values_blst_form(L):
    """unary ops on the 13 special values and 16 random ones; binary ops on every special
    with every special (13 x 13) and on the randoms pairwise"""
    sp = pi.special_list()
    assert len(sp) == 13
    a = [x for x in sp for _ in sp] + RANDOMS
    b = [y for _ in sp for y in sp] + RANDOMS[1:] + RANDOMS[:1]
    assert len(a) == 13 * 13 + 16
    check_blst(L, a, b, "specials x specials, randoms")


def test_stored_forms_and_result_class(L):
    """raw = 1: forms (a), (b) of the specials and randoms, form (c) at the exact maximum and
    under two seeds; every result in class S, every value right"""
    vals = pi.special_list() + RANDOMS
    a = [pi.stored_words(v, False) for v in vals] + [pi.stored_words(v, True) for v in vals]
    partner = vals[1:] + vals[:1]
    b = [pi.stored_words(v, True) for v in partner] + [pi.stored_words(v, False) for v in partner]
    mx = [maxlimb_value(None), maxlimb_value(41), maxlimb_value(42)]
    a += mx + [pi.stored_words(pi.special_fp12()["rand"], True)] * 3
    b += [mx[0], maxlimb_value(141), maxlimb_value(142)] + mx
    assert all(w == (1 << 28) - 1 for k in range(12) for w in mx[0][k * NL:(k + 1) * NL - 1])
    check_raw(L, a, b, "stored forms")


@pytest.mark.parametrize("n", COUNTS)
def test_counts_with_distinct_values_in_every_slot(L, n):
    """each slot checked: a lane pair that read its neighbour's component, or a block edge
    handled wrongly, shows as that slot's value"""
    vs = pi.random_fp12(2 * n, 0xc0 + n)
    a, b = vs[:n], vs[n:]
    assert len({pi.fp12_bytes(v) for v in vs}) == 2 * n
    check_blst(L, a, b, f"n={n}")
    us = [pi.unitary(v) for v in a]
    bad = differing(call_blst(L, CSQR, us, k=3), [pi.fp12_bytes(pi.f12_cyc_sqr(u, 3)) for u in us])
    assert not bad, f"n={n}: cyclotomic squarings: slots {bad[:8]} differ"


def test_cyclotomic_squarings_on_unitary_values(L):
    """unitary inputs only (u = conj(f) / f, then u frob2(u)); the subfield specials give one,
    an edge of its own; every run length of the program, in blst form and in both stored forms"""
    us = [pi.unitary(f) for f in pi.special_list() + RANDOMS[:6]]
    assert sum(pi.f12_is_one(u) for u in us) == len(pi.SPECIAL_FE_ONE)
    for k in CSQR_RUNS:
        want = [pi.f12_cyc_sqr(u, k) for u in us]
        for alias in (0, 1):
            bad = differing(call_blst(L, CSQR, us, k=k, alias=alias), [pi.fp12_bytes(w) for w in want])
            assert not bad, f"k {k} alias {alias}: slots {bad[:8]} differ"
            for plus_p in (False, True):
                got = call_raw(L, CSQR, [pi.stored_words(u, plus_p) for u in us], k=k, alias=alias)
                bad = differing([pi.stored_value(r) for r in got], want)
                assert not bad, f"k {k} alias {alias} plus_p {plus_p}: slots {bad[:8]} differ"


def line_value(T, Q):
    return [T[0], T[1], T[2], Q[0], Q[1], pi.F2_ZERO]


def line_want(kind, v):
    T3, l = pi.line_dbl(tuple(v[:3])) if kind == "dbl" else pi.line_add(tuple(v[:3]), (v[3], v[4]))
    return [T3[0], T3[1], T3[2], l[0], l[1], l[2]]


def test_line_functions(L):
    """the running points of the first three steps of the Miller loop for pairs 0 and 1 (the
    first is T = Q with Z = 1), an addition from an affine T, in blst form and in both stored
    representatives; then max-limb coordinates (plain algebra: no curve point needed)"""
    cases = pi.miller_line_cases()
    q0, q1 = pi.pairs()[0][1], pi.pairs()[1][1]
    cases.append(("add", (q1[0], q1[1], pi.F2_ONE), q0))
    assert cases[0][0] == "dbl" and cases[0][1][2] == pi.F2_ONE and len(cases) == 11
    for kind, op in (("dbl", LINE_DBL), ("add", LINE_ADD)):
        vals = [line_value(T, Q) for kd, T, Q in cases if kd == kind]
        want = [line_want(kind, v) for v in vals]
        bad = differing(call_blst(L, op, vals), [pi.fp12_bytes(w) for w in want])
        assert not bad, f"{kind}: slots {bad} differ"
        for plus_p in (False, True):
            got = call_raw(L, op, [pi.stored_words(v, plus_p) for v in vals])
            bad = differing([pi.stored_value(r) for r in got], want)
            assert not bad, f"{kind} plus_p {plus_p}: slots {bad} differ"
        mx = [maxlimb_value(51), maxlimb_value(52)]
        if kind == "dbl":
            mx.append(maxlimb_value(None))
        else:  # (equal X and U2 would make the addition degenerate: only qx, qy at the exact maximum)
            m = maxlimb_value(53)
            m[3 * 2 * NL:5 * 2 * NL] = maxlimb_value(None)[3 * 2 * NL:5 * 2 * NL]
            mx.append(m)
        got = call_raw(L, op, mx)
        bad = differing([pi.stored_value(r) for r in got], [line_want(kind, pi.stored_value(m)) for m in mx])
        assert not bad, f"{kind} max-limb: slots {bad} differ"
