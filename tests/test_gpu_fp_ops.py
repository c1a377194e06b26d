"""The Fp, Fp2, lane-pair and xyzz layers (csrc/fp.hpp, fp2l.hpp, ec.hpp, coop.hpp) on an
MI355X, one operation per launch on raw stored limbs (msm_test_fp_ops of the C ABI), at
the bounds of the range classes DESIGN 4a proves.

The interval model (tests/fp_bounds.py) proves the classes and the host build of the same
headers runs them at their max-limb representatives (tests/test_fp_bounds.py), but the
host build shares none of what differs on the device: the v_mad_u64_u32 columns, pair_swap
as a DPP move under a partial EXEC mask, the pins of MulChain, the selects, the register
allocation.  Here the device code gets the same operands.

Oracle: plain integers mod p (Montgomery products a b R^-1, R = 2^392) and the xyzz
algebra of tests/test_fp_bounds.py (_ref_madd / _ref_add / _ref_dbl).  Every comparison is
exact.  Each result is checked for its value and for the class the code documents:
products and reductions in S (limbs 0..12 at most 2^28 - 1, below 2p), fp_red / fp_nred
below the bound of fb.red_report(), fp_canon below p, a stored x normalized and below 10p,
lazy results limb for limb as integers (which is more than the value mod p) with limbs
below 2^31 and the value bound the host test asserts.  Every operand class is checked
against the interval model first (prove()), so no case runs an op outside what is proved.

Slot i of a launch takes, by i % 6: the exact max-limb representative of each operand's
class, three random representatives just below it, a canonical edge value (0, 1, p - 1,
the Montgomery one, ...; for Fp2 a value with one component zero), a random canonical
value; the op's class combinations rotate every six slots.  Shapes reach the block edges:
64-thread one-lane blocks, 32 values per lane-pair block, 64 (G1) / 32 (G2) sums per
cooperative block.  The out buffer is longer than n and pre-filled; what lies past n must
come back untouched.
"""
import ctypes
import functools
import random
from fractions import Fraction

import pytest

import fp_bounds as fb
from test_fp_bounds import NL, M28, P, RINV, _F, _limbs, _maxlimb, _ref_add, _ref_dbl, _ref_madd, _val

pytestmark = pytest.mark.gpu

FP, FP2, FP2L = 0, 1, 2
SPLIT, CHAIN = 0, 1
FIELD_NAME = {FP: "Fp", FP2: "Fp2", FP2L: "Fp2L"}
(F_MUL, F_MUL_BS, F_SQR, F_MUL_SUB, F_MUL_SUB_BS, F_ADD, F_SUB4, F_SUB16, F_SUB8, F_SUB32, F_SUB_2X, F_NEG4, F_MUL3,
 F_NORM, F_NRED, F_ONE, F_IS_ZERO_EXACT, F_IS_ZERO_S, FP_MUL2, FP_MUL4, FP_RED, FP_CNEG4, FP_CANON, FP_CSUB_P,
 XYZZ_MADD, XYZZ_ADD, XYZZ_ADD_U1S1, XYZZ_DBL, COOP_ADD) = range(29)
OP_NAME = ("f_mul f_mul_bs f_sqr f_mul_sub f_mul_sub_bs f_add f_sub4 f_sub16 fp_sub<8> fp_sub<32> f_sub_2x f_neg4 "
           "f_mul3 f_norm f_nred f_one f_is_zero_exact f_is_zero_S fp_mul2 fp_mul4 fp_red fp_cneg4 fp_canon "
           "fp_csub_p xyzz_madd xyzz_add xyzz_add_u1s1 xyzz_dbl coop_xyzz_add").split()
NEG, ACC_AFFINE, ACC_NEG = 1, 2, 4
ONE = fb.R % P
SENTINEL = 0xa5a5a5a5
PAD = 3  # slots past n in every out buffer

ONE_LANE_N = [1, 63, 64, 65, 129]   # 64-thread blocks, one value per lane
PAIR_N = [1, 31, 32, 33, 65]        # 32 values per block
COOP_N = {FP: [1, 63, 64, 65], FP2L: [1, 31, 32, 33]}
# (field, form): every way a formula or a product is compiled
KINDS = [(FP, SPLIT), (FP, CHAIN), (FP2, SPLIT), (FP2L, SPLIT)]
KIND_ID = ["Fp-split", "Fp-chain", "Fp2", "Fp2L"]


def counts(field):
    return PAIR_N if field == FP2L else ONE_LANE_N


def ncomp(field):
    return 1 if field == FP else 2


@pytest.fixture(scope="module")
def L():
    import msm_blst_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible")
    return m.lib()


# ------------------------------------------------------------ operand classes ----
S = fb.S()
X = fb.Xc()
CAN = fb.canonical()
LAZY6 = fb.sub(S, S)                      # U2 - U1, S2 - Y1: < 6p, limbs < 3 2^28
LAZY18 = fb.sub(S, X, 16)                 # S - X + 16p: < 18p
LAZY14 = fb.norm(fb.sub(fb.norm(fb.sub(fb.norm(fb.sub(S, S)), S)), S))
MUL3S = fb.mul3(S)
X3RAW = fb.sub2x(S, S, S)                 # R^2 + 8p - PPP - 2Q before f_norm: limbs < 2^31
RED32 = fb.Iv([M28] * NL, 32 * P - 1)     # the normalized < 32p input of fp_red
MPLUSM = fb.add(S, S)                     # m + m of the Fp2 square: limbs < 2^29
NEG4S = fb.neg(S, 4)
NEG8S = fb.neg(S, 8)
N18 = fb.norm(LAZY18)
SUBTRAHEND = {8: fb.Iv([M28] * (NL - 1) + [fb.SUB[8][NL - 1]], 8 * P - 1),
              32: fb.Iv([M28] * (NL - 1) + [fb.SUB[32][NL - 1]], 32 * P - 1)}


@functools.lru_cache(maxsize=None)
def red_bound():
    """the largest fp_red / fp_nred result of the DESIGN 4a table (fb.red_report() gives it as a
    multiple of p, a float: rounded up).  Not at import: the model walks every top limb."""
    bound = int(Fraction(max(vout for _, _, vout in fb.red_report())) * P) + (P >> 48)
    assert bound < 2 * P
    return bound


EDGES = [0, 1, P - 1, ONE, 2]
EDGES_S = [0, P, P + 1, P - 1, 2 * P - 1, 1]   # normalized, below 2p: the zero tests, fp_canon, fp_csub_p


def elem(field, iv, i, salt, edges=EDGES):
    """slot i's representative of class iv: see the module docstring"""
    kind, out = i % 6, []
    for c in range(ncomp(field)):
        rnd = random.Random(f"{salt}/{i}/{c}")
        if kind == 0:
            out += _maxlimb(iv)
        elif kind <= 3:
            out += _maxlimb(iv, rnd)
        elif kind == 4:
            out += _limbs(edges[(i // 6 + 2 * c + sum(map(ord, salt))) % len(edges)])
        else:
            out += _limbs(rnd.randrange(P))
    return out


def comps(field, words):
    """the integer value of each component, as stored (not reduced)"""
    return tuple(_val(words[c * NL:(c + 1) * NL]) for c in range(ncomp(field)))


def modp(v):
    return tuple(x % P for x in v)


def fmul(a, b):
    """Montgomery product of two component tuples mod p"""
    if len(a) == 1:
        return (a[0] * b[0] * RINV % P,)
    return ((a[0] * b[0] - a[1] * b[1]) * RINV % P, (a[0] * b[1] + a[1] * b[0]) * RINV % P)


def fsub(a, b):
    return tuple((x - y) % P for x, y in zip(a, b))


# ---------------------------------------------------------------- the entry ----
def call(L, field, form, op, values, n, nin, nout, flags=None):
    """values: n lists of nin elements (word lists) -> n results (word lists; one word for
    nout = 0); checks the status and that the PAD slots past n came back untouched"""
    w = NL * ncomp(field)
    ow = nout * w if nout else 1
    assert len(values) == n and all(len(v) == nin and all(len(e) == w for e in v) for v in values)
    flat = [x for v in values for e in v for x in e]
    inp = (ctypes.c_uint32 * max(1, len(flat)))(*flat)
    fl = (ctypes.c_uint32 * n)(*flags) if flags is not None else None
    cap = n + PAD
    out = (ctypes.c_uint32 * (cap * ow))(*([SENTINEL] * (cap * ow)))
    what = f"{OP_NAME[op]} {FIELD_NAME[field]} form {form} n {n}"
    assert L.msm_test_fp_ops(field, form, op, inp if nin else None, fl, out, n, cap) == 0, \
        f"{what}: {L.msm_last_error()}"
    out = list(out)
    assert out[n * ow:] == [SENTINEL] * (PAD * ow), f"{what}: a slot past n was written"
    return [out[i * ow:(i + 1) * ow] for i in range(n)]


def fail_slots(what, bad, n):
    assert not bad, f"{what} n {n}: slots {[b[0] for b in bad[:8]]} of {n} differ; first: {bad[0]}"


def normalized(words):
    return all(all(x <= M28 for x in words[c:c + NL - 1]) for c in range(0, len(words), NL))


# ------------------------------------------------------------ the field ops ----
def prove(fn, *ivs):
    """the interval model accepts the op on these classes (fb.RangeError if not)"""
    fn(*ivs)
    return ivs


def _mul_sub_fp(a, b, c, d):
    return fb.mul2(a, b, c, fb.neg(d, 4))


def _mul_fp2(a, b):
    return fb.mul2_fp2(a, b)


def _sqr_any(a):
    fb.sqr(a), fb.sqr_fp2(a), fb.sqr_fp2l(a)


def _mul_sub_any(a, b, c, d):
    _mul_sub_fp(a, b, c, d), fb.mul_sub_fp2(a, b, c, d)


def _mul_any(a, b):
    fb.mul(a, b), _mul_fp2(a, b)


def _mul_bs_any(a, b):
    fb.mul(a, b), fb.mul_bs_fp2(a, b)


def _mul_sub_bs_any(a, b, c, d):   # b normalized already; c may be in class X (ec.hpp xyzz_add_regrouped)
    assert all(l <= M28 for l in b.lim[:NL - 1])
    _mul_sub_fp(a, b, c, d), fb.mul_sub_fp2(a, b, c, d)


def _sub(K):
    return lambda a, b: fb.sub(a, b, K)


# op -> (operand count, class combinations, each proved by the model for every field that runs it)
PRODUCTS = {
    F_MUL: (2, [prove(_mul_any, LAZY6, S), prove(_mul_any, LAZY6, LAZY6), prove(_mul_any, CAN, S),
                prove(_mul_any, LAZY18, S), prove(_mul_any, X, S)]),
    F_MUL_BS: (2, [prove(_mul_bs_any, LAZY6, S), prove(_mul_bs_any, LAZY18, S), prove(_mul_bs_any, CAN, S),
                   prove(_mul_bs_any, X, S)]),
    F_SQR: (1, [prove(_sqr_any, LAZY6), prove(_sqr_any, MUL3S), prove(_sqr_any, LAZY18), prove(_sqr_any, S)]),
    F_MUL_SUB: (4, [prove(_mul_sub_any, LAZY6, LAZY6, S, S), prove(_mul_sub_any, LAZY18, LAZY6, S, S),
                    prove(_mul_sub_any, LAZY18, MUL3S, S, S)]),
    F_MUL_SUB_BS: (4, [prove(_mul_sub_bs_any, X, S, X, S), prove(_mul_sub_bs_any, LAZY18, S, S, S)]),
    FP_MUL2: (4, [prove(fb.mul2, LAZY6, LAZY6, S, NEG4S), prove(fb.mul2, LAZY18, LAZY6, S, NEG4S),
                  prove(fb.mul2, X, S, X, NEG4S)]),
    # the two sums of f_mul_sub(Fp2): a0 b0 + a1 (8p - b1) + c0 (8p - d0) + c1 d1 and its c1 twin
    FP_MUL4: (8, [prove(fb.mul4, LAZY18, fb.norm(LAZY6), LAZY18, fb.neg(fb.norm(LAZY6), 8), S, NEG8S, S, S),
                  prove(fb.mul4, LAZY18, fb.norm(LAZY6), LAZY18, fb.norm(LAZY6), S, NEG8S, S, NEG8S),
                  prove(fb.mul4, LAZY6, fb.norm(MUL3S), LAZY6, fb.neg(fb.norm(MUL3S), 8), X, NEG8S, X, S)]),
}
LAZIES = {
    F_ADD: (2, [prove(fb.add, S, S), prove(fb.add, LAZY6, S)]),
    F_SUB4: (2, [prove(_sub(4), LAZY6, S), prove(_sub(4), S, S)]),
    F_SUB16: (2, [prove(_sub(16), S, X)]),
    F_SUB8: (2, [prove(_sub(8), LAZY6, SUBTRAHEND[8]), prove(_sub(8), S, S)]),
    F_SUB32: (2, [prove(_sub(32), N18, N18), prove(_sub(32), S, SUBTRAHEND[32])]),
    F_SUB_2X: (3, [prove(fb.sub2x, S, S, S)]),
    F_NEG4: (1, [prove(fb.neg, S)]),
    F_MUL3: (1, [prove(fb.mul3, S)]),
    F_NORM: (1, [prove(fb.norm, X3RAW), prove(fb.norm, LAZY6), prove(fb.norm, LAZY18)]),
}


@functools.lru_cache(maxsize=None)
def reductions(op):
    if op == F_NRED:
        return [prove(fb.nred, NEG4S), prove(fb.nred, LAZY14), prove(fb.nred, X3RAW), prove(fb.nred, LAZY18)]
    return [prove(fb.red, RED32), prove(fb.red, MPLUSM), prove(fb.red, fb.norm(X3RAW))]



def operands(field, op, combos, nin, n, edges=EDGES):
    return [[elem(field, combos[(i // 6) % len(combos)][j], i, f"{op}/{j}", edges) for j in range(nin)]
            for i in range(n)]


def product_want(op, v):
    if op in (F_MUL, F_MUL_BS):
        return fmul(v[0], v[1])
    if op == F_SQR:
        return fmul(v[0], v[0])
    if op in (F_MUL_SUB, F_MUL_SUB_BS):
        return fsub(fmul(v[0], v[1]), fmul(v[2], v[3]))
    if op == FP_MUL2:
        return ((v[0][0] * v[1][0] + v[2][0] * v[3][0]) * RINV % P,)
    return (sum(v[2 * k][0] * v[2 * k + 1][0] for k in range(4)) * RINV % P,)


def run_products(L, field, form, op):
    """-> {n: results}: value mod p and class S of every slot"""
    nin, combos = PRODUCTS[op]
    res = {}
    for n in counts(field):
        vals = operands(field, op, combos, nin, n)
        got = call(L, field, form, op, vals, n, nin, 1)
        bad = []
        for i, (v, g) in enumerate(zip(vals, got)):
            want = product_want(op, [comps(field, e) for e in v])
            gv = comps(field, g)
            if modp(gv) != want or not normalized(g) or max(gv) >= 2 * P:
                bad.append((i, "value" if modp(gv) != want else "class S", g))
        fail_slots(f"{OP_NAME[op]} {FIELD_NAME[field]} form {form}", bad, n)
        res[n] = got
    return res


FIELD_PRODUCTS = [F_MUL, F_MUL_BS, F_SQR, F_MUL_SUB, F_MUL_SUB_BS]


@pytest.mark.parametrize("op", FIELD_PRODUCTS + [FP_MUL2, FP_MUL4], ids=lambda o: OP_NAME[o])
def test_fp_products_both_column_forms(L, op):
    """Fp: split columns against the integers, and the single chain equal to them word for word"""
    split = run_products(L, FP, SPLIT, op)
    chain = run_products(L, FP, CHAIN, op)
    for n in split:
        bad = [(i, s, c) for i, (s, c) in enumerate(zip(split[n], chain[n])) if s != c]
        fail_slots(f"{OP_NAME[op]} Fp: MulChain differs from MulSplit", bad, n)


@pytest.mark.parametrize("field", [FP2, FP2L], ids=["Fp2", "Fp2L"])
@pytest.mark.parametrize("op", FIELD_PRODUCTS, ids=lambda o: OP_NAME[o])
def test_fp2_products(L, field, op):
    if field == FP2 and op == F_MUL_SUB_BS:  # fp.hpp has none over the one-lane Fp2: the entry says so
        w = (ctypes.c_uint32 * (4 * 2 * NL))()
        assert L.msm_test_fp_ops(FP2, SPLIT, op, w, None, w, 1, 1) == -1
        return
    run_products(L, field, SPLIT, op)


def lazy_want(op, v):
    """the exact integer each component must hold"""
    K = {F_SUB4: 4, F_SUB16: 16, F_SUB8: 8, F_SUB32: 32}.get(op)
    if K:
        return tuple(a + K * P - b for a, b in zip(v[0], v[1]))
    if op == F_ADD:
        return tuple(a + b for a, b in zip(v[0], v[1]))
    if op == F_SUB_2X:
        return tuple(a + 8 * P - b - 2 * c for a, b, c in zip(*v))
    if op == F_NEG4:
        return tuple(4 * P - a for a in v[0])
    if op == F_MUL3:
        return tuple(3 * a for a in v[0])
    return v[0]  # f_norm


# the value bound the host test asserts for the same op (tests/test_fp_bounds.py), as a multiple of p
LAZY_BOUND = {F_SUB4: 10, F_SUB_2X: 18, F_SUB16: 18}


@pytest.mark.parametrize("field", [FP, FP2, FP2L], ids=["Fp", "Fp2", "Fp2L"])
@pytest.mark.parametrize("op", sorted(LAZIES), ids=lambda o: OP_NAME[o])
def test_lazy_ops(L, field, op):
    nin, combos = LAZIES[op]
    for n in counts(field):
        vals = operands(field, op, combos, nin, n)
        got = call(L, field, SPLIT, op, vals, n, nin, 1)
        bad = []
        for i, (v, g) in enumerate(zip(vals, got)):
            gv = comps(field, g)
            ok = gv == lazy_want(op, [comps(field, e) for e in v]) and all(x < (1 << 31) for x in g)
            if op in LAZY_BOUND:
                ok = ok and max(gv) < LAZY_BOUND[op] * P
            if op == F_NORM:
                ok = ok and normalized(g)
            if not ok:
                bad.append((i, g))
        fail_slots(f"{OP_NAME[op]} {FIELD_NAME[field]}", bad, n)


@pytest.mark.parametrize("field,op", [(FP, F_NRED), (FP2, F_NRED), (FP2L, F_NRED), (FP, FP_RED)],
                         ids=["Fp-nred", "Fp2-nred", "Fp2L-nred", "fp_red"])
def test_reductions(L, field, op):
    for n in counts(field):
        vals = operands(field, op, reductions(op), 1, n)
        got = call(L, field, SPLIT, op, vals, n, 1, 1)
        bad = []
        for i, (v, g) in enumerate(zip(vals, got)):
            gv = comps(field, g)
            if modp(gv) != modp(comps(field, v[0])) or not normalized(g) or max(gv) > red_bound():
                bad.append((i, g))
        fail_slots(f"{OP_NAME[op]} {FIELD_NAME[field]}", bad, n)


@pytest.mark.parametrize("field", [FP, FP2, FP2L], ids=["Fp", "Fp2", "Fp2L"])
def test_f_one(L, field):
    want = _limbs(ONE) + ([0] * NL if field != FP else [])  # Fp2L: the odd lane comes out zero
    for n in counts(field):
        got = call(L, field, SPLIT, F_ONE, [[] for _ in range(n)], n, 0, 1)
        fail_slots(f"f_one {FIELD_NAME[field]}", [(i, g) for i, g in enumerate(got) if g != want], n)


def test_fp_canon_csub_p_cneg4(L):
    for n in ONE_LANE_N:
        # fp_canon: any legal product input, and the normalized edges around p
        vals = operands(FP, FP_CANON, [(LAZY6,), (LAZY18,), (S,), (MUL3S,)], 1, n, EDGES_S)
        got = call(L, FP, SPLIT, FP_CANON, vals, n, 1, 1)
        bad = [(i, g) for i, (v, g) in enumerate(zip(vals, got))
               if _val(g) != _val(v[0]) % P or not normalized(g)]
        fail_slots("fp_canon", bad, n)
        # fp_csub_p: class S in, canonical out
        vals = operands(FP, FP_CSUB_P, [(S,)], 1, n, EDGES_S)
        got = call(L, FP, SPLIT, FP_CSUB_P, vals, n, 1, 1)
        bad = [(i, g) for i, (v, g) in enumerate(zip(vals, got)) if _val(g) != _val(v[0]) % P or not normalized(g)]
        fail_slots("fp_csub_p", bad, n)
        # fp_cneg4: the flag varies from lane to lane
        vals = operands(FP, FP_CNEG4, [(S,)], 1, n)
        flags = [(i ^ (i >> 3)) & 1 for i in range(n)]
        got = call(L, FP, SPLIT, FP_CNEG4, vals, n, 1, 1, flags)
        bad = [(i, g) for i, (v, g, f) in enumerate(zip(vals, got, flags))
               if g != ([a - b for a, b in zip(fb.SUB[4], v[0])] if f else v[0])]
        fail_slots("fp_cneg4", bad, n)


# ---------------------------------------------------------------- zero tests ----
def zero_cases(field):
    """stored elements around 0 and p, normalized and below 2p: the verdict is the whole value's"""
    if field == FP:
        return [_limbs(v) for v in EDGES_S]
    nz = _maxlimb(S)
    z = {"0": _limbs(0), "p": _limbs(P), "nz": nz, "p+1": _limbs(P + 1), "1": _limbs(1), "2p-1": _limbs(2 * P - 1)}
    pairs = [("0", "0"), ("0", "nz"), ("nz", "0"), ("p", "0"), ("0", "p"), ("p", "p"), ("p+1", "0"), ("0", "1"),
             ("nz", "nz"), ("2p-1", "p"), ("p", "p+1")]
    return [z[a] + z[b] for a, b in pairs]


@pytest.mark.parametrize("field", [FP, FP2, FP2L], ids=["Fp", "Fp2", "Fp2L"])
def test_zero_tests(L, field):
    cases = zero_cases(field)
    for n in counts(field):
        vals = [[cases[(i + n) % len(cases)]] for i in range(n)]
        for op in (F_IS_ZERO_EXACT, F_IS_ZERO_S):
            got = call(L, field, SPLIT, op, vals, n, 1, 0)
            bad = []
            for i, (v, g) in enumerate(zip(vals, got)):
                c = comps(field, v[0])
                want = all(x == 0 for x in c) if op == F_IS_ZERO_EXACT else all(x % P == 0 for x in c)
                if g != [int(want)]:
                    bad.append((i, g, c))
            fail_slots(f"{OP_NAME[op]} {FIELD_NAME[field]}", bad, n)


@pytest.mark.parametrize("field", [FP, FP2, FP2L], ids=["Fp", "Fp2", "Fp2L"])
def test_zero_valued_product_is_zero_S(L, field):
    """a product of a zero-valued lazy operand comes out as 0 or as p; f_is_zero_S says yes to both"""
    n = counts(field)[-1]
    zeros = [_limbs(0), _limbs(P), list(fb.SUB[4]), _limbs(5 * P), [a + b for a, b in zip(fb.SUB[4], _limbs(P))]]
    vals = []
    for i in range(n):
        a = sum((zeros[(i + 2 * c) % len(zeros)] for c in range(ncomp(field))), [])
        vals.append([a, elem(field, S, i, "zprod")])
    prods = call(L, field, SPLIT, F_MUL, vals, n, 2, 1)
    for i, g in enumerate(prods):
        assert all(x in (0, P) for x in comps(field, g)) and normalized(g), (i, g)
    assert any(P in comps(field, g) for g in prods), "no product came out as p: the case is not exercised"
    got = call(L, field, SPLIT, F_IS_ZERO_S, [[g] for g in prods], n, 1, 0)
    assert got == [[1]] * n, [i for i, g in enumerate(got) if g != [1]][:8]


# ------------------------------------------------------------ the xyzz formulas ----
def algebra(field):
    return _F(1 if field == FP else 2)


def dec(field, words):
    c = modp(comps(field, words))
    return c[0] if field == FP else c


def pt_dec(field, pt):
    return tuple(dec(field, e) for e in pt)


def is_inf(pt):
    return all(x == 0 for x in pt[3])


def one_elem(field):
    return _limbs(ONE) + ([0] * NL if field != FP else [])


def zero_elem(field):
    return [0] * (NL * ncomp(field))


def xyzz(field, i, salt, cx=X):
    """a stored point at its class bounds: x in class X, the rest in S (not on the curve: the
    formulas are algebraic and the oracle is the same algebra)"""
    return [elem(field, cx, i, salt + "x")] + [elem(field, S, i, salt + c) for c in ("y", "zzz", "zz")]


def affine(field, i, salt):
    return [elem(field, CAN, i, salt + "x"), elem(field, CAN, i, salt + "y")]


def rep_of(field, value, top, i):
    """a normalized representative value + k p below top p of each component of a value mod p,
    k as large as it goes on the even slots"""
    v = (value,) if field == FP else value
    out = []
    for c, x in enumerate(v):
        k = (top * P - 1 - x) // P
        out += _limbs(x + (k if (i + c) % 2 == 0 else k // 2) * P)
    return out


def scaled(field, base, zzz, zz, i, sign=1):
    """(x, y) seen through (zzz, zz): X = x zz in class X, Y = +-y zzz in S, at their bounds"""
    F = algebra(field)
    x, y = dec(field, base[0]), dec(field, base[1])
    Xv = F.mul(x, dec(field, zz))
    Yv = F.mul(y, dec(field, zzz))
    if sign < 0:
        Yv = F.neg(Yv)
    return [rep_of(field, Xv, 10, i), rep_of(field, Yv, 2, i), zzz, zz]


def inf_point(field):
    return [zero_elem(field)] * 4


SPECIALS = ["acc_inf", "b_inf", "dbl", "cancel"]


def special_slots(n, block, variant, kinds):
    """{slot: kind}: slot 0, the middle of the first block, its last slot (and the slot after the
    middle), the kinds rotating with the variant so that each visits each place"""
    last = min(n, block) - 1
    places = [0, last // 2, last, last // 2 + 1]
    return {s: kinds[(variant + j) % len(kinds)] for j, s in enumerate(places) if s < n}


def want_point(field, got, want, xbound=10):
    """'' if the stored result is the expected one, in its classes"""
    if want[0] == "words":
        return "" if got == want[1] else "not the operand, word for word"
    if want[0] == "inf":
        return "" if all(x == 0 for e in got for x in e) else "not the all-zero infinity"
    if pt_dec(field, got) != want[1]:
        return "value"
    if not all(normalized(e) for e in got):
        return "limbs not normalized"
    if max(comps(field, got[0])) >= xbound * P or any(max(comps(field, e)) >= 2 * P for e in got[1:]):
        return "x above 10p or y, zzz, zz above 2p"
    return ""


def ref_add(field, a, b, style):
    """xyzz_add as ec.hpp / coop.hpp order it.  style 'regrouped' and 'coop' double the untouched
    accumulator, 'u1s1' the rewritten one (U1, S1, ZZZ1 ZZZ2, ZZ1 ZZ2); 'raw_u1s1' has no infinity test"""
    F = algebra(field)
    if style != "raw_u1s1":
        if is_inf(b):
            return ("words", a)
        if is_inf(a):
            return ("words", b)
    A, B = pt_dec(field, a), pt_dec(field, b)
    U1, S1 = F.mul(A[0], B[3]), F.mul(A[1], B[2])
    Pd, Rd = F.sub(F.mul(B[0], A[3]), U1), F.sub(F.mul(B[1], A[2]), S1)
    if Pd == F.zero():
        if Rd != F.zero():
            return ("inf",)
        if style in ("regrouped", "coop"):
            return ("val", _ref_dbl(F, A))
        return ("val", _ref_dbl(F, (U1, S1, F.mul(A[2], B[2]), F.mul(A[3], B[3]))))
    return ("val", _ref_add(F, A, B))


def add_inputs(field, n, variant, block, salt, infinities=True):
    """n (acc, b) pairs at class bounds with the special slots of this variant"""
    kinds = SPECIALS if infinities else ["dbl", "cancel"]
    sp = special_slots(n, block, variant, kinds)
    out = []
    for i in range(n):
        a, b = xyzz(field, i, f"{salt}/{variant}/a"), xyzz(field, i, f"{salt}/{variant}/b")
        kind = sp.get(i)
        if kind == "acc_inf":
            a = inf_point(field)
        elif kind == "b_inf":
            b = inf_point(field)
            if variant & 1:
                a = inf_point(field)  # both at infinity
        elif kind in ("dbl", "cancel"):
            sign = 1 if kind == "dbl" else -1
            if variant >= 2 and kind == "dbl":
                b = [list(e) for e in a]  # the very same words
            else:  # the same point seen through other (zzz, zz), every coordinate at its bound
                base = affine(field, i, f"{salt}/base")
                a = scaled(field, base, a[2], a[3], i)
                b = scaled(field, base, b[2], b[3], i + 1, sign)
        out.append((a, b))
    return out


def run_adds(L, field, form, op, style, ns, block):
    res = {}
    for n in ns:
        for variant in range(4):
            pairs = add_inputs(field, n, variant, block, OP_NAME[op], infinities=style != "raw_u1s1")
            got = call(L, field, form, op, [a + b for a, b in pairs], n, 8, 4)
            w = NL * ncomp(field)
            bad = []
            for i, ((a, b), g) in enumerate(zip(pairs, got)):
                g = [g[k * w:(k + 1) * w] for k in range(4)]
                why = want_point(field, g, ref_add(field, a, b, style))
                if why:
                    bad.append((i, why, g))
            fail_slots(f"{OP_NAME[op]} {FIELD_NAME[field]} form {form} variant {variant}", bad, n)
            res[n, variant] = got
    return res


def add_style(field, op):
    if op == XYZZ_ADD_U1S1:
        return "raw_u1s1"
    return "u1s1" if field == FP2 else "regrouped"  # ec.hpp AddRegrouped: the one-lane Fp2 keeps the u1s1 add


@pytest.mark.parametrize("op", [XYZZ_ADD, XYZZ_ADD_U1S1], ids=lambda o: OP_NAME[o])
@pytest.mark.parametrize("field", [FP, FP2, FP2L], ids=["Fp", "Fp2", "Fp2L"])
def test_xyzz_add(L, field, op):
    block = 32 if field == FP2L else 64
    split = run_adds(L, field, SPLIT, op, add_style(field, op), counts(field), block)
    if field == FP:
        chain = run_adds(L, field, CHAIN, op, add_style(field, op), counts(field), block)
        assert chain == split, f"{OP_NAME[op]} Fp: MulChain differs from MulSplit at {[k for k in split if split[k] != chain[k]]}"


@pytest.mark.parametrize("field", [FP, FP2L], ids=["G1", "G2"])
def test_cooperative_add(L, field):
    """coop_xyzz_add through k_pair_step_c<1> / k_pair_step_c2p: inactive lanes still run the
    three barriers; equal, opposite and infinite inputs at slot 0, mid block and the last slot"""
    run_adds(L, field, SPLIT, COOP_ADD, "coop", COOP_N[field], 64 if field == FP else 32)


def ref_madd(field, acc, p, flags):
    F = algebra(field)
    x2, y2 = dec(field, p[0]), dec(field, p[1])
    one = dec(field, one_elem(field))
    if flags & ACC_AFFINE:
        A = (dec(field, acc[0]), F.neg(dec(field, acc[1])) if flags & ACC_NEG else dec(field, acc[1]), one, one)
    elif is_inf(acc):
        return ("val", (x2, F.neg(y2) if flags & NEG else y2, one, one))
    else:
        A = pt_dec(field, acc)
    ys = F.neg(y2) if flags & NEG else y2
    if F.sub(F.mul(x2, A[3]), A[0]) == F.zero():
        if F.sub(F.mul(ys, A[2]), A[1]) == F.zero():
            return ("val", _ref_dbl(F, A))
        return ("inf",)
    return ("val", _ref_madd(F, A, (x2, y2), bool(flags & NEG)))


def madd_inputs(field, n, variant, block):
    sp = special_slots(n, block, variant, ["acc_inf", "dbl", "cancel"])
    out = []
    for i in range(n):
        # both flags alternate from value to value (lane to lane; Fp2L: pair to pair), in every combination
        fl = ((i + variant) & 1) * NEG | ((i >> 1) & 1) * ACC_AFFINE | ((i >> 2) & 1) * ACC_NEG
        acc = xyzz(field, i, f"madd/{variant}/a", CAN if fl & ACC_AFFINE else X)
        if fl & ACC_AFFINE:
            acc[1] = elem(field, CAN, i, f"madd/{variant}/ay")
        p = affine(field, i, f"madd/{variant}/p")
        kind = sp.get(i)
        if kind == "acc_inf":
            fl &= ~ACC_AFFINE
            acc = inf_point(field)
        elif kind in ("dbl", "cancel"):
            same = kind == "dbl"
            if fl & ACC_AFFINE:  # a bucket's first entry +-P meets +-P again
                acc[0], acc[1] = p[0], p[1]
                fl = fl & ~NEG | (NEG if bool(fl & ACC_NEG) == same else 0)
            else:
                acc = scaled(field, p, acc[2], acc[3], i, 1 if bool(fl & NEG) != same else -1)
                # (x2 zz1, +-y2 zzz1) against +-y2: same sign doubles, opposite cancels
        out.append((acc, p, fl))
    return out


@pytest.mark.parametrize("field,form", KINDS, ids=KIND_ID)
def test_xyzz_madd(L, field, form):
    """neg and acc_affine on and off inside one launch, an accumulator at infinity, the doubling
    and the cancelling branch at class bounds"""
    block = 32 if field == FP2L else 64
    w = NL * ncomp(field)
    for n in counts(field):
        for variant in range(4):
            cases = madd_inputs(field, n, variant, block)
            got = call(L, field, form, XYZZ_MADD, [a + p for a, p, _ in cases], n, 6, 4, [f for _, _, f in cases])
            bad = []
            for i, ((a, p, fl), g) in enumerate(zip(cases, got)):
                g = [g[k * w:(k + 1) * w] for k in range(4)]
                want = ref_madd(field, a, p, fl)
                why = want_point(field, g, want)
                if not why and not (fl & ACC_AFFINE) and is_inf(a) and (g[2] != one_elem(field) or g[3] != one_elem(field)):
                    why = "xyzz_from_aff: zzz, zz not the stored one"
                if why:
                    bad.append((i, why, fl, g))
            fail_slots(f"xyzz_madd {FIELD_NAME[field]} form {form} variant {variant}", bad, n)
            if form == CHAIN:
                split = call(L, field, SPLIT, XYZZ_MADD, [a + p for a, p, _ in cases], n, 6, 4, [f for _, _, f in cases])
                assert split == got, f"xyzz_madd Fp n {n} variant {variant}: MulChain differs from MulSplit"


@pytest.mark.parametrize("field,form", KINDS, ids=KIND_ID)
def test_xyzz_dbl(L, field, form):
    F = algebra(field)
    w = NL * ncomp(field)
    for n in counts(field):
        pts = [xyzz(field, i, "dbl") for i in range(n)]
        for s in special_slots(n, 32 if field == FP2L else 64, 0, ["acc_inf"] * 3):
            pts[s] = inf_point(field)
        got = call(L, field, form, XYZZ_DBL, pts, n, 4, 4)
        bad = []
        for i, (p, g) in enumerate(zip(pts, got)):
            g = [g[k * w:(k + 1) * w] for k in range(4)]
            why = want_point(field, g, ("words", p) if is_inf(p) else ("val", _ref_dbl(F, pt_dec(field, p))))
            if why:
                bad.append((i, why, g))
        fail_slots(f"xyzz_dbl {FIELD_NAME[field]} form {form}", bad, n)
        if form == CHAIN:
            assert call(L, field, SPLIT, XYZZ_DBL, pts, n, 4, 4) == got, \
                f"xyzz_dbl Fp n {n}: MulChain differs from MulSplit"
