"""Range invariants of the lazily reduced Fr arithmetic (fr.hpp; DESIGN.md section
27), argued and then exercised at their bounds on the CPU (no GPU needed), in the
manner of test_fp_bounds.py.

1. The column bound of fr_mul and the bound of fr_red are computed exactly here:
   no 64-bit column wraps for the operand classes the kernels multiply, and fr_red
   (bounded exactly over its top limb, and run at both ends of it) leaves a value
   below 1.001 r.
2. The SAME header text is compiled for the host with every range check enabled
   (tests/host/fr_host_shim.cpp, MSM_FP_HOST_TEST) and run on max-limb operands of
   every class, on the butterfly of the transform kernels and on msm_fr_op's
   element formulas, against Python integers; the plain host twin (host_fr.hpp)
   runs beside it.
"""
import ctypes
import os
import random
import subprocess

import pytest

import fr_inputs as fi

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM_SRC = os.path.join(HERE, "host", "fr_host_shim.cpp")
SHIM_SO = os.path.join(HERE, "host", "_build", "fr_host_shim.so")
R = fi.R
NL, B = 9, 29
M29 = (1 << B) - 1
RP = 1 << 261  # the internal Montgomery radix
RPINV = pow(RP, -1, R)
SUB4R = [0x20000004, 0x3fffffdf, 0x3e5bfefe, 0x2d2017fe, 0x360154ee, 0x30101342, 0x3483339c, 0x2994cebd, 0x1cfb69c]
MAG = 0x235509


def _limbs(v):
    return [(v >> (B * i)) & M29 for i in range(NL - 1)] + [v >> (B * (NL - 1))]


def _val(lim):
    return sum(int(x) << (B * i) for i, x in enumerate(lim))


@pytest.fixture(scope="module")
def shim():
    csrc = os.path.join(os.path.dirname(HERE), "msm_blst_amd", "csrc")
    deps = [SHIM_SRC] + [os.path.join(csrc, f) for f in ("fp.hpp", "fr.hpp", "host_fr.hpp")]
    if not os.path.exists(SHIM_SO) or any(os.path.getmtime(d) > os.path.getmtime(SHIM_SO) for d in deps):
        os.makedirs(os.path.dirname(SHIM_SO), exist_ok=True)
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", SHIM_SO,
                        SHIM_SRC], check=True)
    L = ctypes.CDLL(SHIM_SO)
    vp = ctypes.c_void_p
    L.h_fr_overflow.argtypes = [ctypes.c_int]
    L.h_fr_prim.argtypes = [ctypes.c_int, vp, vp, vp]
    L.h_fr_bfly.argtypes = [vp] * 5
    L.h_fr_unpack.argtypes = [vp, vp]
    L.h_fr_pack.argtypes = [vp, vp]
    L.h_fr_elem.argtypes = [ctypes.c_int, vp, vp, vp]
    L.h_fr_host.argtypes = [ctypes.c_int, vp, vp, vp]
    L.h_fr_host_pow.argtypes = [vp, vp, vp]
    return L


# ------------------------------------------------------------ the argument ----
def test_constants():
    assert _val(SUB4R) == 4 * R and all(x >= M29 for x in SUB4R[:NL - 1])
    assert (-pow(R, -1, 1 << B)) % (1 << B) == M29          # m = -acc mod 2^29
    assert MAG == (1 << 44) // ((R >> 232) + 1)
    # the top limb of a class S value stays below the adjusted top limb of 4r (fr_sub4, fr_neg4)
    assert (2 * R) >> 232 < SUB4R[NL - 1]


def test_no_column_wraps():
    """fr_mul: a column holds at most 9 a_i b_j, 9 m_i r_j and the carry of the column
    before it.  The widest operand pairs the kernels multiply: a difference a + 4r - b
    (limbs < 2^29 + SUB4R) by a normalized value, a class S value by a negated twiddle
    (limbs <= SUB4R), and a sum of two class S values by a normalized value."""
    rl = _limbs(R)
    mr = 9 * M29 * max(rl)
    for amax, bmax in ((M29 + max(SUB4R), M29), (M29, max(SUB4R)), (2 * M29, M29), (2 * M29, 2 * M29)):
        col = 9 * amax * bmax + mr
        carry = col >> B
        assert col + carry + M29 * rl[0] < 1 << 64, (amax, bmax)
    # the value bound: the widest product, 6r (a difference) by 4r (a negated twiddle),
    # is far below 2^261 r, so every product is below 2r
    assert 6 * R * 4 * R // RP + R < 2 * R


def test_fr_red_bound():
    """fr_red: q <= floor(v / r) and v - q r < 1.001 r for every normalized v < 16r"""
    r8, top = R >> 232, (16 * R >> 232) + 1
    assert r8 == 0x73eda7
    # exactly: q >= v8 MAG / 2^44 - 1, so v - q r < v8 (2^232 - MAG r / 2^44) + 2^232 + r
    slope = (1 << (232 + 44)) - MAG * R
    assert 0 < slope and (top * slope >> 44) + (1 << 232) + R < 1.001 * R
    # and run: the top limbs at both ends of the range and a stride through it
    worst = 0
    for v8 in list(range(0, top, 9973)) + list(range(4096)) + list(range(top - 4096, top + 1)):
        q = (v8 * MAG) >> 44
        lo, hi = v8 << 232, min(((v8 + 1) << 232) - 1, 16 * R)
        assert q * R <= lo
        worst = max(worst, hi - q * R)
    assert worst < 1.001 * R


# ----------------------------------------------------------- host runs ----
def _arr(words):
    return (ctypes.c_uint32 * len(words))(*words)


def _prim(shim, op, a, b=None):
    r = (ctypes.c_uint32 * NL)()
    shim.h_fr_prim(op, r, _arr(a), _arr(b) if b is not None else None)
    return list(r)


def _max_S(rnd=None):
    """class S: normalized limbs at their maximum (or random), the largest top limb below 2r"""
    low = [M29 if rnd is None else rnd.randrange(M29 // 2, M29 + 1) for _ in range(NL - 1)]
    top = (2 * R - 1 - _val(low + [0])) >> 232
    return low + [top]


def _max_C(rnd=None):
    low = [M29 if rnd is None else rnd.randrange(M29 + 1) for _ in range(NL - 1)]
    top = (R - 1 - _val(low + [0])) >> 232
    return low + [top]


def _is_S(lim):
    return all(x <= M29 for x in lim[:NL - 1]) and _val(lim) < 2 * R


@pytest.mark.parametrize("seed", [None, 1, 2, 3])
def test_primitives_at_class_bounds(shim, seed):
    rnd = random.Random(seed) if seed is not None else None
    S, S2, C = _max_S(rnd), _max_S(rnd), _max_C(rnd)
    shim.h_fr_overflow(1)
    add = _prim(shim, 1, S, S2)
    sub = _prim(shim, 2, S, S2)
    neg = _prim(shim, 5, S)
    assert _val(add) == _val(S) + _val(S2) and _val(sub) == _val(S) + 4 * R - _val(S2)
    assert _val(neg) == 4 * R - _val(S)
    for a, b in ((S, S2), (add, C), (sub, C), (sub, S), (S, neg), (add, add), (C, C)):
        r = _prim(shim, 0, a, b)
        assert shim.h_fr_overflow(1) == 0, (a, b)
        assert _is_S(r) and _val(r) % R == _val(a) * _val(b) * RPINV % R
    for v in (add, sub, neg, _limbs(16 * R - 1)):
        r = _prim(shim, 3, v)
        assert shim.h_fr_overflow(1) == 0
        assert _is_S(r) and _val(r) % R == _val(v) % R
        c = _prim(shim, 4, r)
        assert _val(c) == _val(v) % R
    # a butterfly of the transform kernels on class S inputs and a canonical twiddle
    ra, rb = (ctypes.c_uint32 * NL)(), (ctypes.c_uint32 * NL)()
    shim.h_fr_bfly(ra, rb, _arr(S), _arr(S2), _arr(C))
    assert shim.h_fr_overflow(1) == 0
    assert _is_S(list(ra)) and _is_S(list(rb))
    assert _val(list(ra)) % R == (_val(S) + _val(S2)) % R
    assert _val(list(rb)) % R == (_val(S) - _val(S2)) * _val(C) * RPINV % R


def test_pack_unpack(shim):
    rnd = random.Random(7)
    for v in [0, 1, R - 1, R, 2 * R - 1, (1 << 256) - 1] + [rnd.randrange(1 << 256) for _ in range(50)]:
        w = (ctypes.c_uint8 * 32).from_buffer_copy(v.to_bytes(32, "little"))
        lim = (ctypes.c_uint32 * NL)()
        shim.h_fr_unpack(lim, w)
        assert list(lim) == _limbs(v)
        back = (ctypes.c_uint8 * 32)()
        shim.h_fr_overflow(1)
        shim.h_fr_pack(back, lim)
        assert shim.h_fr_overflow(1) == 0 and bytes(back) == bytes(w)


def _call(fn, op, a, b=None):
    out = (ctypes.c_uint8 * 32)()
    fn(op, out, (ctypes.c_uint8 * 32).from_buffer_copy(a), (ctypes.c_uint8 * 32).from_buffer_copy(b) if b else None)
    return bytes(out)


def test_element_formulas_and_host_twin(shim):
    """msm_fr_op's formulas (device header, host build) and host_fr.hpp on all pairs of
    the special values, byte for byte against the oracle (which the golden pins)."""
    vals = fi.special_values()
    frs = [fi.fr_bytes(v) for v in vals]
    shim.h_fr_overflow(1)
    for code, op in enumerate(fi.OPS):
        if op in fi.BINARY:
            cases = [(a, b) for a in frs for b in frs]
        elif op == "from_scalar":
            cases = [(fi.scalar_bytes(v), None) for v in vals + [R, R + 1, (1 << 256) - 1]]
        else:
            cases = [(a, None) for a in frs]
        for a, b in cases:
            want = fi.op_bytes(op, a, b)
            if op != "inv":
                assert _call(shim.h_fr_elem, code, a, b) == want, (op, a.hex(), b and b.hex())
            assert _call(shim.h_fr_host, code, a, b) == want, (op, a.hex(), b and b.hex())
    assert shim.h_fr_overflow(1) == 0
    out = (ctypes.c_uint8 * 32)()
    e = 0x1234567890abcdef << 100 | 5
    shim.h_fr_host_pow(out, (ctypes.c_uint8 * 32).from_buffer_copy(fi.fr_bytes(7)),
                       (ctypes.c_uint8 * 32).from_buffer_copy(e.to_bytes(32, "little")))
    assert bytes(out) == fi.fr_bytes(pow(7, e, R))
