"""CPU side of the evaluation-form polynomial call and the KZG layer
(msm_fr_eval_quotient, msm_kzg_*).  No GPU needed.

1. The library exports the calls, the Python mirror names them, and every MSM_E_ARG
   that is decided before device work is returned without a device.
2. The Python oracle (tests/kzg_inputs.py) agrees with the golden written from the
   reference (tests/golden/kzg.json), and its eval_quot with Horner on the inverse NTT
   and with the NTT of the synthetic-division quotient.
3. The per-element header of the kernels (csrc/fr_quot.hpp) is compiled for the host
   with every range check armed (tests/host/fr_quot_shim.cpp, MSM_FP_HOST_TEST) and
   run over whole small polynomials with operands at the class bounds, against the
   oracle, with msm_fp_overflow left clear.
"""
import ctypes
import os
import subprocess

import pytest

import enc_inputs as ei
import fr_inputs as fi
import kzg_inputs as ki

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM_SRC = os.path.join(HERE, "host", "fr_quot_shim.cpp")
SHIM_SO = os.path.join(HERE, "host", "_build", "fr_quot_shim.so")
R = fi.R
E_ARG, E_NODEV = -1, -3


@pytest.fixture(scope="module")
def L():
    import msm_blst_amd as m
    return m.lib()


def _err(L):
    return L.msm_last_error().decode()


# ------------------------------------------------------- exports and arguments ----
def test_exports_and_python_names(L):
    import msm_blst_amd as m
    for name in ("msm_fr_eval_quotient", "msm_kzg_ctx_create", "msm_kzg_ctx_destroy", "msm_kzg_commit",
                 "msm_kzg_open", "msm_kzg_verify"):
        assert hasattr(L, name), name
    for name in ("fr_eval_quotient", "KZGContext", "POLY_BITREV"):
        assert name in m.__all__ and hasattr(m, name), name
    assert m.POLY_BITREV == 8 and m.FR_DST_SCALAR == 4
    for meth in ("commit", "open", "verify", "close"):
        assert callable(getattr(m.KZGContext, meth))
    assert "fr_eval_quotient" in m.__doc__ and "KZGContext" in m.__doc__


def test_eval_quotient_arguments(L):
    buf = (ctypes.c_uint8 * (32 * 8))()
    y = (ctypes.c_uint8 * 64)()
    z = (ctypes.c_uint8 * 64)()
    q = (ctypes.c_uint8 * (32 * 8))()
    a = ctypes.addressof
    f = L.msm_fr_eval_quotient
    assert f(0, None, None, None, None, 2, 0, 0, 0, 0, None) == 0           # count == 0: nothing touched
    assert f(0, None, None, None, None, 2, 0, 0, 1, 1, None) == 0
    assert f(0, None, q, buf, z, 2, 2, 0, 0, 0, None) == E_ARG and "null" in _err(L)
    assert f(0, y, q, None, z, 2, 2, 0, 0, 0, None) == E_ARG
    assert f(0, y, q, buf, None, 2, 2, 0, 0, 0, None) == E_ARG
    assert f(0, y, None, buf, z, 27, 1, 0, 0, 0, None) == E_ARG and "log_n" in _err(L)
    assert f(0, y, None, buf, z, 20, (1 << 20) + 1, 0, 0, 0, None) == E_ARG and "count" in _err(L)
    for bad in (1, 2, 16, 4 | 32):
        assert f(0, y, None, buf, z, 2, 2, bad, 0, 0, None) == E_ARG and "flag" in _err(L)
    # q overlapping polys without being equal to it; equal is in place (then: no such device)
    assert f(0, y, a(buf) + 32, buf, z, 2, 1, 0, 0, 0, None) == E_ARG and "overlap" in _err(L)
    assert f(0, a(buf), None, buf, z, 2, 1, 0, 0, 0, None) == E_ARG and "overlap" in _err(L)
    assert f(1 << 20, y, buf, buf, z, 2, 2, 0, 0, 0, None) == E_NODEV
    # misaligned device pointers
    assert f(0, y, None, a(buf) + 4, z, 2, 1, 0, 1, 0, None) == E_ARG and "aligned" in _err(L)
    assert f(0, y, None, buf, a(z) + 4, 2, 1, 0, 1, 0, None) == E_ARG
    assert f(0, a(y) + 4, None, buf, z, 2, 1, 0, 0, 1, None) == E_ARG and "aligned" in _err(L)
    assert f(0, y, a(q) + 2, buf, z, 2, 1, 0, 0, 1, None) == E_ARG
    assert f(1 << 20, y, q, buf, z, 2, 2, 4 | 8, 0, 0, None) == E_NODEV     # every check passed


def test_kzg_arguments(L):
    srs = (ctypes.c_uint8 * (96 * 4))()
    tau = (ctypes.c_uint8 * 192)()
    h = ctypes.c_void_p()
    a = ctypes.addressof
    mk = L.msm_kzg_ctx_create
    assert mk(None, 0, 2, srs, 0, tau, 0, None) == E_ARG
    assert mk(ctypes.byref(h), 0, 2, None, 0, tau, 0, None) == E_ARG
    assert mk(ctypes.byref(h), 0, 2, srs, 0, None, 0, None) == E_ARG
    assert mk(ctypes.byref(h), 0, 21, srs, 0, tau, 0, None) == E_ARG and "log_n" in _err(L)
    assert mk(ctypes.byref(h), 0, 2, srs, 0, tau, 4, None) == E_ARG and "flag" in _err(L)
    assert mk(ctypes.byref(h), 0, 2, a(srs) + 4, 1, tau, 8, None) == E_ARG and "aligned" in _err(L)
    assert mk(ctypes.byref(h), 1 << 20, 2, srs, 0, tau, 8, None) == E_NODEV
    assert not h.value
    L.msm_kzg_ctx_destroy(None)
    out = (ctypes.c_uint8 * 96)()
    assert L.msm_kzg_commit(None, out, srs, 1, 0, 0, None) == E_ARG and "ctx" in _err(L)
    assert L.msm_kzg_open(None, out, out, srs, srs, 1, 0, 0, None) == E_ARG and "ctx" in _err(L)
    ok = (ctypes.c_uint8 * 4)()
    w = (ctypes.c_uint8 * 64)()
    v = L.msm_kzg_verify
    assert v(None, ok, None, srs, srs, srs, srs, 2, None, 0, 0, None, 0, 0, None) == E_ARG and "ctx" in _err(L)
    assert v(None, ok, None, srs, srs, srs, srs, 2, w, 257, 40, None, 0, 0, None) == E_ARG and "nbits" in _err(L)
    assert v(None, ok, None, srs, srs, srs, srs, 2, w, 64, 7, None, 0, 0, None) == E_ARG and "stride" in _err(L)
    dec = (ctypes.c_size_t * 3)(0, 2, 1)
    assert v(None, ok, None, srs, srs, srs, srs, 2, w, 64, 8, dec, 2, 0, None) == E_ARG and "decrease" in _err(L)
    past = (ctypes.c_size_t * 3)(0, 1, 3)
    assert v(None, ok, None, srs, srs, srs, srs, 2, w, 64, 8, past, 2, 0, None) == E_ARG and "past" in _err(L)


# ------------------------------------------------------------ the oracle ----
def test_oracle_against_the_golden(golden):
    g = golden("kzg.json")
    log_n, tau = g["log_n"], int(g["tau"], 16)
    assert (log_n, tau) == (ki.GOLDEN_LOG_N, ki.TAU)
    lag = ki.lagrange_at(tau, log_n)
    assert sum(lag) % R == 1                                   # the basis sums to one
    assert [ki.compressed(1, ki.g1(l)).hex() for l in lag] == g["srs"]
    assert ki.compressed(2, ki.g2(tau)).hex() == g["tau_g2"]
    polys, points = ki.golden_polys(), ki.golden_points()
    assert [ki.compressed(1, ki.g1(ki.commit_scalar(f, lag))).hex() for f in polys] == g["commitments"]
    for f, zs, row in zip(polys, points, g["openings"]):
        assert [int(o["z"], 16) for o in row] == zs
        for z, o in zip(zs, row):
            y, k = ki.proof_scalar(f, z, lag, tau, log_n)
            assert y == int(o["y"], 16)
            assert ki.compressed(1, ki.g1(k)).hex() == o["proof"]
            # and the evaluation-form quotient commits to the same point
            _, q = ki.eval_quot(f, z, log_n)
            assert ki.eval_at(q, lag) == k


def _points_for(log_n, seed):
    n, w = 1 << log_n, fi.root(log_n)
    zs = fi.rand_values(2, seed) + [0, 1]
    return zs + [pow(w, i, R) for i in sorted({0, 1 % n, n // 2, n - 1})]


@pytest.mark.parametrize("log_n", [0, 1, 2, 5])
def test_eval_quot_against_horner_and_synthetic_division(log_n):
    n = 1 << log_n
    f = fi.rand_values(n, 100 + log_n)
    coeffs = fi.ntt(f, inverse=True)
    fb = [f[ki.brev(i, log_n)] for i in range(n)]
    for z in _points_for(log_n, 200 + log_n):
        y, q = ki.eval_quot(f, z, log_n)
        assert y == ki.horner(coeffs, z), (log_n, z)
        qc, rem = ki.synthetic_quotient(coeffs, z, y)
        assert rem == 0 and fi.ntt(qc) == q, (log_n, z)
        yb, qb = ki.eval_quot(fb, z, log_n, bitrev=True)
        assert yb == y and qb == [q[ki.brev(i, log_n)] for i in range(n)], (log_n, z)


# ------------------------------------------------ the per-element header ----
@pytest.fixture(scope="module")
def shim():
    csrc = os.path.join(os.path.dirname(HERE), "msm_blst_amd", "csrc")
    deps = [SHIM_SRC] + [os.path.join(csrc, f) for f in ("fp.hpp", "fr.hpp", "fr_quot.hpp", "host_fr.hpp")]
    if not os.path.exists(SHIM_SO) or any(os.path.getmtime(d) > os.path.getmtime(SHIM_SO) for d in deps):
        os.makedirs(os.path.dirname(SHIM_SO), exist_ok=True)
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", SHIM_SO,
                        SHIM_SRC], check=True)
    S = ctypes.CDLL(SHIM_SO)
    vp = ctypes.c_void_p
    S.h_fq_overflow.argtypes = [ctypes.c_int]
    S.h_fq_poly.argtypes = [vp, vp, vp, vp, vp, vp, ctypes.c_size_t, ctypes.c_int, ctypes.c_int]
    return S


def _host_poly(S, f, z, log_n, bitrev, scalar):
    n = 1 << log_n
    y = (ctypes.c_uint8 * 32)()
    q = (ctypes.c_uint8 * (32 * n))()
    S.h_fq_poly(y, q, fi.pack(f), fi.pack(ki.domain(log_n, bitrev)), fi.fr_bytes(z), fi.fr_bytes(pow(n, -1, R)), n,
                log_n, int(scalar))
    return bytes(y), bytes(q)


@pytest.mark.parametrize("bitrev", [False, True])
@pytest.mark.parametrize("log_n", [0, 1, 2, 4])
def test_header_over_whole_polynomials_at_the_class_bounds(shim, log_n, bitrev):
    """values 0, 1, r - 1 and the special values of fr_inputs as coefficients AND as points,
    with every domain point among the points: byte for byte the oracle, no range check hit"""
    n = 1 << log_n
    special = fi.special_values()
    polys = [[special[(i + s) % len(special)] for i in range(n)] for s in (0, 3, 7)]
    polys += [[0] * n, [R - 1] * n, [1] * n, [R - 1 if i & 1 else 0 for i in range(n)]]
    zs = special + ki.domain(log_n, bitrev)
    shim.h_fq_overflow(1)
    for f in polys:
        for z in zs:
            want_y, want_q = ki.eval_quot(f, z, log_n, bitrev)
            for scalar in (False, True):
                y, q = _host_poly(shim, f, z, log_n, bitrev, scalar)
                assert shim.h_fq_overflow(1) == 0, (f, z, scalar)
                assert y == fi.fr_bytes(want_y), (f, z, scalar)
                assert q == fi.pack(want_q, scalar=scalar), (f, z, scalar)
