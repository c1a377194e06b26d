"""What the context entry points of the C ABI (csrc/abi.cpp: msm_ctx_*,
msm_ches_ctx_*, msm_bgmw_ctx_*, msm_wbits_ctx_*) return on a live context that
is used wrongly: the code and the exact msm_last_error() bytes, the state of
the context afterwards, and the out-pointer.  Every error here is found on the
host before any device work (an argument or state check of abi.cpp, or a
range / parameter check at the head of the engine's function).  The messages
are literals copied from the source, so a reworded message fails here.  The
NULL-context and no-device cases are in test_abi_ctx_host.py."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

MSM_OK, MSM_E_ARG, MSM_E_HIP, MSM_E_NODEV, MSM_E_STATE = 0, -1, -2, -3, -4
vp = ctypes.c_void_p
SENTINEL = 0x5A5A5A5A5A5A
JAC = {1: 144, 2: 288}
AFF = {1: 96, 2: 192}

NO_TABLE = b"no table: build_table, set_table or load_table first"
STRIDE32 = b"bad args (stride must be >= 32)"
OUT_OF_BOUNDS = b"table range out of bounds"
N = 300  # points of the CHES (n_exp = 10) and BGMW95 (q_exp = 16, h = 16) contexts
NW = 4   # points of the wbits (wbits = 4) contexts
PHASES = ("digits", "sort", "accumulate", "reduce", "finalize", "total")


@pytest.fixture(scope="module")
def m():
    import msm_blst_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible")
    return m


def _fails(L, rc, code, msg):
    assert rc == code
    assert L.msm_last_error() == msg


def _create(L, name, group, *args):
    ctx = vp()
    assert getattr(L, f"msm_{name}_create")(ctypes.byref(ctx), group, 0, *args) == MSM_OK, L.msm_last_error()
    return ctx


@pytest.fixture
def ctxs(m):
    """_create with the contexts destroyed after the test."""
    L = m.lib()
    made = []

    def make(name, group, *args):
        made.append((name, _create(L, name, group, *args)))
        return made[-1][1]

    yield make
    for name, ctx in made:
        getattr(L, f"msm_{name}_destroy")(ctx)


def _mult(m, group, call):
    """compressed result of call(ret) == MSM_OK"""
    ret = (ctypes.c_uint8 * JAC[group])()
    assert call(ret) == MSM_OK, m.lib().msm_last_error()
    return m.compress(group, bytes(ret))


def _ref(m, group, pts, sc, n):
    """the same MSM (255-bit scalars, stride 32) through the blst-named Pippenger, compressed"""
    return m.compress(group, (m.p1s_mult_pippenger, m.p2s_mult_pippenger)[group - 1](pts, sc, n))


@pytest.mark.parametrize("group", [1, 2])
def test_mult_before_any_table(m, ctxs, group):
    L = m.lib()
    sc = m.gen_scalars(N, 3)
    ret = (ctypes.c_uint8 * (2 * JAC[group]))(*([0xAB] * (2 * JAC[group])))
    ms = ctypes.c_float(-1.0)
    ches = ctxs("ches_ctx", group, 10, 0)
    _fails(L, L.msm_ches_ctx_mult(ches, ret, sc, 32, 0, None), MSM_E_STATE, NO_TABLE)
    _fails(L, L.msm_ches_ctx_mult_batch(ches, ret, sc, 32, 32 * N, 2, 0, None), MSM_E_STATE, NO_TABLE)
    _fails(L, L.msm_ches_ctx_time_accumulation(ches, sc, 32 * N, 1, 1, ctypes.byref(ms)), MSM_E_STATE, b"no table")
    bgmw = ctxs("bgmw_ctx", group, 16, 16)
    _fails(L, L.msm_bgmw_ctx_mult(bgmw, ret, sc, 32, 0, None), MSM_E_STATE, NO_TABLE)
    wb = ctxs("wbits_ctx", group, 4)
    _fails(L, L.msm_wbits_ctx_mult(wb, ret, sc, 32, 255, 0, None), MSM_E_STATE,
           b"no table: precompute or set_table first")
    # the argument checks come before the state check
    _fails(L, L.msm_ches_ctx_mult(ches, ret, sc, 31, 0, None), MSM_E_ARG, STRIDE32)
    _fails(L, L.msm_ches_ctx_mult_batch(ches, ret, sc, 31, 32 * N, 2, 0, None), MSM_E_ARG, STRIDE32)
    _fails(L, L.msm_bgmw_ctx_mult(bgmw, ret, sc, 31, 0, None), MSM_E_ARG, STRIDE32)
    _fails(L, L.msm_wbits_ctx_mult(wb, ret, sc, 0, 255, 0, None), MSM_E_ARG, b"bad args (stride < nbits/8)")
    assert bytes(ret) == bytes([0xAB] * len(ret)) and ms.value == -1.0


@pytest.mark.parametrize("group", [1, 2])
def test_ches_errors_leave_the_context_usable(m, ctxs, group):
    L = m.lib()
    pts, sc = m.fixed_points(group, N), m.gen_scalars(N, 5)
    ctx = ctxs("ches_ctx", group, 10, 0)
    assert L.msm_ches_ctx_build_table(ctx, pts, N, 0, None) == MSM_OK, L.msm_last_error()
    rows = 3 * 20 * N  # 3 h rows per point, h = 20 in the n_exp = 10 configuration
    before = _mult(m, group, lambda ret: L.msm_ches_ctx_mult(ctx, ret, sc, 32, 0, None))
    ret = (ctypes.c_uint8 * JAC[group])()
    for stride in (0, 31):
        _fails(L, L.msm_ches_ctx_mult(ctx, ret, sc, stride, 0, None), MSM_E_ARG, STRIDE32)
        _fails(L, L.msm_ches_ctx_mult_batch(ctx, ret, sc, stride, 32 * N, 1, 0, None), MSM_E_ARG, STRIDE32)
    _fails(L, L.msm_ches_ctx_mult(ctx, None, sc, 32, 0, None), MSM_E_ARG, STRIDE32)
    out = (ctypes.c_uint8 * (2 * AFF[group]))()
    _fails(L, L.msm_ches_ctx_get_table(ctx, out, rows - 1, 2), MSM_E_HIP, OUT_OF_BOUNDS)
    _fails(L, L.msm_ches_ctx_get_table(ctx, out, rows + 1, 0), MSM_E_HIP, OUT_OF_BOUNDS)
    _fails(L, L.msm_ches_ctx_get_table(ctx, None, 0, 1), MSM_E_ARG, b"bad args")
    assert bytes(out) == bytes(len(out))
    assert L.msm_ches_ctx_get_table(ctx, out, rows - 2, 2) == MSM_OK  # the last two rows
    assert L.msm_ches_ctx_get_table(ctx, None, rows, 0) == MSM_OK  # the empty range at the end
    assert _mult(m, group, lambda ret: L.msm_ches_ctx_mult(ctx, ret, sc, 32, 0, None)) == before
    assert before == _ref(m, group, pts, sc, N)


@pytest.mark.parametrize("group", [1, 2])
def test_bgmw_errors_leave_the_context_usable(m, ctxs, group):
    L = m.lib()
    pts, sc = m.fixed_points(group, N), m.gen_scalars(N, 6)
    ctx = ctxs("bgmw_ctx", group, 16, 16)
    assert L.msm_bgmw_ctx_build_table(ctx, pts, N, 0, None) == MSM_OK, L.msm_last_error()
    rows = 16 * N  # h rows per point
    before = _mult(m, group, lambda ret: L.msm_bgmw_ctx_mult(ctx, ret, sc, 32, 0, None))
    ret = (ctypes.c_uint8 * JAC[group])()
    for stride in (0, 31):
        _fails(L, L.msm_bgmw_ctx_mult(ctx, ret, sc, stride, 0, None), MSM_E_ARG, STRIDE32)
    _fails(L, L.msm_bgmw_ctx_mult(ctx, None, sc, 32, 0, None), MSM_E_ARG, STRIDE32)
    out = (ctypes.c_uint8 * (2 * AFF[group]))()
    _fails(L, L.msm_bgmw_ctx_get_table(ctx, out, rows - 1, 2), MSM_E_HIP, OUT_OF_BOUNDS)
    _fails(L, L.msm_bgmw_ctx_get_table(ctx, out, rows + 1, 0), MSM_E_HIP, OUT_OF_BOUNDS)
    _fails(L, L.msm_bgmw_ctx_get_table(ctx, None, 0, 1), MSM_E_ARG, b"bad args")
    assert bytes(out) == bytes(len(out))
    assert L.msm_bgmw_ctx_get_table(ctx, out, rows - 2, 2) == MSM_OK
    assert _mult(m, group, lambda ret: L.msm_bgmw_ctx_mult(ctx, ret, sc, 32, 0, None)) == before
    assert before == _ref(m, group, pts, sc, N)


@pytest.mark.parametrize("group", [1, 2])
def test_wbits_errors_leave_the_context_usable(m, ctxs, group):
    L = m.lib()
    pts, sc = m.fixed_points(group, NW), m.gen_scalars(NW, 7)
    ctx = ctxs("wbits_ctx", group, 4)
    assert L.msm_wbits_ctx_precompute(ctx, pts, NW, 0, None) == MSM_OK, L.msm_last_error()
    rows = NW << 3  # npoints << (wbits - 1)
    assert L.msm_wbits_ctx_table_rows(ctx) == rows
    before = _mult(m, group, lambda ret: L.msm_wbits_ctx_mult(ctx, ret, sc, 32, 255, 0, None))
    ret = (ctypes.c_uint8 * JAC[group])()
    msg = b"bad args (stride < nbits/8)"
    _fails(L, L.msm_wbits_ctx_mult(ctx, ret, sc, 0, 0, 0, None), MSM_E_ARG, msg)  # stride == 0
    _fails(L, L.msm_wbits_ctx_mult(ctx, ret, sc, 31, 255, 0, None), MSM_E_ARG, msg)  # 32 bytes of scalar
    _fails(L, L.msm_wbits_ctx_mult(ctx, ret, sc, 32, 257, 0, None), MSM_E_ARG, msg)  # 33 bytes of scalar
    _fails(L, L.msm_wbits_ctx_mult(ctx, None, sc, 32, 255, 0, None), MSM_E_ARG, msg)
    out = (ctypes.c_uint8 * (2 * AFF[group]))()
    _fails(L, L.msm_wbits_ctx_get_table(ctx, out, rows - 1, 2), MSM_E_ARG, OUT_OF_BOUNDS)
    _fails(L, L.msm_wbits_ctx_get_table(ctx, out, rows + 1, 0), MSM_E_ARG, OUT_OF_BOUNDS)
    _fails(L, L.msm_wbits_ctx_get_table(ctx, None, 0, 1), MSM_E_ARG, b"bad args")
    assert bytes(out) == bytes(len(out))
    assert L.msm_wbits_ctx_get_table(ctx, out, rows - 2, 2) == MSM_OK
    assert _mult(m, group, lambda ret: L.msm_wbits_ctx_mult(ctx, ret, sc, 32, 255, 0, None)) == before
    assert before == _ref(m, group, pts, sc, NW)


@pytest.mark.parametrize("group", [1, 2])
def test_constructor_rejections_keep_their_codes(m, group):
    """A constructor that throws on its parameters: MSM_E_ARG on these two families
    (MSM_E_HIP on msm_ctx and CHES contexts), its message, *ctx untouched."""
    L = m.lib()
    out = vp(SENTINEL)
    _fails(L, L.msm_wbits_ctx_create(ctypes.byref(out), group, 0, 1), MSM_E_ARG,
           b"wbits must be in [2, 14] (ref multi_scalar.c:67)")
    _fails(L, L.msm_bgmw_ctx_create(ctypes.byref(out), group, 0, 1, 1), MSM_E_ARG,
           b"bad BGMW95 parameters (need q_exp in [2,24], q_exp h >= 255)")
    assert out.value == SENTINEL


@pytest.mark.parametrize("group", [1, 2])
def test_msm_ctx_mult_arguments(m, ctxs, group):
    L = m.lib()
    pts, sc = m.fixed_points(group, N), m.gen_scalars(N, 8)
    ctx = ctxs("ctx", group, 0)
    assert L.msm_ctx_set_points(ctx, pts, N, 0, None) == MSM_OK, L.msm_last_error()
    ret = (ctypes.c_uint8 * JAC[group])(*([0xAB] * JAC[group]))
    for stride, nbits in ((32, 0), (33, 257), (32, 1 << 20), (31, 255), (0, 1)):
        _fails(L, L.msm_ctx_mult(ctx, ret, sc, stride, nbits, 0, None), MSM_E_ARG, b"bad args")
        _fails(L, L.msm_ctx_mult_batch(ctx, ret, sc, stride, 32 * N, nbits, 1, 0, None), MSM_E_ARG, b"bad args")
    _fails(L, L.msm_ctx_mult(ctx, None, sc, 32, 255, 0, None), MSM_E_ARG, b"bad args")
    _fails(L, L.msm_ctx_mult_batch(ctx, None, sc, 32, 32 * N, 255, 1, 0, None), MSM_E_ARG, b"bad args")
    _fails(L, L.msm_ctx_set_points(ctx, None, 1, 0, None), MSM_E_ARG, b"bad args")
    assert bytes(ret) == bytes([0xAB] * len(ret))
    got = _mult(m, group, lambda ret: L.msm_ctx_mult(ctx, ret, sc, 32, 255, 0, None))
    assert got == _ref(m, group, pts, sc, N)


@pytest.mark.parametrize("group", [1, 2])
def test_set_points_encoded_rejection_keeps_the_points(m, ctxs, group):
    L = m.lib()
    n, bad_at = 37, 29
    pts, sc = m.fixed_points(group, n), m.gen_scalars(n, 9)
    other = bytearray(m.ps_encode(group, bytes(m.fixed_points(group, n, start=5)), n))  # compressed
    good = bytes(other)
    other[bad_at * 48 * group] &= 0x7F  # the compressed bit cleared: status 1 (bad encoding)
    ctx = ctxs("ctx", group, 0)
    assert L.msm_ctx_set_points(ctx, pts, n, 0, None) == MSM_OK, L.msm_last_error()
    before = _mult(m, group, lambda ret: L.msm_ctx_mult(ctx, ret, sc, 32, 255, 0, None))
    first_bad = ctypes.c_size_t(SENTINEL)
    src = (ctypes.c_uint8 * len(other)).from_buffer_copy(other)
    rc = L.msm_ctx_set_points_encoded(ctx, src, n, m.ENC_COMPRESSED, m.DECODE_CHECK_GROUP, 0, ctypes.byref(first_bad),
                                      None)
    _fails(L, rc, MSM_E_ARG, b"encoded point 29 rejected: status 1")
    assert first_bad.value == bad_at
    assert _mult(m, group, lambda ret: L.msm_ctx_mult(ctx, ret, sc, 32, 255, 0, None)) == before
    # the decode call's own argument errors come back unchanged
    _fails(L, L.msm_ctx_set_points_encoded(ctx, src, n, 7, 0, 0, None, None), MSM_E_ARG, b"unknown encoding")
    assert _mult(m, group, lambda ret: L.msm_ctx_mult(ctx, ret, sc, 32, 255, 0, None)) == before
    # the intact encoding is accepted, leaves first_bad alone and replaces the points
    first_bad.value = SENTINEL
    src = (ctypes.c_uint8 * len(good)).from_buffer_copy(good)
    assert L.msm_ctx_set_points_encoded(ctx, src, n, m.ENC_COMPRESSED, m.DECODE_CHECK_GROUP, 0,
                                        ctypes.byref(first_bad), None) == MSM_OK, L.msm_last_error()
    assert first_bad.value == SENTINEL
    after = _mult(m, group, lambda ret: L.msm_ctx_mult(ctx, ret, sc, 32, 255, 0, None))
    assert after != before
    assert after == _ref(m, group, m.fixed_points(group, n, start=5), sc, n)


@pytest.mark.parametrize("group", [1, 2])
def test_phase_times_after_a_profiled_mult(m, ctxs, group):
    L = m.lib()
    pts, sc = m.fixed_points(group, N), m.gen_scalars(N, 10)
    ret = (ctypes.c_uint8 * JAC[group])()
    plain = ctxs("ctx", group, 0)
    assert L.msm_ctx_set_points(plain, pts, N, 0, None) == MSM_OK
    ches = ctxs("ches_ctx", group, 10, 0)
    assert L.msm_ches_ctx_build_table(ches, pts, N, 0, None) == MSM_OK
    bgmw = ctxs("bgmw_ctx", group, 16, 16)
    assert L.msm_bgmw_ctx_build_table(bgmw, pts, N, 0, None) == MSM_OK
    for name, ctx, mult in (("ctx", plain, lambda c: L.msm_ctx_mult(c, ret, sc, 32, 255, 0, None)),
                            ("ches_ctx", ches, lambda c: L.msm_ches_ctx_mult(c, ret, sc, 32, 0, None)),
                            ("bgmw_ctx", bgmw, lambda c: L.msm_bgmw_ctx_mult(c, ret, sc, 32, 0, None))):
        assert getattr(L, f"msm_{name}_set_profiling")(ctx, 1) == MSM_OK
        assert mult(ctx) == MSM_OK, L.msm_last_error()
        t = (ctypes.c_float * 6)(*([-1.0] * 6))
        _fails(L, getattr(L, f"msm_{name}_phase_times")(ctx, None), MSM_E_ARG, b"null")
        assert getattr(L, f"msm_{name}_phase_times")(ctx, t) == MSM_OK
        times = dict(zip(PHASES, t))
        assert all(v >= 0.0 for v in times.values()), (name, times)
        assert times["total"] > 0.0 and all(times["total"] >= v for v in times.values()), (name, times)
        assert getattr(L, f"msm_{name}_set_profiling")(ctx, 0) == MSM_OK
