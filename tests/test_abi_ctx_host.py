"""CPU-side pins of the context entry points of the C ABI (include/msm_mi355x.h:
msm_ctx_*, msm_ches_ctx_*, msm_bgmw_ctx_*, msm_wbits_ctx_*, msm_ches_params /
_bucket_set / _digit_table): the return code and the exact msm_last_error()
bytes of every argument error that is returned before any device work, the
order of the checks where a call can be wrong twice, the out-pointer left as
the caller set it, and what a NULL context gives.  The messages are literals
copied from csrc/abi.cpp, so a reworded message fails here.  No GPU is used;
the errors that need a live context are in test_gpu_abi_ctx.py."""
import ctypes

import pytest

MSM_OK, MSM_E_ARG, MSM_E_HIP, MSM_E_NODEV, MSM_E_STATE = 0, -1, -2, -3, -4
vp = ctypes.c_void_p
SENTINEL = 0x5A5A5A5A5A5A

NODEV = b"no such HIP device"
NO_CONFIG = b"no CHES configuration for n_exp/beta"
STRIDE32 = b"bad args (stride must be >= 32)"


@pytest.fixture(scope="module")
def m():
    import msm_blst_amd as m
    m.lib()
    return m


def _fails(L, rc, code, msg):
    assert rc == code
    assert L.msm_last_error() == msg


# name -> (call(L, ctx_ptr, group, device), message of a NULL ctx / a bad group)
def _creators(L):
    v10 = (ctypes.c_int * 9)(10, 0, 13, 20, 231, 6, 1725, 12, 22)  # the n_exp = 10 configuration
    return {
        "msm_ctx_create": (lambda c, g, d: L.msm_ctx_create(c, g, d, 0), b"bad ctx/group"),
        "msm_ches_ctx_create": (lambda c, g, d: L.msm_ches_ctx_create(c, g, d, 10, 0), b"bad ctx/group/params"),
        "msm_ches_ctx_create_params": (lambda c, g, d: L.msm_ches_ctx_create_params(c, g, d, v10),
                                       b"bad ctx/group/params"),
        "msm_ches_ctx_create_multi": (lambda c, g, d: L.msm_ches_ctx_create_multi(c, g, (ctypes.c_int * 1)(d), 1, 10, 0),
                                      b"bad ctx/group/devices"),
        "msm_bgmw_ctx_create": (lambda c, g, d: L.msm_bgmw_ctx_create(c, g, d, 16, 16), b"bad ctx/group"),
        "msm_wbits_ctx_create": (lambda c, g, d: L.msm_wbits_ctx_create(c, g, d, 4), b"bad ctx/group"),
    }


CREATORS = ["msm_ctx_create", "msm_ches_ctx_create", "msm_ches_ctx_create_params", "msm_ches_ctx_create_multi",
            "msm_bgmw_ctx_create", "msm_wbits_ctx_create"]


@pytest.mark.parametrize("name", CREATORS)
def test_create_argument_errors(m, name):
    L = m.lib()
    call, msg = _creators(L)[name]
    _fails(L, call(None, 1, 0), MSM_E_ARG, msg)  # NULL ctx pointer
    out = vp(SENTINEL)
    for group in (0, 3):
        _fails(L, call(ctypes.byref(out), group, 0), MSM_E_ARG, msg)
    # a bad group is reported before a missing device
    _fails(L, call(ctypes.byref(out), 0, -1), MSM_E_ARG, msg)
    for group in (1, 2):
        for dev in (-1, m.device_count()):
            _fails(L, call(ctypes.byref(out), group, dev), MSM_E_NODEV, NODEV)
    assert out.value == SENTINEL


def test_create_null_parameter_arrays(m):
    L = m.lib()
    out = vp(SENTINEL)
    _fails(L, L.msm_ches_ctx_create_params(ctypes.byref(out), 1, 0, None), MSM_E_ARG, b"bad ctx/group/params")
    _fails(L, L.msm_ches_ctx_create_multi(ctypes.byref(out), 1, None, 1, 10, 0), MSM_E_ARG, b"bad ctx/group/devices")
    one = (ctypes.c_int * 1)(0)
    for ndev in (0, -1):
        _fails(L, L.msm_ches_ctx_create_multi(ctypes.byref(out), 1, one, ndev, 10, 0), MSM_E_ARG,
               b"bad ctx/group/devices")
    # every device of the list is checked
    two = (ctypes.c_int * 2)(0, m.device_count())
    _fails(L, L.msm_ches_ctx_create_multi(ctypes.byref(out), 2, two, 2, 10, 0), MSM_E_NODEV, NODEV)
    assert out.value == SENTINEL


def test_create_without_a_configuration(m):
    """The parameter lookup comes before the device check, and in
    msm_ches_ctx_create before the ctx / group check as well."""
    L = m.lib()
    out = vp(SENTINEL)
    nd = m.device_count()
    for n_exp, beta in ((7, 0), (10, 1), (22, 0)):
        _fails(L, L.msm_ches_ctx_create(ctypes.byref(out), 1, nd, n_exp, beta), MSM_E_ARG, NO_CONFIG)
        _fails(L, L.msm_ches_ctx_create(None, 0, -1, n_exp, beta), MSM_E_ARG, NO_CONFIG)
        devs = (ctypes.c_int * 1)(nd)
        _fails(L, L.msm_ches_ctx_create_multi(ctypes.byref(out), 2, devs, 1, n_exp, beta), MSM_E_ARG, NO_CONFIG)
        # ... but after the ctx / group / devices check of create_multi
        _fails(L, L.msm_ches_ctx_create_multi(None, 2, devs, 1, n_exp, beta), MSM_E_ARG, b"bad ctx/group/devices")
    assert out.value == SENTINEL


NULL_CTX_CALLS = [
    ("msm_ctx_set_points", lambda L, b, f: L.msm_ctx_set_points(None, b, 1, 0, None), b"bad args"),
    ("msm_ctx_set_points_encoded", lambda L, b, f: L.msm_ctx_set_points_encoded(None, b, 1, 0, 0, 0, None, None),
     b"bad args"),
    ("msm_ctx_mult", lambda L, b, f: L.msm_ctx_mult(None, b, b, 32, 255, 0, None), b"bad args"),
    ("msm_ctx_mult_batch", lambda L, b, f: L.msm_ctx_mult_batch(None, b, b, 32, 32, 255, 1, 0, None), b"bad args"),
    ("msm_ctx_set_profiling", lambda L, b, f: L.msm_ctx_set_profiling(None, 1), b"null ctx"),
    ("msm_ctx_phase_times", lambda L, b, f: L.msm_ctx_phase_times(None, f), b"null"),
    ("msm_ches_ctx_build_table", lambda L, b, f: L.msm_ches_ctx_build_table(None, b, 1, 0, None), b"bad args"),
    ("msm_ches_ctx_set_table", lambda L, b, f: L.msm_ches_ctx_set_table(None, b, 1, 0, None), b"bad args"),
    ("msm_ches_ctx_get_table", lambda L, b, f: L.msm_ches_ctx_get_table(None, b, 0, 1), b"bad args"),
    ("msm_ches_ctx_mult", lambda L, b, f: L.msm_ches_ctx_mult(None, b, b, 32, 0, None), STRIDE32),
    ("msm_ches_ctx_mult_batch", lambda L, b, f: L.msm_ches_ctx_mult_batch(None, b, b, 32, 32, 1, 0, None), STRIDE32),
    ("msm_ches_ctx_save_table", lambda L, b, f: L.msm_ches_ctx_save_table(None, b"/nonexistent/t"), b"bad args"),
    ("msm_ches_ctx_load_table", lambda L, b, f: L.msm_ches_ctx_load_table(None, b"/nonexistent/t"), b"bad args"),
    ("msm_ches_ctx_set_profiling", lambda L, b, f: L.msm_ches_ctx_set_profiling(None, 1), b"null ctx"),
    ("msm_ches_ctx_phase_times", lambda L, b, f: L.msm_ches_ctx_phase_times(None, f), b"null"),
    ("msm_ches_ctx_time_accumulation",
     lambda L, b, f: L.msm_ches_ctx_time_accumulation(None, b, 32, 1, 1, f), b"bad args"),
    ("msm_bgmw_ctx_build_table", lambda L, b, f: L.msm_bgmw_ctx_build_table(None, b, 1, 0, None), b"bad args"),
    ("msm_bgmw_ctx_set_table", lambda L, b, f: L.msm_bgmw_ctx_set_table(None, b, 1, 0, None), b"bad args"),
    ("msm_bgmw_ctx_get_table", lambda L, b, f: L.msm_bgmw_ctx_get_table(None, b, 0, 1), b"bad args"),
    ("msm_bgmw_ctx_mult", lambda L, b, f: L.msm_bgmw_ctx_mult(None, b, b, 32, 0, None), STRIDE32),
    ("msm_bgmw_ctx_save_table", lambda L, b, f: L.msm_bgmw_ctx_save_table(None, b"/nonexistent/t"), b"bad args"),
    ("msm_bgmw_ctx_load_table", lambda L, b, f: L.msm_bgmw_ctx_load_table(None, b"/nonexistent/t"), b"bad args"),
    ("msm_bgmw_ctx_set_profiling", lambda L, b, f: L.msm_bgmw_ctx_set_profiling(None, 1), b"null ctx"),
    ("msm_bgmw_ctx_phase_times", lambda L, b, f: L.msm_bgmw_ctx_phase_times(None, f), b"null"),
    ("msm_wbits_ctx_precompute", lambda L, b, f: L.msm_wbits_ctx_precompute(None, b, 1, 0, None), b"bad args"),
    ("msm_wbits_ctx_set_table", lambda L, b, f: L.msm_wbits_ctx_set_table(None, b, 1, 0, None), b"bad args"),
    ("msm_wbits_ctx_get_table", lambda L, b, f: L.msm_wbits_ctx_get_table(None, b, 0, 1), b"bad args"),
    ("msm_wbits_ctx_mult", lambda L, b, f: L.msm_wbits_ctx_mult(None, b, b, 32, 255, 0, None),
     b"bad args (stride < nbits/8)"),
]


@pytest.mark.parametrize("name,call,msg", NULL_CTX_CALLS, ids=[c[0] for c in NULL_CTX_CALLS])
def test_null_context_message(m, name, call, msg):
    L = m.lib()
    assert hasattr(L, name)
    buf = (ctypes.c_uint8 * 512)()
    f6 = (ctypes.c_float * 6)()
    L.msm_ches_params(0, 0, None)  # leaves another message behind
    assert L.msm_last_error() == NO_CONFIG
    _fails(L, call(L, buf, f6), MSM_E_ARG, msg)
    assert msg  # a non-empty message
    assert bytes(buf) == bytes(512) and list(f6) == [0.0] * 6


def test_null_context_getters_and_destroy(m):
    L = m.lib()
    assert L.msm_ches_ctx_shards(None) == 0
    assert L.msm_ches_ctx_rccl_exchange(None) == 0
    assert L.msm_ches_ctx_bucket_count(None) == 0
    assert L.msm_ches_ctx_batch_lanes(None) == 0
    assert L.msm_bgmw_ctx_bucket_count(None) == 0
    assert L.msm_wbits_ctx_table_rows(None) == 0
    assert L.msm_ctx_destroy(None) is None
    assert L.msm_ches_ctx_destroy(None) is None
    assert L.msm_bgmw_ctx_destroy(None) is None
    assert L.msm_wbits_ctx_destroy(None) is None


def test_ches_params(m):
    L = m.lib()
    out = (ctypes.c_int * 9)(*([-7] * 9))
    _fails(L, L.msm_ches_params(10, 0, None), MSM_E_ARG, NO_CONFIG)  # NULL out
    for n_exp, beta in ((7, 0), (22, 0), (10, 1), (10, -1), (0, 0)):
        _fails(L, L.msm_ches_params(n_exp, beta, out), MSM_E_ARG, NO_CONFIG)
    assert list(out) == [-7] * 9
    assert L.msm_ches_params(10, 0, out) == MSM_OK
    assert list(out) == [10, 0, 13, 20, 231, 6, 1725, 12, 22]
    assert L.msm_ches_params(16, 1, out) == MSM_OK
    assert list(out) == [16, 1, 18, 15, 7, 6, 54618, 17, 15]


def test_ches_bucket_set(m):
    L = m.lib()
    out = (ctypes.c_int * 8)(*([-7] * 8))
    for q, a_h in ((3, 0), (0, 7), (-4, 7), (4096, -1)):
        assert L.msm_ches_bucket_set(q, a_h, out, 8) == 0
    assert list(out) == [-7] * 8
    assert L.msm_ches_bucket_set(4096, 7, None, 0) == 857  # b_size of the n_exp = 8 configuration
    assert L.msm_ches_bucket_set(4096, 7, out, 4) == 857  # the whole size; `cap` entries written
    assert list(out)[:4] == [0, 1, 4, 5] and list(out)[4:] == [-7] * 4  # 2 and 3 have an odd 2-3 exponent
    assert L.msm_ches_bucket_set(8192, 231, None, 0) == 1725


def test_ches_digit_table(m):
    from msm_blst_amd.ches import Digit
    L = m.lib()
    q, a_h = 4096, 7
    out = (Digit * (q + 1))()
    for bad in ((3, a_h, out), (0, a_h, out), (q, -1, out), (q, a_h, None)):
        _fails(L, L.msm_ches_digit_table(*bad), MSM_E_ARG, b"bad args")
    assert all((d.m, d.b, d.alpha) == (0, 0, 0) for d in out)
    assert L.msm_ches_digit_table(q, a_h, out) == MSM_OK
    from msm_blst_amd.ches import bucket_set
    B = set(bucket_set(q, a_h))
    for d in range(q + 1):  # d = m b, or q - d = m b with a carry
        h = out[d]
        assert h.m in (1, 2, 3) and h.alpha in (0, 1) and h.b in B
        assert h.m * h.b == (q - d if h.alpha else d)
