"""CPU-side checks of the bulk Jacobian -> affine entry points
(include/msm_mi355x.h: msm_p{1,2}s_to_affine, msm_points_to_affine,
msm_to_affine_levels; msm_blst_amd.ps_to_affine / to_affine_levels): argument
errors (returned before any device work), the empty call, the missing-device
code, the level plan and the Python wrapper's marshalling.  No GPU is used; the
GPU parity lives in test_gpu_to_affine.py."""
import ctypes

import pytest

import jac_inputs as ji

MSM_OK, MSM_E_ARG, MSM_E_NODEV = 0, -1, -3
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def m():
    import msm_blst_amd as m
    m.lib()
    return m


def _bufs(group, n):
    src = (ctypes.c_uint8 * (ji.JAC[group] * n))()
    dst = (ctypes.c_uint8 * (ji.AFF[group] * n))()
    return src, dst


def test_exported(m):
    assert "ps_to_affine" in m.__all__ and "to_affine_levels" in m.__all__
    assert "to_affine" in m.__all__  # the one-point helper stays


@pytest.mark.parametrize("group", [1, 2])
def test_empty_call_touches_nothing(m, group):
    L = m.lib()
    assert L.msm_points_to_affine(group, 0, None, None, 0, 0, 0, None) == MSM_OK
    assert L.msm_points_to_affine(group, 0, None, None, 0, 1, 1, None) == MSM_OK
    assert getattr(L, f"msm_p{group}s_to_affine")(None, None, 0) == MSM_OK
    assert m.ps_to_affine(group, b"", 0) == b""


@pytest.mark.parametrize("group", [1, 2])
def test_argument_errors(m, group):
    L = m.lib()
    src, dst = _bufs(group, 4)
    assert L.msm_points_to_affine(group, 0, None, src, 4, 0, 0, None) == MSM_E_ARG
    assert L.msm_points_to_affine(group, 0, dst, None, 4, 0, 0, None) == MSM_E_ARG
    assert L.msm_last_error()
    f = getattr(L, f"msm_p{group}s_to_affine")
    pp = (vp * 2)(ctypes.addressof(src), None)
    assert f(None, pp, 4) == MSM_E_ARG
    assert f(dst, None, 4) == MSM_E_ARG
    assert f(dst, (vp * 2)(None, None), 4) == MSM_E_ARG


def test_bad_group(m):
    L = m.lib()
    src, dst = _bufs(2, 4)
    for group in (0, 3, -1):
        assert L.msm_points_to_affine(group, 0, dst, src, 4, 0, 0, None) == MSM_E_ARG
        assert L.msm_points_to_affine(group, 0, None, None, 0, 0, 0, None) == MSM_E_ARG


@pytest.mark.parametrize("group", [1, 2])
def test_overlapping_host_ranges(m, group):
    L = m.lib()
    n = 8
    jac, aff = ji.JAC[group], ji.AFF[group]
    buf = (ctypes.c_uint8 * (jac * n + aff * n))()
    base = ctypes.addressof(buf)
    # dst inside the source, dst ending inside the source, source inside dst
    assert L.msm_points_to_affine(group, 0, vp(base), vp(base), n, 0, 0, None) == MSM_E_ARG
    assert L.msm_points_to_affine(group, 0, vp(base + jac * n - 8), vp(base), n, 0, 0, None) == MSM_E_ARG
    assert L.msm_points_to_affine(group, 0, vp(base), vp(base + aff * n - 8), n, 0, 0, None) == MSM_E_ARG
    f = getattr(L, f"msm_p{group}s_to_affine")
    assert f(vp(base + jac), (vp * 2)(base, None), n) == MSM_E_ARG
    # one pointer per point, the last one into dst
    ptrs = (vp * n)(*([base + jac * i for i in range(n - 1)] + [base + jac * n + aff]))
    assert f(vp(base + jac * n), ptrs, n) == MSM_E_ARG
    # a misaligned device pointer is an argument error too
    assert L.msm_points_to_affine(group, 0, vp(base + 1), vp(base + jac * n), n, 0, 1, None) == MSM_E_ARG


@pytest.mark.parametrize("group", [1, 2])
def test_no_such_device(m, group):
    L = m.lib()
    src, dst = _bufs(group, 4)
    nd = m.device_count()
    assert L.msm_points_to_affine(group, nd, dst, src, 4, 0, 0, None) == MSM_E_NODEV
    assert L.msm_points_to_affine(group, -1, dst, src, 4, 0, 0, None) == MSM_E_NODEV
    assert bytes(dst) == bytes(len(dst))
    with pytest.raises(m.MsmError):
        m.ps_to_affine(group, bytes(src), 4, device=nd)
    if nd == 0:  # the blst-style call uses the current device: none here
        pp = (vp * 2)(ctypes.addressof(src), None)
        assert getattr(L, f"msm_p{group}s_to_affine")(dst, pp, 4) == MSM_E_NODEV


def test_levels(m):
    assert m.to_affine_levels(0) == 0
    assert m.to_affine_levels(1) >= 1
    assert m.to_affine_levels(4099) >= 2
    prev = 0
    for n in list(range(1, 300)) + [511, 512, 513, 2048, 2049, 4099, 1 << 15, (1 << 18) - 1, 1 << 18, 1 << 20, 1 << 24]:
        lv = m.to_affine_levels(n)
        assert lv >= prev, n
        prev = lv


def test_levels_follow_the_chunk_override(m, monkeypatch):
    big = m.to_affine_levels(1 << 20)
    monkeypatch.setenv("MSM_TO_AFFINE_CHUNK", "96")  # read at each call
    assert m.to_affine_levels(1 << 20) == m.to_affine_levels(96) < big
    monkeypatch.delenv("MSM_TO_AFFINE_CHUNK")
    assert m.to_affine_levels(1 << 20) == big


class _FakeLib:
    def __init__(self):
        self.calls = []

    def msm_points_to_affine(self, *a):
        self.calls.append(a)
        return 0


def test_wrapper_marshalling(m, monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(m, "lib", lambda: fake)
    jac = bytes(range(144)) * 3
    out = m.ps_to_affine(1, jac, 3)
    assert isinstance(out, bytes) and len(out) == 3 * 96
    group, device, dst, src, n, s_dev, d_dev, stream = fake.calls[-1]
    assert (group, device, n, s_dev, d_dev, stream) == (1, 0, 3, 0, 0, None)
    assert bytes(src) == jac and ctypes.sizeof(dst) == 3 * 96
    # device destination: written there, nothing returned; device source passed through
    assert m.ps_to_affine(2, 0x7f0000001000, 5, src_on_device=True, dst=0x7f0000002000, device=1, stream=0x55) is None
    assert fake.calls[-1] == (2, 1, 0x7f0000002000, 0x7f0000001000, 5, 1, 1, 0x55)
    assert m.ps_to_affine(2, bytearray(288 * 2), 2, dst=0x7f0000002000) is None
    assert fake.calls[-1][5:7] == (0, 1) and bytes(fake.calls[-1][3]) == bytes(288 * 2)
    ncalls = len(fake.calls)
    with pytest.raises(ValueError):
        m.ps_to_affine(1, jac, 4)  # 3 points given
    with pytest.raises(ValueError):
        m.ps_to_affine(3, jac, 1)
    with pytest.raises(ValueError):
        m.ps_to_affine(1, jac, -1)
    assert len(fake.calls) == ncalls


@pytest.mark.parametrize("group,n", [(1, 40), (2, 24)])
def test_input_builder_against_the_one_point_host_helper(m, group, n):
    """tests/jac_inputs.py builds Jacobians of known affine form: the library's
    host msm_p{1,2}_to_affine (one Fermat inversion per point) returns the affine
    points they were built from."""
    aff = bytes(m.fixed_points(group, n))
    jac = ji.jacobians(group, aff, n, 99)
    J, A = ji.JAC[group], ji.AFF[group]
    assert len(jac) == n * J and jac[:A] != aff[:A]
    for i in range(n):
        assert m.to_affine(group, jac[i * J:(i + 1) * J]) == aff[i * A:(i + 1) * A], i
    z1 = ji.affine_to_jacobian_z1(group, aff, n)
    assert m.to_affine(group, z1[:J]) == aff[:A]
