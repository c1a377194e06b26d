"""CPU-side checks of the bulk scalar multiplication entry point
(include/msm_mi355x.h: msm_points_mult; msm_blst_amd.ps_mult): exported symbol,
flag value, argument errors (returned before any device work), the empty call, the
missing-device code, the Python wrapper's checks -- and the plain-Python
double-and-add of tests/mult_inputs.py against the reference's recorded answers
(tests/golden/points_mult.json).  No GPU is used; the GPU parity lives in
test_gpu_points_mult.py."""
import ctypes

import pytest

import enc_inputs as ei
import mult_inputs as mi

MSM_OK, MSM_E_ARG, MSM_E_NODEV = 0, -1, -3
ONE_POINT = 1
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def m():
    import msm_blst_amd as m
    m.lib()
    return m


def _bufs(group, n, stride=32):
    pts = (ctypes.c_uint8 * (ei.AFF[group] * n))()
    sc = (ctypes.c_uint8 * (stride * n))()
    dst = (ctypes.c_uint8 * (ei.AFF[group] * n))()
    return pts, sc, dst


def test_exported(m):
    assert hasattr(m.lib(), "msm_points_mult")
    assert "ps_mult" in m.__all__ and callable(m.ps_mult)
    assert m.MULT_ONE_POINT == ONE_POINT
    assert "ps_mult" in m.__doc__


@pytest.mark.parametrize("group", [1, 2])
def test_empty_call_touches_nothing(m, group):
    L = m.lib()
    for flags in (0, ONE_POINT):
        assert L.msm_points_mult(group, 0, None, None, None, 0, 255, 32, flags, 0, 0, None) == MSM_OK
        assert L.msm_points_mult(group, 0, None, None, None, 0, 0, 0, flags, 1, 1, None) == MSM_OK
    assert m.ps_mult(group, b"", b"", 0) == b""
    assert m.ps_mult(group, b"", b"", 0, one_point=True, nbits=0, stride=0) == b""


@pytest.mark.parametrize("group", [1, 2])
def test_argument_errors(m, group):
    L = m.lib()
    pts, sc, dst = _bufs(group, 4)

    def call(*a):
        rc = L.msm_points_mult(*a)
        if rc == MSM_E_ARG:
            assert L.msm_last_error()
        return rc

    assert call(group, 0, None, pts, sc, 4, 255, 32, 0, 0, 0, None) == MSM_E_ARG  # NULL dst
    assert b"null" in L.msm_last_error()
    assert call(group, 0, dst, None, sc, 4, 255, 32, 0, 0, 0, None) == MSM_E_ARG  # NULL points
    assert call(group, 0, dst, pts, None, 4, 255, 32, 0, 0, 0, None) == MSM_E_ARG  # NULL scalars
    assert call(group, 0, dst, pts, sc, 4, 257, 33, 0, 0, 0, None) == MSM_E_ARG  # nbits > 256
    assert b"nbits" in L.msm_last_error()
    assert call(group, 0, dst, pts, sc, 4, 255, 31, 0, 0, 0, None) == MSM_E_ARG  # stride too short
    assert b"stride" in L.msm_last_error()
    assert call(group, 0, dst, pts, sc, 4, 9, 1, 0, 0, 0, None) == MSM_E_ARG
    assert call(group, 0, dst, pts, sc, 4, 255, 32, 2, 0, 0, None) == MSM_E_ARG  # unknown flag bits
    assert b"flag" in L.msm_last_error()
    assert call(group, 0, dst, pts, sc, 4, 255, 32, ONE_POINT | 0x100, 0, 0, None) == MSM_E_ARG
    assert bytes(dst) == bytes(len(dst))
    # host ranges: dst on the points, dst on the scalars; misaligned device pointers
    base = ctypes.addressof(pts)
    assert call(group, 0, vp(base), pts, sc, 4, 255, 32, 0, 0, 0, None) == MSM_E_ARG
    assert b"overlap" in L.msm_last_error()
    assert call(group, 0, vp(ctypes.addressof(sc)), pts, sc, 1, 255, 32, 0, 0, 0, None) == MSM_E_ARG
    assert call(group, 0, vp(base + 1), pts, sc, 4, 255, 32, 0, 0, 1, None) == MSM_E_ARG
    assert call(group, 0, dst, vp(base + 2), sc, 4, 255, 32, 0, 1, 0, None) == MSM_E_ARG


def test_bad_group(m):
    L = m.lib()
    pts, sc, dst = _bufs(2, 4)
    for group in (0, 3, -1):
        assert L.msm_points_mult(group, 0, dst, pts, sc, 4, 255, 32, 0, 0, 0, None) == MSM_E_ARG
        assert b"group" in L.msm_last_error()
        assert L.msm_points_mult(group, 0, None, None, None, 0, 255, 32, 0, 0, 0, None) == MSM_E_ARG


@pytest.mark.parametrize("group", [1, 2])
def test_no_such_device(m, group):
    L = m.lib()
    pts, sc, dst = _bufs(group, 4)
    nd = m.device_count()
    for dev in (nd, -1):
        assert L.msm_points_mult(group, dev, dst, pts, sc, 4, 255, 32, 0, 0, 0, None) == MSM_E_NODEV
        assert L.msm_points_mult(group, dev, dst, pts, sc, 4, 0, 0, ONE_POINT, 0, 0, None) == MSM_E_NODEV
    assert bytes(dst) == bytes(len(dst))
    with pytest.raises(m.MsmError):
        m.ps_mult(group, bytes(pts), bytes(sc), 4, device=nd)


class _FakeLib:
    def __init__(self):
        self.calls = []

    def msm_points_mult(self, *a):
        self.calls.append(a)
        return 0


def test_wrapper_marshalling_and_checks(m, monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(m, "lib", lambda: fake)
    pts, sc = bytes(range(96)) * 3, bytes(range(32)) * 3
    out = m.ps_mult(1, pts, sc, 3)
    assert len(out) == 3 * 96
    group, device, dst, p, s, n, nbits, stride, flags, s_dev, d_dev, stream = fake.calls[-1]
    assert (group, device, n, nbits, stride, flags, s_dev, d_dev, stream) == (1, 0, 3, 255, 32, 0, 0, 0, None)
    assert bytes(p) == pts and bytes(s) == sc and ctypes.sizeof(dst) == 3 * 96
    # one point, narrow scalars packed tight: the last scalar may end the buffer
    out = m.ps_mult(2, bytes(192), bytes(2 * 9 + 8), 3, nbits=64, stride=9, one_point=True)
    assert len(out) == 3 * 192 and fake.calls[-1][5:9] == (3, 64, 9, ONE_POINT)
    # device sources and destination
    assert m.ps_mult(2, 0x7f0000001000, 0x7f0000003000, 5, src_on_device=True, dst=0x7f0000002000, device=1,
                     stream=0x55) is None
    assert fake.calls[-1] == (2, 1, 0x7f0000002000, 0x7f0000001000, 0x7f0000003000, 5, 255, 32, 0, 1, 1, 0x55)
    ncalls = len(fake.calls)
    with pytest.raises(ValueError):
        m.ps_mult(1, pts, sc, 4)  # 3 points given
    with pytest.raises(ValueError):
        m.ps_mult(1, pts + pts, sc, 4)  # 3 scalars given
    with pytest.raises(ValueError):
        m.ps_mult(2, bytes(191), sc, 3, one_point=True)
    with pytest.raises(ValueError):
        m.ps_mult(1, pts, sc, 3, nbits=64, stride=7)
    with pytest.raises(ValueError):
        m.ps_mult(1, pts, sc, 3, nbits=257, stride=40)
    with pytest.raises(ValueError):
        m.ps_mult(3, pts, sc, 1)
    with pytest.raises(ValueError):
        m.ps_mult(1, pts, sc, -1)
    assert len(fake.calls) == ncalls


def test_gen_scalars_in_python(m):
    assert mi.scalar_bytes(mi.gen_scalars(40, 1)) == bytes(m.gen_scalars(40, 1))
    assert mi.scalar_bytes(mi.gen_scalars(5, 3)) == bytes(m.gen_scalars(5, 3))


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("nbits", [255, 256])
def test_smul_reproduces_the_reference(golden, group, nbits):
    """tests/mult_inputs.py smul (double-and-add on Jacobians in plain integers)
    against the reference's recorded blst_p{1,2}_mult results on the in-group
    entries of the special batch."""
    c = [c for c in golden("points_mult.json")["special"] if c["group"] == group and c["nbits"] == nbits][0]
    names, pts, ks, ing, exp = mi.expected_batch(group, nbits)
    assert c["n"] == mi.SPECIAL_N == len(names)
    idx = [i for i in range(len(ks)) if ing[i]]
    assert idx == c["in_group"]
    for i, want in zip(idx, c["compressed"]):
        assert ei.encode(group, exp[i], 1).hex() == want, (i, names[i])
    assert ei.fnv(b"".join(exp[i] for i in idx)) == c["fnv"]
    # the batch holds what the issue asks for
    assert all(k < (1 << nbits) for k in ks)
    assert {"0@gen", "infinity*random", "random"} <= set(names)
    assert any(n.startswith("r@") for n in names) and any(n.startswith("2^254-1@") for n in names)
    assert any(n.startswith("2r@") for n in names) == (nbits == 256)
    q = {1: (3, 11), 2: (13, 23)}[group]
    for o in q:
        assert {f"order{o}*{s}" for s in ("0", "q", "q-1", "q+1", "2^255-1", "random0")} <= set(names)
    # small order: [q]T = infinity, [q + 1]T = T, [q - 1]T = -T
    for o, t in mi.small_order_points(group):
        assert ei.f_mul(group, t[1], t[1]) == ei.curve_rhs(group, t[0]) and not ei.scalar_mul_is_inf(group, t, ei.R)
        assert mi.smul(group, t, o) is None and mi.smul(group, t, o + 1) == t
        assert mi.smul(group, t, o - 1) == (t[0], ei.f_neg(group, t[1]))
    inf = [i for i in range(len(ks)) if not any(exp[i])]
    assert len(inf) >= 15 and any(0 < i < len(ks) - 1 and any(exp[i - 1]) and any(exp[i + 1]) for i in inf)
