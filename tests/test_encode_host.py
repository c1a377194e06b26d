"""CPU-side checks of the bulk point encoding entry point
(include/msm_mi355x.h: msm_points_encode; msm_blst_amd.ps_encode): exported
symbols, argument errors (returned before any device work), the empty call, the
missing-device code, the Python wrapper's length check -- and the plain-Python
encoder (tests/enc_inputs.py, tests/enc_special.py) against the reference's
recorded answers (tests/golden/encode.json).  No GPU is used; the GPU parity
lives in test_gpu_encode.py."""
import ctypes

import pytest

import enc_inputs as ei
import enc_special as es
import jac_inputs as ji

MSM_OK, MSM_E_ARG, MSM_E_NODEV = 0, -1, -3
AFFINE, JACOBIAN = 0, 1
COMPRESSED, SERIALIZED = 0, 1
vp = ctypes.c_void_p
FILL = 0xa5


@pytest.fixture(scope="module")
def m():
    import msm_blst_amd as m
    m.lib()
    return m


def _bufs(group, n, form=AFFINE, encoding=COMPRESSED):
    src = (ctypes.c_uint8 * ((ji.JAC if form else ei.AFF)[group] * n))()
    dst = (ctypes.c_uint8 * (ei.ENC[group] * (1 + encoding) * n))(*([FILL] * (ei.ENC[group] * (1 + encoding) * n)))
    return src, dst


def test_exported(m):
    L = m.lib()
    assert hasattr(L, "msm_points_encode")
    assert "ps_encode" in m.__all__ and "SRC_AFFINE" in m.__all__ and "SRC_JACOBIAN" in m.__all__
    assert (m.SRC_AFFINE, m.SRC_JACOBIAN) == (AFFINE, JACOBIAN)
    assert callable(m.ps_encode)


@pytest.mark.parametrize("group", [1, 2])
def test_empty_call_touches_nothing(m, group):
    L = m.lib()
    _, dst = _bufs(group, 1)
    for form in (AFFINE, JACOBIAN):
        for enc in (COMPRESSED, SERIALIZED):
            assert L.msm_points_encode(group, 0, None, None, 0, form, enc, 0, 0, 0, None) == MSM_OK
            assert L.msm_points_encode(group, 0, dst, None, 0, form, enc, 0, 1, 1, None) == MSM_OK
    assert bytes(dst) == bytes([FILL]) * len(dst)
    assert m.ps_encode(group, b"", 0) == b""
    assert m.ps_encode(group, b"", 0, compressed=False, jacobian=True) == b""


@pytest.mark.parametrize("group", [1, 2])
def test_argument_errors(m, group):
    L = m.lib()
    src, dst = _bufs(group, 4, JACOBIAN, SERIALIZED)

    def call(*a):
        rc = L.msm_points_encode(*a)
        if rc == MSM_E_ARG:
            assert L.msm_last_error()
        return rc

    assert call(group, 0, None, src, 4, AFFINE, COMPRESSED, 0, 0, 0, None) == MSM_E_ARG  # NULL dst
    assert b"null" in L.msm_last_error()
    assert call(group, 0, dst, None, 4, AFFINE, COMPRESSED, 0, 0, 0, None) == MSM_E_ARG  # NULL src
    assert b"null" in L.msm_last_error()
    for form in (2, -1):
        assert call(group, 0, dst, src, 4, form, COMPRESSED, 0, 0, 0, None) == MSM_E_ARG  # unknown source form
        assert b"form" in L.msm_last_error()
    for enc in (2, -1):
        assert call(group, 0, dst, src, 4, JACOBIAN, enc, 0, 0, 0, None) == MSM_E_ARG  # unknown encoding
        assert b"encoding" in L.msm_last_error()
    for flags in (1, 0x100, -1):
        assert call(group, 0, dst, src, 4, AFFINE, SERIALIZED, flags, 0, 0, None) == MSM_E_ARG  # flags must be 0
        assert b"flag" in L.msm_last_error()
    assert bytes(dst) == bytes([FILL]) * len(dst)


def test_bad_group(m):
    L = m.lib()
    src, dst = _bufs(2, 4)
    for group in (0, 3, -1):
        assert L.msm_points_encode(group, 0, dst, src, 4, AFFINE, COMPRESSED, 0, 0, 0, None) == MSM_E_ARG
        assert b"group" in L.msm_last_error()
        assert L.msm_points_encode(group, 0, None, None, 0, AFFINE, COMPRESSED, 0, 0, 0, None) == MSM_E_ARG
    assert bytes(dst) == bytes([FILL]) * len(dst)


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("form", [AFFINE, JACOBIAN])
@pytest.mark.parametrize("encoding", [COMPRESSED, SERIALIZED])
def test_overlapping_host_ranges(m, group, form, encoding):
    L = m.lib()
    n = 8
    pt, enc = (ji.JAC if form else ei.AFF)[group], ei.ENC[group] * (1 + encoding)
    buf = (ctypes.c_uint8 * (pt * n + enc * n))()
    base = ctypes.addressof(buf)

    def call(dst, src):
        rc = L.msm_points_encode(group, 0, vp(dst), vp(src), n, form, encoding, 0, 0, 0, None)
        if rc == MSM_E_ARG:
            assert b"overlap" in L.msm_last_error()
        return rc

    # dst on the source, dst starting inside the source's last bytes, source starting inside dst's last bytes
    assert call(base, base) == MSM_E_ARG
    assert call(base + pt * n - 8, base) == MSM_E_ARG
    assert call(base, base + enc * n - 8) == MSM_E_ARG
    assert bytes(buf) == bytes(len(buf))
    # a misaligned device pointer is an argument error too: src 8 bytes, dst 4 bytes
    assert L.msm_points_encode(group, 0, vp(base + 2), vp(base + 64), n, form, encoding, 0, 0, 1, None) == MSM_E_ARG
    assert L.msm_points_encode(group, 0, vp(base + 64), vp(base + 4), n, form, encoding, 0, 1, 0, None) == MSM_E_ARG


@pytest.mark.parametrize("group", [1, 2])
def test_no_such_device(m, group):
    L = m.lib()
    src, dst = _bufs(group, 4)
    nd = m.device_count()
    for dev in (nd, -1):
        assert L.msm_points_encode(group, dev, dst, src, 4, AFFINE, COMPRESSED, 0, 0, 0, None) == MSM_E_NODEV
    assert bytes(dst) == bytes([FILL]) * len(dst)
    with pytest.raises(m.MsmError):
        m.ps_encode(group, bytes(src), 4, device=nd)


class _FakeLib:
    def __init__(self):
        self.calls = []

    def msm_points_encode(self, *a):
        self.calls.append(a)
        return 0


def test_wrapper_marshalling_and_length_check(m, monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(m, "lib", lambda: fake)
    aff = bytes(range(96)) * 3
    out = m.ps_encode(1, aff, 3)
    assert len(out) == 3 * 48
    group, device, dst, src, n, form, encoding, flags, s_dev, d_dev, stream = fake.calls[-1]
    assert (group, device, n, form, encoding, flags, s_dev, d_dev, stream) == (1, 0, 3, 0, 0, 0, 0, 0, None)
    assert bytes(src) == aff and ctypes.sizeof(dst) == 3 * 48
    assert len(m.ps_encode(2, bytes(288 * 2), 2, compressed=False, jacobian=True)) == 2 * 192
    assert fake.calls[-1][4:8] == (2, 1, 1, 0) and ctypes.sizeof(fake.calls[-1][2]) == 2 * 192
    # serialized Jacobians, device source and destination
    out = m.ps_encode(2, 0x7f0000001000, 5, compressed=False, jacobian=True, src_on_device=True,
                      dst=0x7f0000002000, device=1, stream=0x55)
    assert out is None
    assert fake.calls[-1] == (2, 1, 0x7f0000002000, 0x7f0000001000, 5, 1, 1, 0, 1, 1, 0x55)
    ncalls = len(fake.calls)
    with pytest.raises(ValueError):
        m.ps_encode(1, aff, 4)  # 3 points given
    with pytest.raises(ValueError):
        m.ps_encode(1, aff, 3, jacobian=True)  # 2 Jacobians given
    with pytest.raises(ValueError):
        m.ps_encode(2, bytes(192 * 2 - 1), 2)
    with pytest.raises(ValueError):
        m.ps_encode(3, aff, 1)
    with pytest.raises(ValueError):
        m.ps_encode(1, aff, -1)
    assert len(fake.calls) == ncalls


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("form", es.FORMS)
@pytest.mark.parametrize("encoding", ["compressed", "serialized"])
def test_python_encoder_reproduces_the_reference(golden, group, form, encoding):
    """enc_inputs.encode_point with enc_special's sign rule for stored limbs (plain
    integers; Jacobians normalised with pow(z, -1, p)) against the reference's
    recorded output hash and flag bytes on every batch."""
    c = [c for c in golden("encode.json")["cases"]
         if c["group"] == group and c["form"] == form and c["encoding"] == encoding][0]
    compressed = encoding == "compressed"
    raw, n, jac = es.batch(group, form)
    E = ei.ENC[group] * (1 if compressed else 2)
    out = es.expected(group, raw, n, compressed, jac)
    assert c["n"] == n and len(out) == n * E
    assert bytes(out[i * E] for i in range(n)).hex() == c["first"]
    assert ei.fnv(out) == c["fnv"]


@pytest.mark.parametrize("group", [1, 2])
def test_batches_hold_every_class(group):
    raw, names = es.affine_batch(group)
    n, A, E = es.SPECIAL_N, ei.AFF[group], ei.ENC[group]
    assert len(names) == n and len(raw) == n * A
    inf = [i for i, nm in enumerate(names) if nm == "infinity"]
    assert inf[0] == 0 and inf[-1] == n - 1 and len(inf) == 11
    assert any(all(i + k in inf for k in range(9)) for i in inf)
    for nm in ("good", "x_zero_y_two", "off_curve", "off_group", "x_boundary", "x_plus_p", "y_plus_p",
               "limbs_of_p"):
        assert nm in names, nm
    out = es.expected(group, raw, n, True)
    first = {nm: set() for nm in names}
    for i, nm in enumerate(names):
        first[nm].add(out[i * E] & 0xe0)
    assert first["infinity"] == {0xc0} and first["good"] == {0x80, 0xa0}
    assert first["x_zero_y_two"] == {0x80}  # X all zero, Y not: a finite entry
    assert first["limbs_of_p"] == {0xa0}    # value zero, sign set (the reference's rule)
    ser = es.expected(group, raw, n, False)
    assert all(ser[i * 2 * E] == (0x40 if nm == "infinity" else ser[i * 2 * E] & 0x1f) for i, nm in enumerate(names))
    jac, jn = es.jacobian_batch(group)
    assert len(jac) == es.JAC_N * ji.JAC[group]
    zero = [i for i, nm in enumerate(jn) if nm == "z_zero"]
    assert zero == [0] + list(range(8, 16)) + [es.JAC_N - 1] and "z_one" in jn
    J, co = ji.JAC[group], 48 * group
    assert all(any(jac[i * J:i * J + co]) and any(jac[i * J + co:i * J + 2 * co]) for i in zero)  # X, Y left in place
