"""CPU-side checks of the bulk point decoding entry points
(include/msm_mi355x.h: msm_points_decode, msm_ctx_set_points_encoded;
msm_blst_amd.ps_decode / MSMContext.set_points_encoded): exported symbols,
argument errors (returned before any device work), the empty call, the
missing-device code, the Python wrapper's length check -- and the plain-Python
decoder of tests/enc_inputs.py against the reference's recorded answers
(tests/golden/decode.json).  No GPU is used; the GPU parity lives in
test_gpu_decode.py."""
import ctypes

import pytest

import enc_inputs as ei

MSM_OK, MSM_E_ARG, MSM_E_NODEV = 0, -1, -3
COMPRESSED, SERIALIZED, CHECK_GROUP = 0, 1, 1
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def m():
    import msm_blst_amd as m
    m.lib()
    return m


def _bufs(group, n, encoding=COMPRESSED):
    src = (ctypes.c_uint8 * (ei.ENC[group] * (1 + encoding) * n))()
    dst = (ctypes.c_uint8 * (ei.AFF[group] * n))()
    st = (ctypes.c_uint8 * n)()
    return src, dst, st


def test_exported(m):
    L = m.lib()
    assert hasattr(L, "msm_points_decode") and hasattr(L, "msm_ctx_set_points_encoded")
    assert "ps_decode" in m.__all__ and "MSMContext" in m.__all__
    assert callable(m.MSMContext.set_points_encoded)
    assert (m.ENC_COMPRESSED, m.ENC_SERIALIZED, m.DECODE_CHECK_GROUP) == (COMPRESSED, SERIALIZED, CHECK_GROUP)


@pytest.mark.parametrize("group", [1, 2])
def test_empty_call_touches_nothing(m, group):
    L = m.lib()
    nbad = ctypes.c_size_t(77)
    for enc in (COMPRESSED, SERIALIZED):
        assert L.msm_points_decode(group, 0, None, None, ctypes.byref(nbad), None, 0, enc, CHECK_GROUP, 0, 0, None) == MSM_OK
        assert L.msm_points_decode(group, 0, None, None, None, None, 0, enc, 0, 1, 1, None) == MSM_OK
    assert nbad.value == 77
    assert m.ps_decode(group, b"", 0) == (b"", b"")
    assert m.ps_decode(group, b"", 0, compressed=False, check_group=False) == (b"", b"")


@pytest.mark.parametrize("group", [1, 2])
def test_argument_errors(m, group):
    L = m.lib()
    src, dst, st = _bufs(group, 4)

    def call(*a):
        rc = L.msm_points_decode(*a)
        if rc == MSM_E_ARG:
            assert L.msm_last_error()
        return rc

    assert call(group, 0, None, st, None, src, 4, COMPRESSED, 0, 0, 0, None) == MSM_E_ARG  # NULL dst
    assert b"null" in L.msm_last_error()
    assert call(group, 0, dst, st, None, None, 4, COMPRESSED, 0, 0, 0, None) == MSM_E_ARG  # NULL src
    assert call(group, 0, dst, st, None, src, 4, 2, 0, 0, 0, None) == MSM_E_ARG  # unknown encoding
    assert b"encoding" in L.msm_last_error()
    assert call(group, 0, dst, st, None, src, 4, -1, 0, 0, 0, None) == MSM_E_ARG
    assert call(group, 0, dst, st, None, src, 4, COMPRESSED, 2, 0, 0, None) == MSM_E_ARG  # unknown flag bits
    assert b"flag" in L.msm_last_error()
    assert call(group, 0, dst, st, None, src, 4, COMPRESSED, CHECK_GROUP | 0x100, 0, 0, None) == MSM_E_ARG
    assert bytes(dst) == bytes(len(dst)) and bytes(st) == bytes(4)


def test_bad_group(m):
    L = m.lib()
    src, dst, st = _bufs(2, 4)
    for group in (0, 3, -1):
        assert L.msm_points_decode(group, 0, dst, st, None, src, 4, COMPRESSED, 0, 0, 0, None) == MSM_E_ARG
        assert b"group" in L.msm_last_error()
        assert L.msm_points_decode(group, 0, None, None, None, None, 0, COMPRESSED, 0, 0, 0, None) == MSM_E_ARG


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("encoding", [COMPRESSED, SERIALIZED])
def test_overlapping_host_ranges(m, group, encoding):
    L = m.lib()
    n = 8
    enc, aff = ei.ENC[group] * (1 + encoding), ei.AFF[group]
    buf = (ctypes.c_uint8 * (enc * n + aff * n + n))()
    base = ctypes.addressof(buf)
    st = vp(base + enc * n + aff * n)

    def call(dst, status, src):
        rc = L.msm_points_decode(group, 0, vp(dst), status, None, vp(src), n, encoding, 0, 0, 0, None)
        if rc == MSM_E_ARG:
            assert b"overlap" in L.msm_last_error()
        return rc

    # dst on the source, dst ending inside the source, source ending inside dst
    assert call(base, st, base) == MSM_E_ARG
    assert call(base + enc * n - 8, None, base) == MSM_E_ARG
    assert call(base, None, base + aff * n - 8) == MSM_E_ARG
    # status inside the source, status inside dst
    assert call(base + enc * n, vp(base + 8), base) == MSM_E_ARG
    assert call(base + enc * n, vp(base + enc * n + 8), base) == MSM_E_ARG
    # a misaligned device pointer is an argument error too
    assert L.msm_points_decode(group, 0, vp(base + 1), None, None, vp(base + 64), n, encoding, 0, 0, 1, None) == MSM_E_ARG
    assert L.msm_points_decode(group, 0, vp(base + 64), None, None, vp(base + 2), n, encoding, 0, 1, 0, None) == MSM_E_ARG


@pytest.mark.parametrize("group", [1, 2])
def test_no_such_device(m, group):
    L = m.lib()
    src, dst, st = _bufs(group, 4)
    nd = m.device_count()
    for dev in (nd, -1):
        assert L.msm_points_decode(group, dev, dst, st, None, src, 4, COMPRESSED, 0, 0, 0, None) == MSM_E_NODEV
    assert bytes(dst) == bytes(len(dst))
    with pytest.raises(m.MsmError):
        m.ps_decode(group, bytes(src), 4, device=nd)


class _FakeLib:
    def __init__(self):
        self.calls = []

    def msm_points_decode(self, *a):
        self.calls.append(a)
        return 0


def test_wrapper_marshalling_and_length_check(m, monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(m, "lib", lambda: fake)
    enc = bytes(range(48)) * 3
    out, st = m.ps_decode(1, enc, 3)
    assert (len(out), len(st)) == (3 * 96, 3)
    group, device, dst, status, nbad, src, n, encoding, flags, s_dev, d_dev, stream = fake.calls[-1]
    assert (group, device, nbad, n, encoding, flags, s_dev, d_dev, stream) == (1, 0, None, 3, 0, 1, 0, 0, None)
    assert bytes(src) == enc and ctypes.sizeof(dst) == 3 * 96 and ctypes.sizeof(status) == 3
    # serialized, no group check, device source and destination
    out, st = m.ps_decode(2, 0x7f0000001000, 5, compressed=False, check_group=False, src_on_device=True,
                          dst=0x7f0000002000, device=1, stream=0x55)
    assert out is None and st == bytes(5)
    assert fake.calls[-1][:3] == (2, 1, 0x7f0000002000) and fake.calls[-1][5:] == (0x7f0000001000, 5, 1, 0, 1, 1, 0x55)
    ncalls = len(fake.calls)
    with pytest.raises(ValueError):
        m.ps_decode(1, enc, 4)  # 3 entries given
    with pytest.raises(ValueError):
        m.ps_decode(1, enc, 2, compressed=False)  # 1.5 serialized entries given
    with pytest.raises(ValueError):
        m.ps_decode(2, bytes(96 * 2 - 1), 2)
    with pytest.raises(ValueError):
        m.ps_decode(3, enc, 1)
    with pytest.raises(ValueError):
        m.ps_decode(1, enc, -1)
    assert len(fake.calls) == ncalls


def test_set_points_encoded_argument_errors(m):
    L = m.lib()
    assert L.msm_ctx_set_points_encoded(None, None, 0, COMPRESSED, 0, 0, None, None) == MSM_E_ARG
    assert L.msm_last_error()


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("encoding", ["compressed", "serialized"])
def test_python_decoder_reproduces_the_reference(golden, group, encoding):
    """tests/enc_inputs.py (plain integers: pow(a, (p+1)//4, p), an Fp2 root through
    the norm, the sign rules, [r]P) against the reference's recorded statuses,
    subgroup Booleans and output hashes on the mixed batch."""
    c = [c for c in golden("decode.json")["cases"] if c["group"] == group and c["encoding"] == encoding][0]
    ser = encoding == "serialized"
    data, names = ei.mixed_batch(group, ser)
    assert c["n"] == ei.MIXED_N == len(names) and len(data) == ei.MIXED_N * ei.ENC[group] * (2 if ser else 1)
    st, out = ei.expected(group, ser, False)
    assert st == c["status"]
    assert ei.fnv(out) == c["fnv"]
    A = ei.AFF[group]
    assert [ei.in_group(group, out[i * A:(i + 1) * A]) if s == 0 else None for i, s in enumerate(st)] == c["in_group"]
    st_g, out_g = ei.expected(group, ser, True)
    assert st_g == [3 if g is False else s for s, g in zip(c["status"], c["in_group"])]
    assert ei.fnv(out_g) == c["fnv_group"]
    # every class of the issue's table occurs, with its status
    by_name = {}
    for nm, s, sg in zip(names, st, st_g):
        by_name.setdefault(nm.replace("compressed_in_serialized_", ""), set()).add((s, sg))
    assert by_name["good"] == {(0, 0)} and by_name["infinity"] == {(0, 0)}
    assert by_name["off_curve"] == {(2, 2)} and by_name["off_group"] == {(0, 3)}
    assert by_name["x_zero"] == ({(3, 3)} if group == 1 else {(2, 2)})
    assert by_name["infinity_stray_low_bit"] == {(1, 1)}
    if ser:
        assert by_name["y_plus_one"] == {(2, 2)} and by_name["sign_flag_alone"] == {(1, 1)}
        assert by_name["y_eq_p" if group == 1 else "y1_eq_p"] == {(1, 1)}
    else:
        assert by_name["compressed_bit_clear"] == {(1, 1)}
    assert by_name["x_ge_p_0" if group == 1 else "x1_ge_p_0"] == {(1, 1)}


@pytest.mark.parametrize("group", [1, 2])
def test_encode_round_trip_in_python(group):
    aff = ei.fixed_affine(group, 6)
    for compressed in (True, False):
        enc = ei.encode(group, aff, 6, compressed)
        assert len(enc) == 6 * ei.ENC[group] * (1 if compressed else 2)
        st, out = ei.decode(group, enc, 6, not compressed)
        assert st == [0] * 6 and out == aff
