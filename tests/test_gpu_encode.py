"""GPU parity of the bulk point encoding (msm_points_encode; csrc/encode.hip and
the encoded kinds of the inversion tree, csrc/to_affine.hip) on an MI355X.

Oracle: the plain-Python encoder of tests/enc_inputs.py / tests/enc_special.py,
which tests/golden/encode.json pins to the reference's own four functions
(test_encode_host.py).  Every comparison is byte for byte.
"""
import ctypes
import threading

import pytest

import enc_inputs as ei
import enc_special as es
import jac_inputs as ji
import mult_inputs as mi

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 127, 129, 1000]
NMAX = 2049  # Jacobians: the smallest n with two tree levels above the points (257, then 33)

_SRC, _WANT = {}, {}


@pytest.fixture(scope="module")
def m():
    import msm_blst_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible")
    return m


def source(group, n, jacobian):
    """the first n signed fixed points, affine or as Jacobians with random Z (computed once, never modified)"""
    if (group, False) not in _SRC:
        aff = b"".join(ei.affine_bytes(group, pt) for pt in es.signed_points(group, NMAX))
        _SRC[(group, False)] = aff
        _SRC[(group, True)] = ji.jacobians(group, aff, NMAX, 0x5eed + group)
    return _SRC[(group, jacobian)][:n * (ji.JAC if jacobian else ei.AFF)[group]]


def want(group, n, compressed):
    if (group, compressed) not in _WANT:
        _WANT[(group, compressed)] = b"".join(ei.encode_point(group, pt, compressed)
                                              for pt in es.signed_points(group, NMAX))
    return _WANT[(group, compressed)][:n * ei.ENC[group] * (1 if compressed else 2)]


def assert_entries(got, exp, group, compressed, names=None):
    E = ei.ENC[group] * (1 if compressed else 2)
    assert len(got) == len(exp)
    bad = [(i, names[i] if names else "") for i in range(len(exp) // E) if got[i * E:(i + 1) * E] != exp[i * E:(i + 1) * E]]
    assert not bad, f"{len(bad)} differing entries, first (index, class): {bad[:8]}"


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("compressed", [True, False])
@pytest.mark.parametrize("jacobian", [False, True])
def test_sizes(m, group, compressed, jacobian):
    for n in SIZES + ([NMAX] if jacobian else []):
        got = m.ps_encode(group, source(group, n, jacobian), n, compressed=compressed, jacobian=jacobian)
        assert_entries(got, want(group, n, compressed), group, compressed)


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("form", es.FORMS)
@pytest.mark.parametrize("encoding", ["compressed", "serialized"])
def test_special_batches(m, golden, group, form, encoding):
    c = [c for c in golden("encode.json")["cases"]
         if c["group"] == group and c["form"] == form and c["encoding"] == encoding][0]
    compressed = encoding == "compressed"
    raw, n, jac = es.batch(group, form)
    names = {"affine": es.affine_batch(group)[1], "jacobian": es.jacobian_batch(group)[1]}.get(form)
    got = m.ps_encode(group, raw, n, compressed=compressed, jacobian=jac)
    assert_entries(got, es.expected(group, raw, n, compressed, jac), group, compressed, names)
    E = ei.ENC[group] * (1 if compressed else 2)
    assert bytes(got[i * E] for i in range(n)).hex() == c["first"]
    assert ei.fnv(got) == c["fnv"]


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("jacobian", [False, True])
def test_chunks(m, group, jacobian, monkeypatch):
    n = 1000
    monkeypatch.setenv("MSM_ENCODE_CHUNK", "96")  # ten full chunks and a partial one
    for compressed in (True, False):
        got = m.ps_encode(group, source(group, n, jacobian), n, compressed=compressed, jacobian=jacobian)
        assert_entries(got, want(group, n, compressed), group, compressed)
    # a special batch split inside its infinity run
    monkeypatch.setenv("MSM_ENCODE_CHUNK", "45")
    raw, ns, jac = es.batch(group, "jacobian" if jacobian else "affine")
    assert_entries(m.ps_encode(group, raw, ns, jacobian=jac), es.expected(group, raw, ns, True, jac), group, True)


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("jacobian", [False, True])
@pytest.mark.parametrize("path", ["d2d", "h2d", "d2h"])
def test_device_memory_on_a_stream(m, group, jacobian, path):
    """Source written by a torch copy queued on a non-default stream just before
    the call (behind a device-side delay): the call must order itself after it."""
    import torch
    n = 1000
    src_b, exp = source(group, n, jacobian), want(group, n, True)
    dev = torch.device("cuda:0")
    pinned = torch.frombuffer(bytearray(src_b), dtype=torch.uint8).pin_memory()
    d_in = torch.frombuffer(bytearray(src_b), dtype=torch.uint8).to(dev)
    d_src = torch.zeros(len(src_b), dtype=torch.uint8, device=dev)
    h_src = torch.zeros(len(src_b), dtype=torch.uint8).pin_memory()
    d_dst = torch.zeros(len(exp), dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        torch.cuda._sleep(10_000_000)
        if path == "h2d":
            h_src.copy_(d_in, non_blocking=True)
            src = (ctypes.c_uint8 * len(src_b)).from_address(h_src.data_ptr())
            got = m.ps_encode(group, src, n, jacobian=jacobian, dst=d_dst.data_ptr(), stream=st.cuda_stream)
        else:
            d_src.copy_(pinned, non_blocking=True)
            if path == "d2d":
                got = m.ps_encode(group, d_src.data_ptr(), n, jacobian=jacobian, src_on_device=True,
                                  dst=d_dst.data_ptr(), stream=st.cuda_stream)
            else:
                got = m.ps_encode(group, d_src.data_ptr(), n, jacobian=jacobian, src_on_device=True,
                                  stream=st.cuda_stream)
    st.synchronize()
    if got is None:
        got = bytes(d_dst.cpu().numpy())
    assert_entries(got, exp, group, True)


def test_device_destination_at_a_4_byte_offset(m):
    """a device dst that is 4-byte but not 8-byte aligned (entries of 48 bytes pack at any word)"""
    import torch
    n = 65
    for group in (1, 2):
        exp = want(group, n, False)
        d_dst = torch.zeros(len(exp) + 8, dtype=torch.uint8, device="cuda:0")
        assert d_dst.data_ptr() % 8 == 0
        m.ps_encode(group, source(group, n, True), n, compressed=False, jacobian=True, dst=d_dst.data_ptr() + 4)
        torch.cuda.synchronize()
        out = bytes(d_dst.cpu().numpy())
        assert out[:4] == bytes(4) and out[-4:] == bytes(4)
        assert_entries(out[4:-4], exp, group, False)


def test_threads_and_engine_cache(m):
    n = 500
    jobs = [(1, False, True), (1, True, False), (1, False, False), (1, True, True)]  # (group, jacobian, compressed)
    E = {True: 48, False: 96}
    inputs = [source(1, 4 * n, jac)[t * n * (144 if jac else 96):(t + 1) * n * (144 if jac else 96)]
              for t, (_, jac, _) in enumerate(jobs)]
    exp = [want(1, 4 * n, comp)[t * n * E[comp]:(t + 1) * n * E[comp]] for t, (_, _, comp) in enumerate(jobs)]
    out = [None] * 4
    m.release_engine_cache()

    def work(t):
        g, jac, comp = jobs[t]
        out[t] = m.ps_encode(g, inputs[t], n, compressed=comp, jacobian=jac)

    ts = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for t in range(4):
        assert out[t] is not None
        assert_entries(out[t], exp[t], 1, jobs[t][2])
    live, idle, idle_bytes = m.engine_cache_stats()
    assert 1 <= idle <= 4 and live >= idle and idle_bytes > 0  # the encode engines, back in the pool
    m.release_engine_cache()
    assert m.engine_cache_stats()[1] == 0


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("compressed", [True, False])
def test_round_trips(m, group, compressed):
    n = 129
    P = bytes(m.fixed_points(group, n))
    assert P[:8 * ei.AFF[group]] == ei.fixed_affine(group, 8)
    enc = m.ps_encode(group, P, n, compressed=compressed)
    got, st = m.ps_decode(group, enc, n, compressed=compressed, check_group=True)
    assert st == bytes(n) and got == P
    # and from entries: the mixed batch's valid ones, infinity included
    data, _ = ei.mixed_batch(group, not compressed)
    aff, st = m.ps_decode(group, data, ei.MIXED_N, compressed=compressed, check_group=False)
    E = ei.ENC[group] * (1 if compressed else 2)
    again = m.ps_encode(group, aff, ei.MIXED_N, compressed=compressed)
    ok = [i for i in range(ei.MIXED_N) if st[i] == 0 and (compressed or not data[i * E] & 0x80)]
    assert len(ok) > 40
    for i in ok:
        assert again[i * E:(i + 1) * E] == data[i * E:(i + 1) * E], i


@pytest.mark.parametrize("group", [1, 2])
def test_mult_then_encode_on_one_stream(m, group):
    """ps_mult into a device buffer, ps_encode from it on the same stream, against the
    Python double-and-add oracle encoded in Python"""
    import torch
    n = 129
    pts = list(es.signed_points(group, n))
    ks = [k >> 192 for k in mi.gen_scalars(n, 11)]  # 63-bit scalars: a quick oracle
    ks[5], pts[77] = 0, None                         # infinity from a zero scalar and from an infinity input
    exp_pts = [mi.smul(group, p, k) for p, k in zip(pts, ks)]
    dev = torch.device("cuda:0")
    d_pts = torch.frombuffer(bytearray(mi.points_bytes(group, pts)), dtype=torch.uint8).to(dev)
    d_sc = torch.frombuffer(bytearray(mi.scalar_bytes(ks, 8)), dtype=torch.uint8).to(dev)
    d_aff = torch.zeros(n * ei.AFF[group], dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    for compressed in (True, False):
        d_enc = torch.zeros(n * ei.ENC[group] * (1 if compressed else 2), dtype=torch.uint8, device=dev)
        with torch.cuda.stream(st):
            m.ps_mult(group, d_pts.data_ptr(), d_sc.data_ptr(), n, nbits=64, stride=8, src_on_device=True,
                      dst=d_aff.data_ptr(), stream=st.cuda_stream)
            m.ps_encode(group, d_aff.data_ptr(), n, compressed=compressed, src_on_device=True, dst=d_enc.data_ptr(),
                        stream=st.cuda_stream)
        st.synchronize()
        exp = b"".join(ei.encode_point(group, p, compressed) for p in exp_pts)
        assert exp_pts[5] is None and exp_pts[77] is None and exp_pts[6] is not None
        assert_entries(bytes(d_enc.cpu().numpy()), exp, group, compressed)
