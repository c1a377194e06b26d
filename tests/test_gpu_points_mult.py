"""GPU parity of the bulk scalar multiplication (msm_points_mult / ps_mult;
csrc/points_mult.hip) on an MI355X.

Oracles: tests/mult_inputs.py smul, double-and-add in plain Python integers, for
every entry (the only oracle for the points of small order outside the subgroup);
tests/golden/points_mult.json holds the reference's own blst_p{1,2}_mult results
on the in-group entries of the special batch and the hashes of two 1000-point
runs.
"""
import ctypes
import threading

import pytest

import enc_inputs as ei
import mult_inputs as mi

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 127, 129]
_CACHE = {}


@pytest.fixture(scope="module")
def m():
    import msm_blst_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible")
    return m


def first_diff(got, want, sz):
    for i in range(len(want) // sz):
        if got[i * sz:(i + 1) * sz] != want[i * sz:(i + 1) * sz]:
            return i
    return None


def assert_points(got, want, group, names=None):
    assert len(got) == len(want)
    i = first_diff(got, want, ei.AFF[group])
    assert i is None, f"first differing point: {i}" + (f" ({names[i]})" if names else "")


def sized_case(group):
    """129 fixed points with SplitMix64 scalars and what smul gives (computed once, never modified)"""
    if ("sized", group) not in _CACHE:
        n = max(SIZES)
        pts, ks = ei.fixed_points(group, n), mi.gen_scalars(n, 11)
        _CACHE[("sized", group)] = (mi.points_bytes(group, pts), mi.scalar_bytes(ks),
                                    b"".join(ei.affine_bytes(group, mi.smul(group, p, k)) for p, k in zip(pts, ks)))
    return _CACHE[("sized", group)]


def bulk(golden, group):
    return [c for c in golden("points_mult.json")["bulk"] if c["group"] == group][0]


@pytest.mark.parametrize("group", [1, 2])
def test_sizes(m, golden, group):
    pts, sc, want = sized_case(group)
    A = ei.AFF[group]
    for n in SIZES:
        assert_points(m.ps_mult(group, pts[:n * A], sc[:n * 32], n), want[:n * A], group)
    c = bulk(golden, group)
    n = c["n"]
    got = m.ps_mult(group, m.fixed_points(group, n), m.gen_scalars(n, c["seed"]), n, nbits=c["nbits"])
    assert ei.fnv(got) == c["fnv"]


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("nbits", [255, 256])
def test_special_batch(m, golden, group, nbits):
    names, pts, ks, ing, exp = mi.expected_batch(group, nbits)
    n, A = len(ks), ei.AFF[group]
    got = m.ps_mult(group, mi.points_bytes(group, pts), mi.scalar_bytes(ks), n, nbits=nbits)
    assert_points(got, b"".join(exp), group, names)
    # the in-group entries against the reference's recorded values
    c = [c for c in golden("points_mult.json")["special"] if c["group"] == group and c["nbits"] == nbits][0]
    assert c["in_group"] == [i for i in range(n) if ing[i]]
    for i, want in zip(c["in_group"], c["compressed"]):
        assert ei.encode(group, got[i * A:(i + 1) * A], 1).hex() == want, (i, names[i])
    assert ei.fnv(b"".join(got[i * A:(i + 1) * A] for i in c["in_group"])) == c["fnv"]
    # infinity inputs and infinity results are all zero, their neighbours intact
    for i in range(n):
        if pts[i] is None or ks[i] == 0:
            assert got[i * A:(i + 1) * A] == bytes(A), (i, names[i])
    zero = [i for i in range(n) if not any(got[i * A:(i + 1) * A])]
    assert any(0 < i < n - 1 and any(got[(i - 1) * A:i * A]) and any(got[(i + 1) * A:(i + 2) * A]) for i in zero)
    assert any(names[i].startswith("order") and names[i].endswith("*q") for i in zero)


@pytest.mark.parametrize("group", [1, 2])
def test_narrow_scalars(m, group):
    n, A = 9, ei.AFF[group]
    pts = ei.fixed_points(group, n)
    pb = mi.points_bytes(group, pts)
    full = mi.gen_scalars(n, 5)
    for nbits in (1, 4, 5, 64, 129, 176):
        ks = [k & ((1 << nbits) - 1) for k in full]
        ks[0], ks[1] = (1 << nbits) - 1, 1 << (nbits - 1)
        want = b"".join(ei.affine_bytes(group, mi.smul(group, p, k)) for p, k in zip(pts, ks))
        nb = (nbits + 7) // 8
        tight = mi.scalar_bytes(ks, nb, nb)
        assert len(tight) == n * nb
        assert_points(m.ps_mult(group, pb, tight, n, nbits=nbits, stride=nb), want, group)
        assert_points(m.ps_mult(group, pb, mi.scalar_bytes(ks), n, nbits=nbits, stride=32), want, group)
        if nbits == 129:  # a stride wider than a scalar, from host memory (packed while staged) and from device memory
            import torch
            wide = mi.scalar_bytes(ks, 48)
            assert_points(m.ps_mult(group, pb, wide, n, nbits=nbits, stride=48), want, group)
            d = torch.frombuffer(bytearray(pb + wide), dtype=torch.uint8).to("cuda:0")
            torch.cuda.synchronize()
            assert_points(m.ps_mult(group, d.data_ptr(), d.data_ptr() + len(pb), n, nbits=nbits, stride=48,
                                    src_on_device=True), want, group)
    # stray bits above nbits in the last byte (and beyond it) are ignored
    nbits = 61
    ks = [k & ((1 << nbits) - 1) for k in full]
    want = b"".join(ei.affine_bytes(group, mi.smul(group, p, k)) for p, k in zip(pts, ks))
    stray = mi.scalar_bytes([k | (0x7 << nbits) | (0xabcd << 64) for k in ks], 11)
    assert_points(m.ps_mult(group, pb, stray, n, nbits=nbits, stride=11), want, group)
    # nbits = 0: every output is infinity
    assert m.ps_mult(group, pb, mi.scalar_bytes(full), n, nbits=0) == bytes(n * A)
    assert m.ps_mult(group, pb, b"", n, nbits=0, stride=0) == bytes(n * A)


@pytest.mark.parametrize("group", [1, 2])
def test_one_point(m, golden, group):
    A = ei.AFF[group]
    n = 70
    ks = mi.gen_scalars(n, 9)
    q, t = mi.small_order_points(group)[0]
    ks[:6] = [0, 1, q, q - 1, q + 1, (1 << 255) - 1]
    sc = mi.scalar_bytes(ks)
    for pt in (ei.GEN[group], t):
        one = ei.affine_bytes(group, pt)
        got = m.ps_mult(group, one, sc, n, one_point=True)
        assert_points(got, m.ps_mult(group, one * n, sc, n), group)
        for i in (0, 1, 2, 3, 4, 5, 6, n - 1):
            assert got[i * A:(i + 1) * A] == ei.affine_bytes(group, mi.smul(group, pt, ks[i])), i
    c = bulk(golden, group)
    got = m.ps_mult(group, ei.affine_bytes(group, ei.GEN[group]), m.gen_scalars(c["n"], c["seed"]), c["n"],
                    one_point=True)
    assert ei.fnv(got) == c["fnv_one_point"]


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("one_point", [False, True])
def test_chunks(m, group, one_point, monkeypatch):
    n = 257
    names, pts, ks, ing, exp = mi.expected_batch(group, 255)
    sc = mi.scalar_bytes(ks) + bytes(m.gen_scalars(n - len(ks), 13))
    pb = ei.affine_bytes(group, ei.GEN[group]) if one_point else \
        mi.points_bytes(group, pts) + bytes(m.fixed_points(group, n - len(ks)))
    whole = m.ps_mult(group, pb, sc, n, one_point=one_point)
    monkeypatch.setenv("MSM_POINTS_MULT_CHUNK", "96")  # two full chunks and a ragged tail
    chunked = m.ps_mult(group, pb, sc, n, one_point=one_point)
    assert_points(chunked, whole, group)
    if not one_point:
        assert whole[:len(ks) * ei.AFF[group]] == b"".join(exp)


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("path", ["d2d", "h2d", "d2h"])
def test_device_memory_on_a_stream(m, group, path, monkeypatch):
    """Sources written by torch copies queued on a non-default stream just before
    the call (behind a device-side delay): the call must order itself after them,
    in every one of its chunks (four here)."""
    import torch
    monkeypatch.setenv("MSM_POINTS_MULT_CHUNK", "40")
    pts, sc, want = sized_case(group)
    n = max(SIZES)
    dev = torch.device("cuda:0")
    src = pts + sc  # points, then scalars, in one buffer
    pinned = torch.frombuffer(bytearray(src), dtype=torch.uint8).pin_memory()
    d_ref = torch.frombuffer(bytearray(src), dtype=torch.uint8).to(dev)
    d_src = torch.zeros(len(src), dtype=torch.uint8, device=dev)
    h_src = torch.zeros(len(src), dtype=torch.uint8).pin_memory()
    d_dst = torch.zeros(len(want), dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        torch.cuda._sleep(10_000_000)
        if path == "h2d":
            h_src.copy_(d_ref, non_blocking=True)
            hp = (ctypes.c_uint8 * len(pts)).from_address(h_src.data_ptr())
            hs = (ctypes.c_uint8 * len(sc)).from_address(h_src.data_ptr() + len(pts))
            got = m.ps_mult(group, hp, hs, n, dst=d_dst.data_ptr(), stream=st.cuda_stream)
        else:
            d_src.copy_(pinned, non_blocking=True)
            got = m.ps_mult(group, d_src.data_ptr(), d_src.data_ptr() + len(pts), n, src_on_device=True,
                            dst=d_dst.data_ptr() if path == "d2d" else None, stream=st.cuda_stream)
    st.synchronize()
    if got is None:
        got = bytes(d_dst.cpu().numpy())
    assert_points(got, want, group)


def test_threads_and_engine_cache(m):
    pts, sc, want = sized_case(1)
    n = 64
    out = [None, None]
    m.release_engine_cache()

    def work(t):
        out[t] = m.ps_mult(1, pts[t * n * 96:(t + 1) * n * 96], sc[t * n * 32:(t + 1) * n * 32], n)

    ts = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for t in range(2):
        assert out[t] is not None
        assert_points(out[t], want[t * n * 96:(t + 1) * n * 96], 1)
    live, idle, idle_bytes = m.engine_cache_stats()
    assert 1 <= idle <= 2 and live >= idle and idle_bytes > 0  # the engines, back in the pool
    m.release_engine_cache()
    assert m.engine_cache_stats()[1] == 0


@pytest.mark.parametrize("group", [1, 2])
def test_srs_end_to_end(m, group):
    """[tau^i]G by ps_mult(one_point) into device memory, a context on it, and one
    MSM with scalars s: the sum must be [sum s_i tau^i mod r]G."""
    import torch
    n, A = 1024, ei.AFF[group]
    tau = mi.gen_scalars(1, 21)[0]
    pw = [pow(tau, i, mi.R) for i in range(n)]
    gen = ei.affine_bytes(group, ei.GEN[group])
    d_srs = torch.zeros(n * A, dtype=torch.uint8, device="cuda:0")
    assert m.ps_mult(group, gen, mi.scalar_bytes(pw), n, one_point=True, dst=d_srs.data_ptr()) is None
    torch.cuda.synchronize()
    ctx = m.MSMContext(group, 0, 10)
    ctx.set_points(d_srs.data_ptr(), n, on_device=True)
    s = mi.gen_scalars(n, 3)
    assert mi.scalar_bytes(s) == bytes(m.gen_scalars(n, 3))
    got = m.compress(group, ctx.mult(m.gen_scalars(n, 3)))
    ctx.close()
    k = sum(a * b for a, b in zip(s, pw)) % mi.R
    want = m.ps_mult(group, gen, mi.scalar_bytes([k]), 1, one_point=True)
    assert got == ei.encode(group, want, 1)
    assert want == ei.affine_bytes(group, mi.smul(group, ei.GEN[group], k))
