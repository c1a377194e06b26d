"""GPU parity of the segmented sums and MSMs (msm_points_msm_segments /
ps_msm_segments, ps_sum_segments; csrc/point_segments.hip) on an MI355X.

Oracle: tests/seg_inputs.py, mult_inputs.smul per point and the Jacobian addition
of enc_inputs.py in plain Python integers (the only oracle for points outside the
subgroup); tests/golden/points_segments.json holds the reference's own sums of the
in-group segments of one batch.  Every comparison is byte for byte.  Batches stay
at 400 points or fewer per group and use 64-bit scalars wherever 255 bits are not
the point: the oracle is the cost.
"""
import ctypes
import threading

import pytest

import enc_inputs as ei
import mult_inputs as mi
import seg_inputs as si

pytestmark = pytest.mark.gpu

_CACHE = {}


@pytest.fixture(scope="module")
def m():
    import msm_blst_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible")
    return m


@pytest.fixture(autouse=True)
def _no_overrides(monkeypatch):
    monkeypatch.delenv("MSM_POINTS_SEGMENTS_PIECE", raising=False)
    monkeypatch.delenv("MSM_POINTS_SEGMENTS_CHUNK", raising=False)


def assert_points(got, want, group, what=""):
    assert len(got) == len(want)
    A = ei.AFF[group]
    bad = [j for j in range(len(want) // A) if got[j * A:(j + 1) * A] != want[j * A:(j + 1) * A]]
    assert not bad, f"differing segments {bad[:8]} {what}"


def base_case(group):
    """206 fixed points with 64-bit scalars, the sums of the layouts the tests use (computed once, never modified)"""
    if group not in _CACHE:
        pts, ks = si.batch(group, 206, 17, 64)
        _CACHE[group] = {"pts": pts, "ks": ks, "pb": mi.points_bytes(group, pts), "sb": mi.scalar_bytes(ks, 8), "exp": {}}
    return _CACHE[group]


def want(group, offsets, sums=False):
    c = base_case(group)
    key = (tuple(offsets), sums)
    if key not in c["exp"]:
        c["exp"][key] = si.expected(group, c["pts"], None if sums else c["ks"], list(offsets))
    return c["exp"][key]


def run(m, group, offsets, sums=False, **kw):
    c = base_case(group)
    if sums:
        return m.ps_sum_segments(group, c["pb"], offsets, **kw)
    return m.ps_msm_segments(group, c["pb"], c["sb"], offsets, nbits=64, stride=8, **kw)


@pytest.mark.parametrize("group", [1, 2])
def test_one_point_segments_equal_ps_mult(m, group):
    n = 130
    pts, sc = bytes(m.fixed_points(group, n)), bytes(m.gen_scalars(n, 23))
    got = m.ps_msm_segments(group, pts, sc, range(n + 1))
    assert_points(got, m.ps_mult(group, pts, sc, n), group)
    assert m.ps_sum_segments(group, pts, range(n + 1)) == pts


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("sums", [False, True])
def test_one_segment_of_200(m, group, sums, monkeypatch):
    o = [0, 200]
    assert_points(run(m, group, o, sums), want(group, o, sums), group, "default piece")
    monkeypatch.setenv("MSM_POINTS_SEGMENTS_PIECE", "8")  # 25 partials: a merge tree of 5 levels
    assert len(m.segments_plan(o, 8)) == 25
    assert_points(run(m, group, o, sums), want(group, o, sums), group, "piece 8")


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("sums", [False, True])
def test_piece_edges(m, group, sums, monkeypatch):
    monkeypatch.setenv("MSM_POINTS_SEGMENTS_PIECE", "8")
    o = si.offsets_of(si.EDGE_LENGTHS)
    got = run(m, group, o, sums)
    assert_points(got, want(group, o, sums), group)
    A = ei.AFF[group]
    for j, n in enumerate(si.EDGE_LENGTHS):
        assert any(got[j * A:(j + 1) * A]) == (n > 0), j  # empty segments all zero, their neighbours intact


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("sums", [False, True])
def test_chunk_carry(m, group, sums, monkeypatch):
    """chunks of 48 points: a segment over three chunks (0 .. 129), one that ends on the
    boundary 144, one that ends a point before 192, one that starts there, an empty one"""
    o = si.offsets_of([129, 15, 47, 10, 0, 5])
    assert o[1:4] == [129, 144, 191] and o[-1] == 206
    whole = run(m, group, o, sums)
    monkeypatch.setenv("MSM_POINTS_SEGMENTS_CHUNK", "48")
    chunked = run(m, group, o, sums)
    assert_points(chunked, whole, group, "chunked against whole")
    assert_points(chunked, want(group, o, sums), group)
    monkeypatch.setenv("MSM_POINTS_SEGMENTS_PIECE", "5")
    assert_points(run(m, group, o, sums), whole, group, "chunk 48, piece 5")
    # more segments than a chunk holds: the chunk is cut by its segments too
    monkeypatch.setenv("MSM_POINTS_SEGMENTS_CHUNK", "3")
    o2 = si.offsets_of([0] * 7 + [2, 0, 0, 0, 0, 7] + [0] * 4)
    assert_points(run(m, group, o2, sums), want(group, o2, sums), group, "chunk 3")


def special_case(group):
    """branches inside a piece and in the merge, 255-bit scalars; computed once"""
    key = ("special", group)
    if key not in _CACHE:
        f = ei.fixed_points(group, 12)
        r = mi.gen_scalars(12, 29)
        P, Q = f[0], f[1]
        nP, nQ = si.neg(group, P), si.neg(group, Q)
        segs = [  # (points, scalars)
            ([P, P], [r[0], r[0]]),
            ([P, nP], [r[1], r[1]]),
            ([P, nP, Q], [r[2], r[2], r[3]]),
            ([None, P], [r[4], r[5]]),
            ([None, None], [r[4], r[5]]),
            ([P, Q, f[2]], [0, 0, 0]),
            ([P, P], [r[6], mi.R - r[6]]),
            # the merge, at a piece of 4: the second piece repeats the first; negates it; the first sums to infinity
            (f[2:6] + f[2:6], r[0:4] + r[0:4]),
            (f[2:6] + [si.neg(group, p) for p in f[2:6]], r[0:4] + r[0:4]),
            ([P, nP, Q, nQ] + f[6:10], [r[7], r[7], r[8], r[8]] + r[8:12]),
        ]
        pts = [p for s in segs for p in s[0]]
        ks = [k for s in segs for k in s[1]]
        o = si.offsets_of([len(s[0]) for s in segs])
        _CACHE[key] = (pts, ks, o, si.expected(group, pts, ks, o), si.expected(group, pts, None, o))
    return _CACHE[key]


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("piece", [4, 64])
def test_exceptional_branches(m, group, piece, monkeypatch):
    monkeypatch.setenv("MSM_POINTS_SEGMENTS_PIECE", str(piece))
    pts, ks, o, exp, exp_sum = special_case(group)
    A = ei.AFF[group]
    got = m.ps_msm_segments(group, mi.points_bytes(group, pts), mi.scalar_bytes(ks), o)
    assert_points(got, exp, group)
    for j in (1, 4, 5, 6, 8):  # P - P, inf + inf, zero scalars, [k]P + [r - k]P, a piece and its negation
        assert got[j * A:(j + 1) * A] == bytes(A), j
    assert got[0:A] == ei.affine_bytes(group, mi.smul(group, pts[0], 2 * ks[0] % mi.R))
    got = m.ps_sum_segments(group, mi.points_bytes(group, pts), o)
    assert_points(got, exp_sum, group, "sums")
    assert got[0:A] == ei.affine_bytes(group, ei._affine_dbl(group, pts[0]))


@pytest.mark.parametrize("group", [1, 2])
def test_small_order_points(m, group, monkeypatch):
    """points outside the subgroup between in-group points: the sums are exact"""
    key = ("small", group)
    if key not in _CACHE:
        f = ei.fixed_points(group, 10)
        ks = [k & ((1 << 64) - 1) for k in mi.gen_scalars(20, 37)]
        (q1, t1), (q2, t2) = mi.small_order_points(group)
        pts = [f[0], t1, f[1], t1, si.neg(group, t1), t2, t2, f[2], t1, t2, f[3], f[4], t1, t1, t1, f[5], t2, f[6], f[7], t2]
        ks[3], ks[4] = q1 - 1, q1 + 1
        o = si.offsets_of([3, 2, 4, 9, 2])
        _CACHE[key] = (pts, ks, o, si.expected(group, pts, ks, o), si.expected(group, pts, None, o))
    pts, ks, o, exp, exp_sum = _CACHE[key]
    pb, sb = mi.points_bytes(group, pts), mi.scalar_bytes(ks, 8)
    for piece in ("4", "64"):
        monkeypatch.setenv("MSM_POINTS_SEGMENTS_PIECE", piece)
        assert_points(m.ps_msm_segments(group, pb, sb, o, nbits=64, stride=8), exp, group, f"piece {piece}")
        assert_points(m.ps_sum_segments(group, pb, o), exp_sum, group, f"sums, piece {piece}")


@pytest.mark.parametrize("group", [1, 2])
def test_nbits_and_stride(m, group):
    n, A = 9, ei.AFF[group]
    o = [0, 3, 3, 8, 9]
    pts = ei.fixed_points(group, n)
    pb = mi.points_bytes(group, pts)
    full = mi.gen_scalars(n, 5) + []
    full[0] = (1 << 256) - 1
    for nbits in (1, 64, 255, 256):
        ks = [k & ((1 << nbits) - 1) for k in full]
        exp = si.expected(group, pts, ks, o)
        nb = (nbits + 7) // 8
        assert_points(m.ps_msm_segments(group, pb, mi.scalar_bytes(ks, nb, nb), o, nbits=nbits, stride=nb), exp, group,
                      f"nbits {nbits}, tight")
        # stray bits above nbits are masked
        assert_points(m.ps_msm_segments(group, pb, mi.scalar_bytes(full), o, nbits=nbits, stride=32), exp, group,
                      f"nbits {nbits}, stride 32")
    # a stride of 9 bytes at 64 bits, the last scalar ending the buffer; from host and from device memory
    ks = [k & ((1 << 64) - 1) for k in full]
    exp = si.expected(group, pts, ks, o)
    sb = mi.scalar_bytes(ks, 9, 8)
    assert len(sb) == 8 * 9 + 8
    assert_points(m.ps_msm_segments(group, pb, sb, o, nbits=64, stride=9), exp, group, "stride 9")
    import torch
    d = torch.frombuffer(bytearray(pb + sb), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    assert_points(m.ps_msm_segments(group, d.data_ptr(), d.data_ptr() + len(pb), o, nbits=64, stride=9,
                                    src_on_device=True), exp, group, "stride 9, device")
    # nbits = 0: every result is infinity
    assert m.ps_msm_segments(group, pb, mi.scalar_bytes(full), o, nbits=0) == bytes(4 * A)
    assert m.ps_msm_segments(group, pb, b"", o, nbits=0, stride=0) == bytes(4 * A)


@pytest.mark.parametrize("group", [1, 2])
def test_plain_sum_against_ps_add(m, group):
    c = base_case(group)
    n = 150
    got = m.ps_sum_segments(group, c["pb"], [0, n])
    assert got == m.to_affine(group, m.ps_add(group, c["pb"][:n * ei.AFF[group]], n))
    # every segment empty: all infinity, no points read
    assert m.ps_sum_segments(group, c["pb"], [4, 4, 4]) == bytes(2 * ei.AFF[group])


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("sums", [False, True])
def test_first_offset_above_zero(m, group, sums):
    o = si.offsets_of(si.EDGE_LENGTHS, first=5)
    assert_points(run(m, group, o, sums), want(group, o, sums), group)


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("path", ["d2d", "h2d", "d2h"])
def test_device_memory_on_a_stream(m, group, path, monkeypatch):
    """Sources written by torch copies queued on a non-default stream just before
    the call (behind a device-side delay): the call must order itself after them,
    in every one of its chunks (five here)."""
    import torch
    monkeypatch.setenv("MSM_POINTS_SEGMENTS_CHUNK", "48")
    c = base_case(group)
    o = si.offsets_of([129, 15, 47, 10, 0, 5])
    exp = want(group, o)
    pts, sc = c["pb"], c["sb"]
    dev = torch.device("cuda:0")
    src = pts + sc  # points, then scalars, in one buffer
    pinned = torch.frombuffer(bytearray(src), dtype=torch.uint8).pin_memory()
    d_ref = torch.frombuffer(bytearray(src), dtype=torch.uint8).to(dev)
    d_src = torch.zeros(len(src), dtype=torch.uint8, device=dev)
    h_src = torch.zeros(len(src), dtype=torch.uint8).pin_memory()
    d_dst = torch.zeros(len(exp), dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        torch.cuda._sleep(10_000_000)
        if path == "h2d":
            h_src.copy_(d_ref, non_blocking=True)
            hp = (ctypes.c_uint8 * len(pts)).from_address(h_src.data_ptr())
            hs = (ctypes.c_uint8 * len(sc)).from_address(h_src.data_ptr() + len(pts))
            got = m.ps_msm_segments(group, hp, hs, o, nbits=64, stride=8, dst=d_dst.data_ptr(), stream=st.cuda_stream)
        else:
            d_src.copy_(pinned, non_blocking=True)
            got = m.ps_msm_segments(group, d_src.data_ptr(), d_src.data_ptr() + len(pts), o, nbits=64, stride=8,
                                    src_on_device=True, dst=d_dst.data_ptr() if path == "d2d" else None,
                                    stream=st.cuda_stream)
    st.synchronize()
    if got is None:
        got = bytes(d_dst.cpu().numpy())
    assert_points(got, exp, group)
    if path == "d2d":  # plain sums, device to device
        d_dst.zero_()
        assert m.ps_sum_segments(group, d_src.data_ptr(), o, src_on_device=True, dst=d_dst.data_ptr(),
                                 stream=st.cuda_stream) is None
        st.synchronize()
        assert_points(bytes(d_dst.cpu().numpy()), want(group, o, True), group, "sums")


def test_threads_and_engine_cache(m):
    layouts = [si.offsets_of(si.EDGE_LENGTHS), [0, 200]]
    out = [None, None]
    m.release_engine_cache()
    before = m.engine_cache_stats()

    def work(t):
        out[t] = run(m, 1, layouts[t], sums=(t == 1))

    ts = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for t in range(2):
        assert out[t] is not None
        assert_points(out[t], want(1, layouts[t], t == 1), 1, f"thread {t}")
    live, idle, idle_bytes = m.engine_cache_stats()
    assert 1 <= idle - before[1] <= 2 and live >= idle and idle_bytes > before[2]  # the engines, back in the pool
    m.release_engine_cache()
    assert m.engine_cache_stats()[1] == 0


@pytest.mark.parametrize("group", [1, 2])
def test_reference_segments(m, golden, group):
    """the reference's recorded sums of the in-group segments of the golden batch"""
    c = [c for c in golden("points_segments.json")["segments"] if c["group"] == group][0]
    pts, ks, o, ing = si.golden_batch(group)
    A = ei.AFF[group]
    got = m.ps_msm_segments(group, mi.points_bytes(group, pts), mi.scalar_bytes(ks), o, nbits=c["nbits"])
    for j, hexs in zip(c["in_group"], c["compressed"]):
        assert ei.encode(group, got[j * A:(j + 1) * A], 1).hex() == hexs, j
    assert ei.fnv(b"".join(got[j * A:(j + 1) * A] for j in c["in_group"])) == c["fnv"]
    assert_points(got, si.expected(group, pts, ks, o), group)
