"""GPU parity of the bulk hash-to-curve (msm_points_hash, msm_hash_to_field,
msm_points_map; csrc/hash_to_curve.hip) on an MI355X.

Oracle: tests/golden/hash_to_curve.json, written from the reference's own
blst_hash_to_g{1,2} / blst_encode_to_g{1,2} / blst_map_to_g{1,2}: per point the
compressed encoding and an FNV of the affine bytes.  No curve arithmetic runs in
Python here: affine outputs are compared through their FNV and, compressed by
ps_encode on the GPU, byte for byte.
"""
import ctypes
import threading

import pytest

import h2c_inputs as h

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 127, 129, 1000]


@pytest.fixture(scope="module")
def m():
    import msm_blst_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible")
    return m


@pytest.fixture(scope="module")
def fx(golden):
    return golden("hash_to_curve.json")["groups"]


MSGS = h.messages()


def check_points(m, group, got, want, what=""):
    """got: affine bytes; want: fixture entries.  Reports the first differing index."""
    A, n = h.AFF[group], len(want)
    assert len(got) == n * A, (what, len(got), n * A)
    bad = [i for i in range(n) if h.fnv(got[i * A:(i + 1) * A]) != want[i]["fnv"]]
    assert not bad, f"{what}: first differing point {bad[0]} ({len(bad)} of {n} differ)"
    enc = m.ps_encode(group, got, n)
    E = 48 * group
    bad = [i for i in range(n) if enc[i * E:(i + 1) * E].hex() != want[i]["c"]]
    assert not bad, f"{what}: first differing compressed point {bad[0]}"


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("encode", [False, True])
def test_mixed_batch(m, fx, group, encode):
    want = fx[str(group)]["mixed"]["encode" if encode else "hash"]
    got = m.ps_hash_to_curve(group, MSGS, dst_tag=h.DST[group], encode=encode)
    check_points(m, group, got, want, f"G{group} encode={encode}")


@pytest.mark.parametrize("group", [1, 2])
def test_field_elements(m, fx, group):
    want = bytes.fromhex("".join(fx[str(group)]["fields"]))
    got = m.ps_hash_to_field(group, MSGS[:16], dst_tag=h.DST[group], count=2)
    E = 2 * h.ELEM[group]
    bad = [i for i in range(16) if got[i * E:(i + 1) * E] != want[i * E:(i + 1) * E]]
    assert not bad and len(got) == len(want), f"first differing message {bad[:1]}"
    # count = 1 is a different expansion (len_in_bytes enters the hash), not a prefix
    one = m.ps_hash_to_field(group, MSGS[:16], dst_tag=h.DST[group], count=1)
    assert one == h.field_bytes(group, [e for k in range(16) for e in h.hash_to_field(group, MSGS[k], h.DST[group], 1)])


@pytest.mark.parametrize("group", [1, 2])
def test_map_special_u(m, fx, group):
    us, pairs = h.map_cases(group)
    u1 = h.field_bytes(group, us)
    check_points(m, group, m.ps_map_to_curve(group, u1, len(us), count=1), fx[str(group)]["map1"], "count 1")
    u2 = h.field_bytes(group, [e for p in pairs for e in p])
    got = m.ps_map_to_curve(group, u2, len(pairs), count=2)
    check_points(m, group, got, fx[str(group)]["map2"], "count 2")
    A = h.AFF[group]
    assert any(got[i * A:(i + 1) * A] == bytes(A) for i in range(len(pairs))), "u == -v gives infinity"


@pytest.mark.parametrize("group", [1, 2])
def test_sizes(m, fx, group):
    want = fx[str(group)]["mixed"]["hash"]
    for n in SIZES:
        got = m.ps_hash_to_curve(group, [MSGS[i % h.MIXED_N] for i in range(n)], dst_tag=h.DST[group])
        check_points(m, group, got, [want[i % h.MIXED_N] for i in range(n)], f"n={n}")


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("name", list(h.CASES))
def test_dst_aug_and_fixed_length(m, fx, group, name):
    msgs, dst, aug, fixed = h.case(group, name)
    kw = dict(dst_tag=dst)
    if aug:
        kw.update(aug=b"".join(aug), aug_len=len(aug[0]))
    if fixed:
        got = m.ps_hash_to_curve(group, b"".join(msgs), msg_len=32, **kw)
    else:
        got = m.ps_hash_to_curve(group, msgs, **kw)
    check_points(m, group, got, fx[str(group)]["cases"][name], name)


@pytest.mark.parametrize("group", [1, 2])
def test_chunks(m, fx, group, monkeypatch):
    n = 257
    msgs = [MSGS[i % h.MIXED_N] for i in range(n)]
    aug = bytes((i * 5 + 1) & 0xff for i in range(n * 3))
    whole = m.ps_hash_to_curve(group, msgs, dst_tag=h.DST[group], aug=aug, aug_len=3)
    plain = m.ps_hash_to_curve(group, msgs, dst_tag=h.DST[group])
    fields = m.ps_hash_to_field(group, msgs, dst_tag=h.DST[group])
    monkeypatch.setenv("MSM_H2C_CHUNK", "96")  # two full chunks and a ragged tail
    assert m.ps_hash_to_curve(group, msgs, dst_tag=h.DST[group], aug=aug, aug_len=3) == whole
    chunked = m.ps_hash_to_curve(group, msgs, dst_tag=h.DST[group])
    assert chunked == plain
    assert m.ps_hash_to_field(group, msgs, dst_tag=h.DST[group]) == fields
    assert m.ps_map_to_curve(group, fields, n, count=2) == plain
    want = fx[str(group)]["mixed"]["hash"]
    check_points(m, group, chunked, [want[i % h.MIXED_N] for i in range(n)], "chunked")
    assert whole != plain


@pytest.mark.parametrize("group", [1, 2])
def test_round_trip_in_group(m, group):
    """1000 distinct messages: every point decodes with the subgroup check (a wrong
    cofactor clearing leaves the subgroup), encode / decode is the identity, no two agree."""
    n = 1000
    pts = m.ps_hash_to_curve(group, h.distinct_messages(n), dst_tag=h.DST[group])
    enc = m.ps_encode(group, pts, n)
    back, st = m.ps_decode(group, enc, n, check_group=True)
    assert st == bytes(n), [i for i in range(n) if st[i]][:5]
    assert back == pts
    E = 48 * group
    assert len({enc[i * E:(i + 1) * E] for i in range(n)}) == n
    assert bytes(h.AFF[group]) not in {pts[i * h.AFF[group]:(i + 1) * h.AFF[group]] for i in range(n)}


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("path", ["d2d", "h2d", "d2h"])
def test_device_memory_on_a_stream(m, group, path):
    """Messages written by a torch copy queued on a non-default stream just before
    the call (behind a device-side delay): the call must order itself after it.  A
    device dst feeds ps_encode(src_on_device=True) on the same stream."""
    import torch
    n = 1000
    msgs = b"".join(h._bytes(32, i) for i in range(n))
    want = m.ps_hash_to_curve(group, msgs, msg_len=32, dst_tag=h.DST[group])
    dev = torch.device("cuda:0")
    pinned = torch.frombuffer(bytearray(msgs), dtype=torch.uint8).pin_memory()
    d_msgs = torch.frombuffer(bytearray(msgs), dtype=torch.uint8).to(dev)
    d_src = torch.zeros(len(msgs), dtype=torch.uint8, device=dev)
    h_src = torch.zeros(len(msgs), dtype=torch.uint8).pin_memory()
    d_dst = torch.zeros(len(want), dtype=torch.uint8, device=dev)
    d_enc = torch.zeros(n * 48 * group, dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    got = None
    with torch.cuda.stream(st):
        torch.cuda._sleep(10_000_000)
        if path == "h2d":
            h_src.copy_(d_msgs, non_blocking=True)
            src = (ctypes.c_uint8 * len(msgs)).from_address(h_src.data_ptr())
            m.ps_hash_to_curve(group, src, msg_len=32, dst_tag=h.DST[group], dst=d_dst.data_ptr(), stream=st.cuda_stream)
        else:
            d_src.copy_(pinned, non_blocking=True)
            if path == "d2d":
                m.ps_hash_to_curve(group, d_src.data_ptr(), msg_len=32, n=n, dst_tag=h.DST[group], src_on_device=True,
                                   dst=d_dst.data_ptr(), stream=st.cuda_stream)
            else:
                got = m.ps_hash_to_curve(group, d_src.data_ptr(), offsets=range(0, 32 * n + 1, 32), dst_tag=h.DST[group],
                                         src_on_device=True, stream=st.cuda_stream)
        if got is None:
            m.ps_encode(group, d_dst.data_ptr(), n, src_on_device=True, dst=d_enc.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    if got is None:
        got = bytes(d_dst.cpu().numpy())
        assert bytes(d_enc.cpu().numpy()) == m.ps_encode(group, want, n)
    assert got == want


def test_threads_and_engine_cache(m, fx):
    out = [None, None]
    m.release_engine_cache()

    def work(t):
        out[t] = m.ps_hash_to_curve(1, MSGS, dst_tag=h.DST[1], encode=bool(t))

    ts = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for t in range(2):
        assert out[t] is not None
        check_points(m, 1, out[t], fx["1"]["mixed"]["encode" if t else "hash"], f"thread {t}")
    live, idle, idle_bytes = m.engine_cache_stats()
    assert idle >= 1 and live >= idle and idle_bytes > 0  # the engines are back in the pool
    m.release_engine_cache()
    assert m.engine_cache_stats()[1] == 0
