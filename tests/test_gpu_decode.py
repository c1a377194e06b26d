"""GPU parity of the bulk point decoding (msm_points_decode,
msm_ctx_set_points_encoded; csrc/decode.hip) on an MI355X.

Oracles: tests/enc_inputs.py encodes affine points in plain Python integers, so
the expected output of a valid entry is the affine input itself, byte for byte;
tests/golden/decode.json holds the reference's own statuses, subgroup Booleans
and output hashes on the mixed batch of good and bad entries.
"""
import ctypes
import threading

import pytest

import enc_inputs as ei

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 127, 129, 1000]
NMAX = 1024

_AFF, _ENC = {}, {}


@pytest.fixture(scope="module")
def m():
    import msm_blst_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible")
    return m


def affine(m, group, n):
    """the first n fixed points (computed once per group, never modified)"""
    if group not in _AFF:
        _AFF[group] = bytes(m.fixed_points(group, NMAX))
        assert _AFF[group][:8 * ei.AFF[group]] == ei.fixed_affine(group, 8)
    return _AFF[group][:n * ei.AFF[group]]


def encoded(m, group, n, compressed):
    key = (group, compressed)
    if key not in _ENC:
        _ENC[key] = ei.encode(group, affine(m, group, NMAX), NMAX, compressed)
    return _ENC[key][:n * ei.ENC[group] * (1 if compressed else 2)]


def first_diff(got, want, sz):
    for i in range(len(want) // sz):
        if got[i * sz:(i + 1) * sz] != want[i * sz:(i + 1) * sz]:
            return i
    return None


def assert_points(got, want, group):
    assert len(got) == len(want)
    assert got == want, f"first differing point: {first_diff(got, want, ei.AFF[group])}"


def case(golden, group, serialized):
    name = "serialized" if serialized else "compressed"
    return [c for c in golden("decode.json")["cases"] if c["group"] == group and c["encoding"] == name][0]


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("compressed", [True, False])
@pytest.mark.parametrize("check_group", [False, True])
def test_round_trip(m, group, compressed, check_group):
    L = m.lib()
    for n in SIZES:
        want = affine(m, group, n)
        enc = encoded(m, group, n, compressed)
        got, st = m.ps_decode(group, enc, n, compressed=compressed, check_group=check_group)
        assert st == bytes(n), (n, list(st))
        assert_points(got, want, group)
        # nbad, with and without a status array
        dst = (ctypes.c_uint8 * len(want))()
        nbad = ctypes.c_size_t(99)
        src = (ctypes.c_uint8 * len(enc)).from_buffer_copy(enc)
        assert L.msm_points_decode(group, 0, dst, None, ctypes.byref(nbad), src, n, 0 if compressed else 1,
                                   int(check_group), 0, 0, None) == 0, L.msm_last_error()
        assert nbad.value == 0 and bytes(dst) == want


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("serialized", [False, True])
def test_mixed_batch(m, golden, group, serialized):
    c = case(golden, group, serialized)
    data, names = ei.mixed_batch(group, serialized)
    n, A = ei.MIXED_N, ei.AFF[group]
    for check_group in (False, True):
        want_st = [3 if (check_group and g is False) else s for s, g in zip(c["status"], c["in_group"])]
        got, st = m.ps_decode(group, data, n, compressed=not serialized, check_group=check_group)
        bad = [(i, names[i], st[i], want_st[i]) for i in range(n) if st[i] != want_st[i]]
        assert not bad, f"(index, class, status, expected): {bad}"
        assert ei.fnv(got) == (c["fnv_group"] if check_group else c["fnv"])
        for i in range(n):
            if st[i]:
                assert got[i * A:(i + 1) * A] == bytes(A), (i, names[i])
        # failed entries all zero, their neighbours intact: the whole output, entry by entry
        exp_st, exp_out = ei.expected(group, serialized, check_group)
        assert exp_st == want_st
        assert_points(got, exp_out, group)
        assert any(st[i] and not st[i + 1] and any(got[(i + 1) * A:(i + 2) * A]) for i in range(n - 1))
        # nbad
        nbad = ctypes.c_size_t(0)
        dst = (ctypes.c_uint8 * (n * A))()
        src = (ctypes.c_uint8 * len(data)).from_buffer_copy(data)
        assert m.lib().msm_points_decode(group, 0, dst, None, ctypes.byref(nbad), src, n, int(serialized),
                                         int(check_group), 0, 0, None) == 0
        assert nbad.value == sum(1 for s in want_st if s) and bytes(dst) == exp_out


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("serialized", [False, True])
def test_chunks(m, group, serialized, monkeypatch):
    n = 257
    data, _ = ei.mixed_batch(group, serialized)
    data += encoded(m, group, n - ei.MIXED_N, not serialized)
    whole = m.ps_decode(group, data, n, compressed=not serialized)
    monkeypatch.setenv("MSM_DECODE_CHUNK", "96")  # two full chunks and a ragged tail
    chunked = m.ps_decode(group, data, n, compressed=not serialized)
    assert chunked[1] == whole[1]
    assert_points(chunked[0], whole[0], group)
    assert whole[0][ei.MIXED_N * ei.AFF[group]:] == affine(m, group, n - ei.MIXED_N)
    assert any(whole[1]) and not any(whole[1][ei.MIXED_N:])


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("path", ["d2d", "h2d", "d2h"])
def test_device_memory_on_a_stream(m, group, path):
    """Source written by a torch copy queued on a non-default stream just before
    the call (behind a device-side delay): the call must order itself after it."""
    import torch
    n = 1000
    enc, want = encoded(m, group, n, True), affine(m, group, n)
    dev = torch.device("cuda:0")
    pinned = torch.frombuffer(bytearray(enc), dtype=torch.uint8).pin_memory()
    d_enc = torch.frombuffer(bytearray(enc), dtype=torch.uint8).to(dev)
    d_src = torch.zeros(len(enc), dtype=torch.uint8, device=dev)
    h_src = torch.zeros(len(enc), dtype=torch.uint8).pin_memory()
    d_dst = torch.zeros(len(want), dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        torch.cuda._sleep(10_000_000)
        if path == "h2d":
            h_src.copy_(d_enc, non_blocking=True)
            src = (ctypes.c_uint8 * len(enc)).from_address(h_src.data_ptr())
            got, status = m.ps_decode(group, src, n, dst=d_dst.data_ptr(), stream=st.cuda_stream)
        else:
            d_src.copy_(pinned, non_blocking=True)
            if path == "d2d":
                got, status = m.ps_decode(group, d_src.data_ptr(), n, src_on_device=True, dst=d_dst.data_ptr(),
                                          stream=st.cuda_stream)
            else:
                got, status = m.ps_decode(group, d_src.data_ptr(), n, src_on_device=True, stream=st.cuda_stream)
    st.synchronize()
    assert status == bytes(n)
    if got is None:
        got = bytes(d_dst.cpu().numpy())
    assert_points(got, want, group)


def test_threads_and_engine_cache(m):
    n = 500
    want = [affine(m, 1, 2 * n)[:n * 96], affine(m, 1, 2 * n)[n * 96:]]
    inputs = [encoded(m, 1, 2 * n, True)[:n * 48], encoded(m, 1, 2 * n, True)[n * 48:]]
    out = [None, None]
    m.release_engine_cache()

    def work(t):
        out[t] = m.ps_decode(1, inputs[t], n)

    ts = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for t in range(2):
        assert out[t] is not None and out[t][1] == bytes(n)
        assert_points(out[t][0], want[t], 1)
    live, idle, idle_bytes = m.engine_cache_stats()
    assert 1 <= idle <= 2 and live >= idle and idle_bytes > 0  # the decode engines, back in the pool
    m.release_engine_cache()
    assert m.engine_cache_stats()[1] == 0


@pytest.mark.parametrize("group", [1, 2])
def test_set_points_encoded(m, golden, group):
    n = 1024
    c = [c for c in golden(f"msm_g{group}.json")["cases"]
         if c["n"] == n and c["seed"] == 1 and c["nbits"] == 255 and c["case"] == "rand"][0]
    enc = encoded(m, group, n, True)
    sc = m.gen_scalars(n, 1)
    ctx = m.MSMContext(group, 0, 10)
    ctx.set_points_encoded(enc, n)
    assert ctx.n == n and ctx.first_bad is None
    assert m.compress(group, ctx.mult(sc)).hex() == c["compressed"]
    # entry 700 replaced by an off-curve x: rejected, the context keeps its points
    E = ei.ENC[group]
    off = ei.with_flags(ei.be_bytes(group, ei.OFF_CURVE[group][0]), 0x80)
    bad = enc[:700 * E] + off + enc[701 * E:]
    ctx.set_points(affine(m, group, 16), 16)
    small = m.compress(group, ctx.mult(m.gen_scalars(16, 5)))
    with pytest.raises(m.MsmError) as e:
        ctx.set_points_encoded(bad, n)
    assert "700" in str(e.value) and "status 2" in str(e.value)
    assert ctx.first_bad == 700 and ctx.n == 16
    assert m.compress(group, ctx.mult(m.gen_scalars(16, 5))) == small
    # serialized input
    ctx.set_points_encoded(encoded(m, group, n, False), n, compressed=False)
    assert m.compress(group, ctx.mult(sc)).hex() == c["compressed"]
    ctx.close()
