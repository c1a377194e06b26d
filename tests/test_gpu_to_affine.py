"""GPU parity of the bulk Jacobian -> affine normalisation (msm_p{1,2}s_to_affine,
msm_points_to_affine; csrc/to_affine.hip) on an MI355X.

Oracle: tests/jac_inputs.py builds the Jacobians (x l^2, y l^3, l) from affine
points in plain Python integers, so the expected output of every finite point
is the affine input itself, byte for byte -- independent of the code under
test and of the reference; tests/golden/to_affine.json adds the FNV of the
reference's own blst_p{1,2}s_to_affine output on the same inputs.

The pointer-rule case follows ref multi_scalar.c:30 as the library states it: a
NULL entry is never stepped over, so a NULL can only be the tail of the array.
Three separate buffers of 1, 130 and 169 points are therefore named as
{p0, pA[0], ..., pA[129], pB, NULL}: explicit adjacent pointers for the middle
buffer (merged into one run), one pointer and a NULL for the last.
"""
import ctypes
import os
import re
import threading

import pytest

import jac_inputs as ji

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = ctypes.c_void_p
# group size of the product tree (the sizes below straddle it)
K = int(re.search(r"TA_K = (\d+);", open(os.path.join(REPO, "msm_blst_amd", "csrc", "to_affine.hpp")).read()).group(1))
NMAX = 4099
SIZES = [1, 2, K - 1, K, K + 1, K * K - 1, K * K + 1, 1000, NMAX]
GOLDEN_N = {1: (1000, 4099), 2: (500, 1000)}

_AFF, _JAC = {}, {}


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
    return _AFF[group][:n * ji.AFF[group]]


def jacobians(m, group, n, seed):
    key = (group, n, seed)
    if key not in _JAC:
        _JAC[key] = ji.jacobians(group, affine(m, group, n), n, seed)
    return _JAC[key]


def first_diff(got, want, sz):
    for i in range(len(want) // sz):
        if got[i * sz:(i + 1) * sz] != want[i * sz:(i + 1) * sz]:
            return i
    return None


def assert_points(got, want, group):
    assert len(got) == len(want)
    assert got == want, f"first differing point: {first_diff(got, want, ji.AFF[group])}"


def test_plan_has_two_levels_at_4099(m):
    assert K >= 2
    assert m.to_affine_levels(NMAX) >= 2  # a change of K / LEAF cannot turn the sizes test into a one-level test


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("n", SIZES + [500])
def test_sizes_host_flat(m, golden, group, n):
    seeds = {(c["group"], c["n"]): c for c in golden("to_affine.json")["cases"]}
    c = seeds.get((group, n))
    want = affine(m, group, n)
    got = m.ps_to_affine(group, jacobians(m, group, n, c["seed"] if c else 1000 + n), n)
    assert_points(got, want, group)
    if n in GOLDEN_N[group]:
        assert c is not None and ji.fnv(got) == c["fnv"]


@pytest.mark.parametrize("group", [1, 2])
def test_infinity_inputs(m, group):
    n = 4 * K + 5
    A, co = ji.AFF[group], 48 * group
    want = bytearray(affine(m, group, n))
    jac = jacobians(m, group, n, 21)
    # index 0, the last index, one whole group, both sides of a group boundary
    inf = sorted({0, n - 1, 3 * K - 1, 3 * K} | set(range(K, 2 * K)))
    for i in inf:
        jac = ji.with_z(group, jac, i, bytes(co))  # Z = 0, X and Y stay nonzero
        want[i * A:(i + 1) * A] = bytes(A)
    for i in inf:
        assert any(jac[i * ji.JAC[group]:i * ji.JAC[group] + 2 * co])
    assert_points(m.ps_to_affine(group, jac, n), bytes(want), group)
    # all infinity
    n2 = 40
    j2 = jacobians(m, group, n2, 22)
    for i in range(n2):
        j2 = ji.with_z(group, j2, i, bytes(co))
    assert m.ps_to_affine(group, j2, n2) == bytes(n2 * A)
    # Z = 1: the coordinates come back unchanged
    assert_points(m.ps_to_affine(group, ji.affine_to_jacobian_z1(group, affine(m, group, n), n), n),
                  affine(m, group, n), group)


@pytest.mark.parametrize("group", [1, 2])
def test_pointer_rule(m, group):
    n, J, A = 300, ji.JAC[group], ji.AFF[group]
    jac = jacobians(m, group, n, 31)
    f = getattr(m.lib(), f"msm_p{group}s_to_affine")

    def call(ptrs, keep):
        dst = (ctypes.c_uint8 * (A * n))()
        assert f(dst, ptrs, n) == 0, m.lib().msm_last_error()
        del keep
        return bytes(dst)

    flat_buf = (ctypes.c_uint8 * len(jac)).from_buffer_copy(jac)
    flat = call((vp * 2)(ctypes.addressof(flat_buf), None), flat_buf)
    assert_points(flat, affine(m, group, n), group)
    # three separate buffers of 1, 130 and 169 points
    b0 = (ctypes.c_uint8 * J).from_buffer_copy(jac[:J])
    bA = (ctypes.c_uint8 * (130 * J)).from_buffer_copy(jac[J:131 * J])
    bB = (ctypes.c_uint8 * (169 * J)).from_buffer_copy(jac[131 * J:])
    ptrs = [ctypes.addressof(b0)] + [ctypes.addressof(bA) + i * J for i in range(130)] + [ctypes.addressof(bB), None]
    assert_points(call((vp * len(ptrs))(*ptrs), (b0, bA, bB)), flat, group)
    # one pointer per point, in reversed order: the flat result of the reversed sequence
    rev = b"".join(jac[i * J:(i + 1) * J] for i in reversed(range(n)))
    rbuf = (ctypes.c_uint8 * len(rev)).from_buffer_copy(rev)
    flat_rev = call((vp * 2)(ctypes.addressof(rbuf), None), rbuf)
    ptrs = [ctypes.addressof(flat_buf) + i * J for i in reversed(range(n))]
    assert_points(call((vp * n)(*ptrs), flat_buf), flat_rev, group)
    assert flat_rev == b"".join(flat[i * A:(i + 1) * A] for i in reversed(range(n)))


@pytest.mark.parametrize("group", [1, 2])
def test_chunks(m, group, monkeypatch):
    n = 1000
    monkeypatch.setenv("MSM_TO_AFFINE_CHUNK", "96")  # several chunks and a ragged tail
    assert m.to_affine_levels(n) == m.to_affine_levels(96)
    assert_points(m.ps_to_affine(group, jacobians(m, group, n, 41), n), affine(m, group, n), group)


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("path", ["d2d", "h2d", "d2h"])
def test_device_memory_on_a_stream(m, group, path):
    """Source written by a torch copy queued on a non-default stream just before
    the call (behind a device-side delay): the call must order itself after it."""
    import torch
    n = 1000
    jac, want = jacobians(m, group, n, 51), affine(m, group, n)
    dev = torch.device("cuda:0")
    pinned = torch.frombuffer(bytearray(jac), dtype=torch.uint8).pin_memory()
    d_jac = torch.frombuffer(bytearray(jac), dtype=torch.uint8).to(dev)
    d_src = torch.zeros(len(jac), dtype=torch.uint8, device=dev)
    h_src = torch.zeros(len(jac), dtype=torch.uint8).pin_memory()
    d_dst = torch.zeros(len(want), dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    got = None
    with torch.cuda.stream(st):
        torch.cuda._sleep(10_000_000)
        if path == "h2d":
            h_src.copy_(d_jac, non_blocking=True)
            src = (ctypes.c_uint8 * len(jac)).from_address(h_src.data_ptr())
            m.ps_to_affine(group, src, n, dst=d_dst.data_ptr(), stream=st.cuda_stream)
        else:
            d_src.copy_(pinned, non_blocking=True)
            if path == "d2d":
                m.ps_to_affine(group, d_src.data_ptr(), n, src_on_device=True, dst=d_dst.data_ptr(),
                               stream=st.cuda_stream)
            else:
                got = m.ps_to_affine(group, d_src.data_ptr(), n, src_on_device=True, stream=st.cuda_stream)
    st.synchronize()
    if got is None:
        got = bytes(d_dst.cpu().numpy())
    assert_points(got, want, group)


@pytest.mark.parametrize("group,n", [(1, 1024), (2, 256)])
def test_chain_into_ches(m, golden, group, n):
    """Jacobians -> device affine -> CHES table built from device points -> MSM
    (G2: 256 is the smallest n with a seed-1 "rand" golden and a CHES configuration)."""
    import torch
    c = [c for c in golden(f"msm_g{group}.json")["cases"]
         if c["n"] == n and c["seed"] == 1 and c["nbits"] == 255 and c["case"] == "rand"][0]
    jac = ji.jacobians(group, bytes(m.fixed_points(group, n)), n, 61)
    d_aff = torch.zeros(n * ji.AFF[group], dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    m.ps_to_affine(group, jac, n, dst=d_aff.data_ptr())
    ctx = m.CHESContext(group, 0, n_exp=n.bit_length() - 1)
    ctx.build_table(d_aff.data_ptr(), n, on_device=True)
    got = m.compress(group, ctx.mult(m.gen_scalars(n, 1)))
    ctx.close()
    assert got.hex() == c["compressed"]


def test_threads_and_engine_cache(m):
    n = 1000
    want = affine(m, 1, n)
    inputs = [jacobians(m, 1, n, 70 + t) for t in range(4)]
    out = [None] * 4

    def work(t):
        out[t] = m.ps_to_affine(1, inputs[t], n)

    ts = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for t in range(4):
        assert out[t] is not None
        assert_points(out[t], want, 1)
    assert m.engine_cache_stats()[1] > 0
    m.release_engine_cache()
    assert m.engine_cache_stats()[1] == 0
