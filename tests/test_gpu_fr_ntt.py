"""GPU parity of the Fr layer (msm_fr_op, msm_fr_ntt / fr_op, fr_ntt;
csrc/fr_ntt.hip) on an MI355X.

Oracle: tests/fr_inputs.py in plain Python integers; tests/golden/fr_ops.json holds
the reference's own answers on the special values and the hash of its 2^10-point
transform.  Every comparison is byte for byte.  Sizes stay at 2^16 elements or
fewer: the oracle is the cost.
"""
import ctypes
import json
import os
import threading

import pytest

import enc_inputs as ei
import fr_inputs as fi

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fr_ops.json")
_CACHE = {}


@pytest.fixture(scope="module")
def m():
    import msm_blst_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible")
    return m


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(autouse=True)
def _no_overrides(monkeypatch):
    monkeypatch.delenv("MSM_NTT_TILE", raising=False)
    monkeypatch.delenv("MSM_NTT_CHUNK", raising=False)


def values(count, seed):
    """`count` random elements (computed once, never modified)"""
    key = ("v", count, seed)
    if key not in _CACHE:
        _CACHE[key] = fi.rand_values(count, seed)
    return _CACHE[key]


def expected(log_n, batch, seed, inverse=False, shift=None):
    key = ("e", log_n, batch, seed, inverse, shift)
    if key not in _CACHE:
        _CACHE[key] = fi.ntt_batch(values(batch << log_n, seed), log_n, batch, inverse=inverse, shift=shift)
    return _CACHE[key]


def assert_elems(got, want, what="", per=1):
    """byte for byte; names the differing elements (per > 1: the differing transforms)"""
    assert len(got) == len(want), what
    if got != want:
        w = 32 * per
        bad = [i for i in range(len(want) // w) if got[i * w:(i + 1) * w] != want[i * w:(i + 1) * w]]
        raise AssertionError(f"{len(bad)} differing {'transforms' if per > 1 else 'elements'} {bad[:8]} {what}")


# ------------------------------------------------------------------ fr_op ----
def test_ops_on_the_special_pairs(m, golden):
    vals = fi.special_values()
    frs = [fi.fr_bytes(v) for v in vals]
    k = len(frs)
    a2 = b"".join(a for a in frs for _ in frs)
    b2 = b"".join(frs) * k
    for op in fi.OPS:
        if op in fi.BINARY:
            got = m.fr_op(op, a2, b2)
            want = b"".join(fi.op_bytes(op, a, b) for a in frs for b in frs)
        else:
            src = fi.pack(vals, scalar=True) if op == "from_scalar" else b"".join(frs)
            got = m.fr_op(op, src)
            want = b"".join(fi.op_bytes(op, src[i:i + 32]) for i in range(0, len(src), 32))
        assert_elems(got, want, op)
        assert [got[i:i + 32].hex() for i in range(0, len(got), 32)] == golden[op], op
    wide = fi.pack([int(v, 16) for v, _ in golden["from_scalar_wide"]], scalar=True)
    assert m.fr_op("from_scalar", wide).hex() == "".join(w for _, w in golden["from_scalar_wide"])


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_ops_on_random_elements(m, n):
    a, b = fi.pack(values(n, 11)), fi.pack(values(n, 12))
    for op in fi.OPS:
        src = fi.pack(values(n, 11), scalar=True) if op == "from_scalar" else a
        got = m.fr_op(op, src, b if op in fi.BINARY else None)
        want = b"".join(fi.op_bytes(op, src[i:i + 32], b[i:i + 32]) for i in range(0, 32 * n, 32))
        assert_elems(got, want, f"{op} n={n}")


def test_inverse_with_zeros(m):
    n = 300
    base = list(values(n, 13))
    for zeros in ([0], [n - 1], [100, 101], [0, 7, 8, 63, 64, 299], list(range(n))):
        v = list(base)
        for z in zeros:
            v[z] = 0
        got = m.fr_op("inv", fi.pack(v))
        want = fi.pack([pow(x, fi.R - 2, fi.R) for x in v])
        assert_elems(got, want, f"zeros at {zeros[:6]}")
    assert m.fr_op("inv", bytes(32)) == bytes(32)


def test_b_one(m):
    n = 65
    a, k = values(n, 14), values(1, 15)[0]
    for op, f in (("add", lambda x: x + k), ("sub", lambda x: x - k), ("mul", lambda x: x * k)):
        got = m.fr_op(op, fi.pack(a), fi.fr_bytes(k), b_one=True)
        assert_elems(got, fi.pack([f(x) % fi.R for x in a]), op)


def test_ops_in_place_on_the_device(m):
    import torch
    n = 257
    a, b = values(n, 16), values(n, 17)
    dev = torch.device("cuda:0")
    for op, want in (("mul", [x * y % fi.R for x, y in zip(a, b)]), ("inv", [pow(x, fi.R - 2, fi.R) for x in a]),
                     ("neg", [-x % fi.R for x in a])):
        d_a = torch.frombuffer(bytearray(fi.pack(a)), dtype=torch.uint8).to(dev)
        d_b = torch.frombuffer(bytearray(fi.pack(b)), dtype=torch.uint8).to(dev)
        torch.cuda.synchronize()
        assert m.fr_op(op, d_a.data_ptr(), d_b.data_ptr(), n, src_on_device=True, dst=d_a.data_ptr()) is None
        torch.cuda.synchronize()
        assert_elems(bytes(d_a.cpu().numpy()), fi.pack(want), f"{op} dst = a")
        assert bytes(d_b.cpu().numpy()) == fi.pack(b)
    # dst = b, and dst = a on the host
    d_a = torch.frombuffer(bytearray(fi.pack(a)), dtype=torch.uint8).to(dev)
    d_b = torch.frombuffer(bytearray(fi.pack(b)), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize()
    m.fr_op("sub", d_a.data_ptr(), d_b.data_ptr(), n, src_on_device=True, dst=d_b.data_ptr())
    torch.cuda.synchronize()
    assert_elems(bytes(d_b.cpu().numpy()), fi.pack([(x - y) % fi.R for x, y in zip(a, b)]), "sub dst = b")
    h = (ctypes.c_uint8 * (32 * n)).from_buffer_copy(fi.pack(a))
    m.check(m.lib().msm_fr_op(0, m.FR_OPS["sqr"], h, h, None, n, 0, 0, 0, None))
    assert_elems(bytes(h), fi.pack([x * x % fi.R for x in a]), "sqr in place on the host")


# ------------------------------------------------------------- transforms ----
def run_ntt(m, log_n, batch, seed, **kw):
    return m.fr_ntt(fi.pack(values(batch << log_n, seed)), log_n, batch, **kw)


@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 5, 6, 7, 9, 10, 11, 12, 16])
def test_default_plan(m, log_n):
    batch = 3 if log_n <= 12 else 1
    seed = 20 + log_n
    fwd = run_ntt(m, log_n, batch, seed)
    assert_elems(fwd, fi.pack(expected(log_n, batch, seed)), f"forward 2^{log_n}")
    inv = run_ntt(m, log_n, batch, seed, inverse=True)
    assert_elems(inv, fi.pack(expected(log_n, batch, seed, inverse=True)), f"inverse 2^{log_n}")
    back = m.fr_ntt(fwd, log_n, batch, inverse=True)
    assert_elems(back, fi.pack(values(batch << log_n, seed)), f"inverse of forward 2^{log_n}")


def test_golden_hash(m, golden):
    g = golden["ntt"]
    got = m.fr_ntt(fi.pack(fi.rand_values(1 << g["log_n"], g["seed"])), g["log_n"])
    assert ei.fnv(got) == g["fnv"]


@pytest.mark.parametrize("tile,log_n", [(4, 3), (4, 4), (4, 5), (4, 8), (4, 9), (4, 12), (4, 13), (2, 7), (11, 11),
                                        (11, 12)])
@pytest.mark.parametrize("batch", [1, 3])
def test_pass_structure_at_small_sizes(m, tile, log_n, batch, monkeypatch):
    monkeypatch.setenv("MSM_NTT_TILE", str(tile))
    plan = m.ntt_plan(log_n)
    assert sum(plan) == log_n and (len(plan) > 1) == (log_n > tile)
    seed = 50 + log_n
    assert_elems(run_ntt(m, log_n, batch, seed), fi.pack(expected(log_n, batch, seed)), f"forward {plan}")
    assert_elems(run_ntt(m, log_n, batch, seed, inverse=True), fi.pack(expected(log_n, batch, seed, inverse=True)),
                 f"inverse {plan}")


@pytest.mark.parametrize("log_n", [1, 4])
@pytest.mark.parametrize("batch", [1, 63, 64, 65, 1000])
def test_sub_tile_batching(m, log_n, batch):
    """many transforms share a workgroup; each is checked alone"""
    seed = 70 + log_n
    assert_elems(run_ntt(m, log_n, batch, seed), fi.pack(expected(log_n, batch, seed)), "forward", per=1 << log_n)
    assert_elems(run_ntt(m, log_n, batch, seed, inverse=True), fi.pack(expected(log_n, batch, seed, inverse=True)),
                 "inverse", per=1 << log_n)


@pytest.mark.parametrize("src_scalar", [False, True])
@pytest.mark.parametrize("dst_scalar", [False, True])
def test_forms(m, src_scalar, dst_scalar):
    log_n, batch, seed = 8, 2, 80
    v = values(batch << log_n, seed)
    for inverse in (False, True):
        got = m.fr_ntt(fi.pack(v, scalar=src_scalar), log_n, batch, inverse=inverse, src_scalar=src_scalar,
                       dst_scalar=dst_scalar)
        assert_elems(got, fi.pack(expected(log_n, batch, seed, inverse=inverse), scalar=dst_scalar),
                     f"inverse={inverse}")
    # log_n = 0: a copy, or a change of form
    got = m.fr_ntt(fi.pack(v, scalar=src_scalar), 0, len(v), src_scalar=src_scalar, dst_scalar=dst_scalar)
    assert_elems(got, fi.pack(v, scalar=dst_scalar), "log_n = 0")


def test_scalar_source_above_r(m):
    log_n = 6
    wide = [fi.R, fi.R + 1, (1 << 256) - 1, 2 * fi.R + 5] + [v + fi.R for v in values(60, 81)]
    assert all(fi.R <= w < 1 << 256 for w in wide)
    got = m.fr_ntt(fi.pack(wide, scalar=True), log_n, src_scalar=True)
    assert_elems(got, fi.pack(fi.ntt([w % fi.R for w in wide])))


@pytest.mark.parametrize("shift", [7, "random"])
@pytest.mark.parametrize("log_n", [0, 3, 8, 14])
def test_coset_shift(m, shift, log_n):
    s = fi.rand_values(1, 82)[0] if shift == "random" else shift
    seed = 83 + log_n
    ev = run_ntt(m, log_n, 1, seed, shift=s)
    assert_elems(ev, fi.pack(expected(log_n, 1, seed, shift=s)), "forward")
    back = m.fr_ntt(ev, log_n, inverse=True, shift=s.to_bytes(32, "little"))
    assert_elems(back, fi.pack(values(1 << log_n, seed)), "inverse of forward")
    inv = run_ntt(m, log_n, 1, seed, inverse=True, shift=s, dst_scalar=True)
    assert_elems(inv, fi.pack(expected(log_n, 1, seed, inverse=True, shift=s), scalar=True), "inverse, scalar form")


# ------------------------------------------------------------------ paths ----
@pytest.mark.parametrize("path", ["h2h", "h2d", "d2h", "d2d", "inplace"])
def test_paths_on_a_stream(m, path, monkeypatch):
    """Sources written by torch copies queued on a non-default stream just before the
    call (behind a device-side delay): the call must order itself after them, in
    every one of its chunks (batch 5 at log_n 6 in chunks of two transforms: three)."""
    import torch
    monkeypatch.setenv("MSM_NTT_CHUNK", "128")
    log_n, batch, seed = 6, 5, 90
    src = fi.pack(values(batch << log_n, seed))
    exp = fi.pack(expected(log_n, batch, seed))
    if path == "h2h":
        assert_elems(m.fr_ntt(src, log_n, batch), exp, per=64)
        return
    dev = torch.device("cuda:0")
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
            hp = (ctypes.c_uint8 * len(src)).from_address(h_src.data_ptr())
            got = m.fr_ntt(hp, log_n, batch, dst=d_dst.data_ptr(), stream=st.cuda_stream)
        else:
            d_src.copy_(pinned, non_blocking=True)
            dst = {"d2h": None, "d2d": d_dst.data_ptr(), "inplace": d_src.data_ptr()}[path]
            got = m.fr_ntt(d_src.data_ptr(), log_n, batch, src_on_device=True, dst=dst, stream=st.cuda_stream)
    st.synchronize()
    if got is None:
        got = bytes((d_src if path == "inplace" else d_dst).cpu().numpy())
    assert_elems(got, exp, path, per=64)


def test_transform_larger_than_the_chunk(m, monkeypatch):
    monkeypatch.setenv("MSM_NTT_CHUNK", "128")
    log_n, batch, seed = 8, 3, 91
    assert_elems(run_ntt(m, log_n, batch, seed), fi.pack(expected(log_n, batch, seed)), per=256)
    a = values(700, 92)
    assert_elems(m.fr_op("inv", fi.pack(a)), fi.pack([pow(x, fi.R - 2, fi.R) for x in a]), "inv in six chunks")


def test_hand_off_to_the_msm(m):
    """coefficients -> evaluations -> (on the device) coefficients in scalar form ->
    msm_ctx_mult(on_device) commits to the same point as the host scalars do"""
    import torch
    log_n = 10
    n = 1 << log_n
    c = values(n, 93)
    evals = m.fr_ntt(fi.pack(c), log_n)
    dev = torch.device("cuda:0")
    d_ev = torch.frombuffer(bytearray(evals), dtype=torch.uint8).to(dev)
    d_sc = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx = m.MSMContext(1, 0, 10)
    try:
        ctx.set_points(m.fixed_points(1, n), n)
        assert m.fr_ntt(d_ev.data_ptr(), log_n, inverse=True, dst_scalar=True, src_on_device=True,
                        dst=d_sc.data_ptr()) is None
        got = m.compress(1, ctx.mult(d_sc.data_ptr(), on_device=True))
        want = m.compress(1, ctx.mult(fi.pack(c, scalar=True)))
    finally:
        ctx.close()
    assert bytes(d_sc.cpu().numpy()) == fi.pack(c, scalar=True)
    assert got == want


def test_threads_and_engine_cache(m):
    cases = [(9, 2, 94), (12, 1, 95)]
    out = [None, None]
    m.release_engine_cache()
    before = m.engine_cache_stats()

    def work(t):
        log_n, batch, seed = cases[t]
        out[t] = run_ntt(m, log_n, batch, seed)

    for t in range(2):
        expected(*cases[t])  # (the oracle, before the threads start)
    ts = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for t in range(2):
        assert out[t] is not None
        assert_elems(out[t], fi.pack(expected(*cases[t])), f"thread {t}")
    live, idle, idle_bytes = m.engine_cache_stats()
    assert 1 <= idle - before[1] <= 2 and live >= idle and idle_bytes > before[2]  # the engines, back in the pool
    m.release_engine_cache()
    assert m.engine_cache_stats()[1] == 0


def test_probe(m):
    rate, ms = m.fr_probe()
    assert rate > 1e9 and ms > 0
