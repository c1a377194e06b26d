"""GPU parity of the NTT over group elements (msm_points_ntt / ps_ntt,
msm_kzg_ctx_create_monomial / KZGContext.from_monomial; csrc/points_ntt.hip on the plan
of csrc/points_ntt_plan.hpp) on an MI355X.

Oracle: for scalars a_j held as Python integers the inputs are P_j = [a_j]G and the
expected result of a transform is [fr_inputs.ntt(a)_k]G; both sides are made by
ps_mult on the generator, which its own goldens pin to the reference
(tests/pntt_inputs.py).  tests/golden/points_ntt.json holds the reference's own sums at
n = 8, tests/golden/kzg.json its Lagrange SRS at n = 16.  Every comparison is byte for
byte.
"""
import ctypes
import json
import os

import pytest

import enc_inputs as ei
import fr_inputs as fi
import kzg_inputs as ki
import pntt_inputs as pi

pytestmark = pytest.mark.gpu

R = fi.R
HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = [(False, False), (True, False), (False, True), (True, True)]
_CACHE = {}


@pytest.fixture(scope="module")
def m():
    import msm_blst_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible")
    return m


@pytest.fixture(autouse=True)
def _no_overrides(monkeypatch):
    monkeypatch.delenv("MSM_POINTS_NTT_SLICE", raising=False)
    monkeypatch.delenv("MSM_POINTS_NTT_CHUNK", raising=False)


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def scalars(count, seed, zeros=()):
    a = list(fi.rand_values(count, seed))
    for i in zeros:
        a[i % count] = 0
    return a


def points(m, group, a):
    """[a_j]G as affine bytes (computed once per input)"""
    return cached(("pts", group, tuple(a)), lambda: pi.gen_mults(m, group, a))


def check(m, group, a, log_n, batch=1, inverse=False, bitrev=False, what=""):
    got = m.ps_ntt(group, points(m, group, a), log_n, batch, inverse=inverse, bitrev=bitrev)
    want = points(m, group, pi.ntt_scalars(a, log_n, batch, inverse=inverse, bitrev=bitrev))
    if got != want:
        bad = pi.diff(got, want, group)
        raise AssertionError(f"G{group} log_n {log_n} batch {batch} inverse {inverse} bitrev {bitrev}: "
                             f"{len(bad)} differing points {bad[:8]} {what}")
    return got


# ---------------------------------------------------------------- goldens ----
@pytest.mark.parametrize("group", [1, 2])
def test_golden(m, group):
    """n = 8 against the reference's own sums of blst_p{1,2}_mult results"""
    with open(os.path.join(HERE, "golden", "points_ntt.json")) as f:
        g = json.load(f)
    e, n = g["groups"][str(group)], 1 << g["log_n"]

    def decode(entries):
        pts, st = m.ps_decode(group, bytes.fromhex("".join(entries)), n)
        assert not any(st)
        return pts

    src = decode(e["inputs"])
    assert src == points(m, group, pi.golden_scalars())
    assert m.ps_ntt(group, src, g["log_n"]) == decode(e["forward"])
    assert m.ps_ntt(group, src, g["log_n"], inverse=True) == decode(e["inverse"])


@pytest.fixture(scope="module")
def kzg_gold(m):
    with open(os.path.join(HERE, "golden", "kzg.json")) as f:
        g = json.load(f)
    log_n = g["log_n"]
    srs, st = m.ps_decode(1, bytes.fromhex("".join(g["srs"])), 1 << log_n)
    tau_g2, st2 = m.ps_decode(2, bytes.fromhex(g["tau_g2"]), 1)
    assert not any(st) and not any(st2) and int(g["tau"], 16) == ki.TAU
    mono = pi.gen_mults(m, 1, [pow(ki.TAU, i, R) for i in range(1 << log_n)])
    return {"g": g, "log_n": log_n, "srs": srs, "tau_g2": tau_g2, "mono": mono}


def test_kzg_golden_srs(m, kzg_gold):
    """the inverse transform of the powers of tau is the reference's Lagrange SRS"""
    k = kzg_gold
    assert m.ps_ntt(1, k["mono"], k["log_n"], inverse=True) == k["srs"]
    rev = m.ps_ntt(1, k["mono"], k["log_n"], inverse=True, bitrev=True)
    n = 1 << k["log_n"]
    assert rev == b"".join(pi.point_at(k["srs"], 1, pi.brev(i, k["log_n"])) for i in range(n))


def test_kzg_golden_from_monomial(m, kzg_gold):
    """KZGContext.from_monomial reproduces the golden's commitments and proofs"""
    g, log_n = kzg_gold["g"], kzg_gold["log_n"]
    ctx = m.KZGContext.from_monomial(log_n, kzg_gold["mono"], kzg_gold["tau_g2"])
    try:
        polys = ki.golden_polys()
        comp = lambda pts, k: [m.ps_encode(1, pts, k)[48 * i:48 * i + 48].hex() for i in range(k)]  # noqa: E731
        assert comp(ctx.commit(fi.pack([v for f in polys for v in f]), 3), 3) == g["commitments"]
        rep = fi.pack([v for j, row in enumerate(g["openings"]) for _ in row for v in polys[j]])
        zs = [int(o["z"], 16) for row in g["openings"] for o in row]
        proofs, y = ctx.open(rep, fi.pack(zs), len(zs))
        assert y == fi.pack([int(o["y"], 16) for row in g["openings"] for o in row])
        assert comp(proofs, len(zs)) == [o["proof"] for row in g["openings"] for o in row]
    finally:
        ctx.close()


# ------------------------------------------------------------ small sizes ----
@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 6, 7, 8])
def test_small_sizes(m, group, log_n):
    """the copy (0), the level with no ladder alone (1), one table level (2), the first real
    twiddle table (3); at 2^7 the 64 butterflies are one G1 wave and two G2 waves, at 2^8 the
    128 are one G1 block and two G2 blocks"""
    n = 1 << log_n
    for batch in (1, 3):
        a = scalars(batch * n, 5000 + 10 * log_n + batch, zeros=(2,) if log_n else ())
        for inverse, bitrev in FLAGS:
            check(m, group, a, log_n, batch, inverse, bitrev)


# ------------------------------------------------- the branches of the add ----
@pytest.mark.parametrize("group", [1, 2])
def test_all_inputs_the_same_point(m, group):
    """every first-level butterfly doubles and has a difference of infinity, hence an infinity
    table and an infinity ladder: [n]P at 0, infinity elsewhere"""
    log_n = 4
    n, c = 1 << log_n, scalars(1, 5100)[0]
    got = check(m, group, [c] * n, log_n)
    s = ei.AFF[group]
    assert got[:s] == pi.gen_mults(m, group, [c * n]) and got[s:] == bytes(s * (n - 1))
    check(m, group, [c] * n, log_n, inverse=True)
    check(m, group, [c] * n, log_n, bitrev=True)


@pytest.mark.parametrize("group", [1, 2])
def test_single_point_at_index_one(m, group):
    """infinity plus P on both sides of every butterfly it meets: output [omega^k]P"""
    log_n = 4
    n, c = 1 << log_n, scalars(1, 5101)[0]
    a = [0] * n
    a[1] = c
    got = check(m, group, a, log_n)
    w = fi.root(log_n)
    assert got == pi.gen_mults(m, group, [c * pow(w, k, R) for k in range(n)])
    check(m, group, a, log_n, inverse=True, bitrev=True)


@pytest.mark.parametrize("group", [1, 2])
def test_alternating_signs_and_infinities(m, group):
    log_n = 4
    n, c = 1 << log_n, scalars(1, 5102)[0]
    alt = [c if j % 2 == 0 else R - c for j in range(n)]  # P, -P, P, -P, ..: sums of infinity
    got = check(m, group, alt, log_n)
    s = ei.AFF[group]
    assert [k for k in range(n) if any(pi.point_at(got, group, k))] == [n // 2]
    check(m, group, alt, log_n, inverse=True)
    check(m, group, alt, log_n, bitrev=True)  # read as P .. P, -P .. -P: every first-level sum is infinity
    for inverse, bitrev in FLAGS:  # all infinity
        assert m.ps_ntt(group, bytes(s * n), log_n, inverse=inverse, bitrev=bitrev) == bytes(s * n)
    a = scalars(2 * n, 5103, zeros=(0, 3, 4, 9, 15, 16, 21, 31))  # zeros scattered
    for inverse, bitrev in FLAGS:
        check(m, group, a, log_n, 2, inverse, bitrev)


# ----------------------------------------------------- slices and chunks ----
@pytest.mark.parametrize("group", [1, 2])
def test_slices_and_chunks(m, monkeypatch, group):
    """log_n = 5, batch 5: a level in several ragged slices, a slice that spans two
    transforms; three chunks; a transform longer than the chunk -- against the unsliced call"""
    log_n, batch = 5, 5
    a = scalars(batch << log_n, 5200, zeros=(7, 40))
    src = points(m, group, a)
    plain = {f: check(m, group, a, log_n, batch, *f) for f in FLAGS}
    for name, value in (("MSM_POINTS_NTT_SLICE", "5"), ("MSM_POINTS_NTT_CHUNK", "64"), ("MSM_POINTS_NTT_CHUNK", "1")):
        monkeypatch.delenv("MSM_POINTS_NTT_SLICE", raising=False)
        monkeypatch.delenv("MSM_POINTS_NTT_CHUNK", raising=False)
        monkeypatch.setenv(name, value)
        for f in FLAGS:
            assert m.ps_ntt(group, src, log_n, batch, inverse=f[0], bitrev=f[1]) == plain[f], (name, value, f)
    monkeypatch.setenv("MSM_POINTS_NTT_SLICE", "7")  # both at once
    monkeypatch.setenv("MSM_POINTS_NTT_CHUNK", "64")
    assert m.ps_ntt(group, src, log_n, batch, inverse=True, bitrev=True) == plain[(True, True)]


# ------------------------------------------------------------ round trips ----
@pytest.mark.parametrize("group,log_n", [(1, 10), (2, 8)])
def test_round_trips(m, group, log_n):
    src = points(m, group, scalars(1 << log_n, 5300 + group))
    assert m.ps_ntt(group, m.ps_ntt(group, src, log_n), log_n, inverse=True) == src
    assert m.ps_ntt(group, m.ps_ntt(group, src, log_n, inverse=True, bitrev=True), log_n, bitrev=True) == src


# ---------------------------------------------------- multi-level sizes ----
def test_g1_4096_inverse_bitrev(m):
    """the EIP-4844 shape"""
    check(m, 1, scalars(1 << 12, 5400, zeros=(100,)), 12, inverse=True, bitrev=True)


def test_g2_1024_forward(m):
    check(m, 2, scalars(1 << 10, 5401, zeros=(5,)), 10)


@pytest.mark.parametrize("log_n,bitrev", [(10, False), (10, True), (12, False), (12, True)])
def test_from_monomial_on_a_built_srs(m, log_n, bitrev):
    """the context from [tau^i]G1 commits and opens as the Lagrange context of
    test_gpu_kzg.test_commit_and_open_on_a_built_srs: a random, a constant (its proof is
    infinity) and the zero polynomial against [f(tau)]G1 and [q(tau)]G1"""
    n, tau = 1 << log_n, ki.TAU
    D = cached(("dom", log_n, bitrev), lambda: ki.domain(log_n, bitrev))
    lag = cached(("lag", log_n, bitrev), lambda: ki.lagrange_at(tau, log_n, bitrev, D))
    powers = cached(("pow", log_n), lambda: [pow(tau, i, R) for i in range(n)])
    mono = points(m, 1, powers)
    ctx = m.KZGContext.from_monomial(log_n, mono, ki.p2_bytes(ki.g2(tau)), bitrev=bitrev)
    try:
        c = fi.rand_values(1, 1000 + log_n)[0]
        f = cached(("poly", log_n), lambda: fi.rand_values(n, 1010))
        polys = [f, [c] * n, [0] * n]
        zs = [fi.rand_values(1, 1020)[0], D[5], D[n - 1]]
        ftau = ki.eval_at(f, lag)
        y0 = cached(("eq", log_n, bitrev), lambda: ki.eval_quot(f, zs[0], log_n, bitrev, D))[0]
        want_c = [ftau, c, 0]
        want_p = [(ftau - y0) * ki.inv0(tau - zs[0]) % R, 0, 0]
        flat = fi.pack([v for p in polys for v in p])
        assert ctx.commit(flat, 3) == b"".join(ki.p1_bytes(ki.g1(k)) for k in want_c)
        proofs, y = ctx.open(flat, fi.pack(zs), 3)
        assert y == fi.pack([y0, c, 0])
        assert proofs == b"".join(ki.p1_bytes(ki.g1(k)) for k in want_p)
    finally:
        ctx.close()


# ---------------------------------------------------------- device memory ----
@pytest.mark.parametrize("group", [1, 2])
def test_device_memory_on_either_side(m, monkeypatch, group):
    import torch
    monkeypatch.setenv("MSM_POINTS_NTT_CHUNK", "64")  # two transforms per chunk, two chunks
    log_n, batch = 5, 3
    a = scalars(batch << log_n, 5500 + group, zeros=(11,))
    src = points(m, group, a)
    want = points(m, group, pi.ntt_scalars(a, log_n, batch, inverse=True))
    dev = torch.device("cuda:0")

    def up(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    def down(t):
        return bytes(t.cpu().numpy())

    d_src = up(src)
    d_dst = torch.zeros(len(src), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    # device -> host, host -> device
    assert m.ps_ntt(group, d_src.data_ptr(), log_n, batch, inverse=True, src_on_device=True) == want
    assert m.ps_ntt(group, src, log_n, batch, inverse=True, dst=d_dst.data_ptr()) is None
    torch.cuda.synchronize()
    assert down(d_dst) == want and down(d_src) == src
    # device -> device on a stream: the source is unchanged; then back in place
    d_dst.zero_()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        m.ps_ntt(group, d_src.data_ptr(), log_n, batch, inverse=True, src_on_device=True, dst=d_dst.data_ptr(),
                 stream=s.cuda_stream)
    s.synchronize()
    assert down(d_dst) == want and down(d_src) == src
    with torch.cuda.stream(s):
        m.ps_ntt(group, d_dst.data_ptr(), log_n, batch, src_on_device=True, dst=d_dst.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    assert down(d_dst) == src
    # in place on the host
    buf = (ctypes.c_uint8 * len(src)).from_buffer_copy(src)
    m.check(m.lib().msm_points_ntt(group, 0, buf, buf, log_n, batch, 1, 0, 0, None))
    assert bytes(buf) == want
    # the engines are pooled and counted
    live, idle, nbytes = m.engine_cache_stats()
    assert live >= 1 and idle >= 1 and nbytes > 0


def test_from_monomial_with_a_device_srs(m, kzg_gold):
    import torch
    k = kzg_gold
    d = torch.frombuffer(bytearray(k["mono"]), dtype=torch.uint8).to(torch.device("cuda:0"))
    torch.cuda.synchronize()
    ctx = m.KZGContext.from_monomial(k["log_n"], d.data_ptr(), k["tau_g2"], srs_on_device=True)
    try:
        polys = ki.golden_polys()
        got = ctx.commit(fi.pack(polys[0]), 1)
        assert m.ps_encode(1, got, 1).hex() == k["g"]["commitments"][0]
        assert bytes(d.cpu().numpy()) == k["mono"]
    finally:
        ctx.close()
