"""GPU parity of the evaluation-form polynomial call and the KZG layer
(msm_fr_eval_quotient, msm_kzg_* / fr_eval_quotient, KZGContext; csrc/fr_poly.hip,
csrc/kzg.cpp) on an MI355X.

Oracle: tests/kzg_inputs.py in plain Python integers (an insecure setup with a known
tau: commitments and proofs are multiples of the generator by f(tau) and (f(tau) - y) /
(tau - z), which do not use the evaluation-form quotient); tests/golden/kzg.json holds
the reference's own points at n = 16.  Every comparison is byte for byte.  One Python
evaluation at n = 2^12 costs about a second, so the large sizes take few points.
"""
import ctypes
import json
import os

import pytest

import enc_inputs as ei
import fr_inputs as fi
import kzg_inputs as ki

pytestmark = pytest.mark.gpu

R = fi.R
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kzg.json")
_CACHE = {}


@pytest.fixture(scope="module")
def m():
    import msm_blst_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible")
    return m


@pytest.fixture(autouse=True)
def _no_overrides(monkeypatch):
    monkeypatch.delenv("MSM_POLY_TILE", raising=False)
    monkeypatch.delenv("MSM_POLY_CHUNK", raising=False)


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def dom(log_n, bitrev=False):
    return cached(("dom", log_n, bitrev), lambda: ki.domain(log_n, bitrev))


def poly(log_n, seed):
    return cached(("poly", log_n, seed), lambda: fi.rand_values(1 << log_n, seed))


def expect(f, z, log_n, bitrev=False):
    """(y, q) of the oracle, computed once per input"""
    return cached(("eq", tuple(f), z, log_n, bitrev),
                  lambda: ki.eval_quot(f, z, log_n, bitrev, dom(log_n, bitrev)))


def check_call(m, polys, zs, log_n, bitrev=False, scalar=False, want_q=True, what=""):
    y, q = m.fr_eval_quotient(fi.pack([v for f in polys for v in f]), fi.pack(zs), log_n, len(polys), want_q=want_q,
                              dst_scalar=scalar, bitrev=bitrev)
    n = 1 << log_n
    for j, (f, z) in enumerate(zip(polys, zs)):
        wy, wq = expect(f, z, log_n, bitrev)
        assert y[32 * j:32 * j + 32] == fi.fr_bytes(wy), f"y of polynomial {j} {what}"
        if want_q:
            got, want = q[32 * n * j:32 * n * (j + 1)], fi.pack(wq, scalar=scalar)
            if got != want:
                bad = [i for i in range(n) if got[32 * i:32 * i + 32] != want[32 * i:32 * i + 32]]
                raise AssertionError(f"polynomial {j}: {len(bad)} differing quotient elements {bad[:8]} {what}")
    assert (q is None) == (not want_q)


# ------------------------------------------------------- fr_eval_quotient ----
@pytest.mark.parametrize("log_n", [0, 1, 2, 5, 6, 7])
def test_small_sizes(m, log_n):
    """one tile, some lanes idle; at 2^7 the points on each side of the wave boundary"""
    n, D = 1 << log_n, dom(log_n)
    zs = fi.rand_values(1, 300 + log_n) + [0, D[0], D[n - 1], D[min(63, n - 1)], D[64 % n]]
    for count in (1, 3, 5):
        polys = [poly(log_n, 310 + j) for j in range(count)]
        for first in (0, 3):
            check_call(m, polys, [zs[(first + j) % len(zs)] for j in range(count)], log_n, what=f"count {count}")


@pytest.mark.parametrize("log_n,idx", [(10, (0, 1023, 255, 256)), (11, (1023, 1024)), (12, (1024, 4095))])
def test_whole_tiles(m, log_n, idx):
    """four elements per lane (their boundary at 255 | 256), then two and four tiles per
    polynomial with points on each side of the tile boundary"""
    D = dom(log_n)
    zs = fi.rand_values(1, 400 + log_n) + [D[i] for i in idx]
    polys = [poly(log_n, 410 + j) for j in range(len(zs))]
    check_call(m, polys, zs, log_n)


@pytest.mark.parametrize("log_n", [3, 4, 5, 6])
@pytest.mark.parametrize("bitrev", [False, True])
def test_tile_override(m, monkeypatch, log_n, bitrev):
    """MSM_POLY_TILE=4: n below, equal to, twice and four times the tile (the combine over
    workgroups); points at index 0, n - 1 and each side of a tile boundary, the same z for
    two polynomials, a domain point beside a polynomial whose point is outside"""
    monkeypatch.setenv("MSM_POLY_TILE", "4")
    n, D = 1 << log_n, dom(log_n, bitrev)
    rnd = fi.rand_values(2, 500 + log_n)
    zs = [rnd[0], rnd[0], D[0], rnd[1], D[n - 1], D[15 % n], D[16 % n], 0, D[n // 2], 1]
    for count in (1, 3, 5):
        for first in (0, 2, 5):
            polys = [poly(log_n, 510 + j) for j in range(count)]
            check_call(m, polys, [zs[(first + j) % len(zs)] for j in range(count)], log_n, bitrev=bitrev,
                       what=f"count {count} from {first}")


def test_zero_and_constant_polynomials(m, monkeypatch):
    log_n = 5
    n, D = 1 << log_n, dom(log_n)
    c = fi.rand_values(1, 600)[0]
    polys = [[0] * n, [c] * n, poly(log_n, 601), [c] * n, [0] * n]
    zs = [fi.rand_values(1, 602)[0], D[7], D[7], fi.rand_values(1, 603)[0], D[n - 1]]
    for tile in (None, "3"):
        if tile:
            monkeypatch.setenv("MSM_POLY_TILE", tile)
        check_call(m, polys, zs, log_n, what=f"tile {tile}")
    y, q = m.fr_eval_quotient(fi.pack(polys[1]), fi.pack([zs[0]]), log_n)
    assert y == fi.fr_bytes(c) and q == bytes(32 * n)  # a constant: the quotient is zero


@pytest.mark.parametrize("scalar,want_q,bitrev", [(True, True, False), (True, True, True), (False, False, False),
                                                  (False, False, True), (True, False, False)])
def test_forms(m, monkeypatch, scalar, want_q, bitrev):
    """the blst_scalar form, no quotient, bit-reversed order: one tile and four"""
    for log_n, tile in ((6, None), (6, "4")):
        if tile:
            monkeypatch.setenv("MSM_POLY_TILE", tile)
        D = dom(log_n, bitrev)
        zs = [fi.rand_values(1, 700)[0], D[17], D[0]]
        polys = [poly(log_n, 710 + j) for j in range(3)]
        check_call(m, polys, zs, log_n, bitrev=bitrev, scalar=scalar, want_q=want_q, what=f"tile {tile}")


def test_three_chunks(m, monkeypatch):
    monkeypatch.setenv("MSM_POLY_CHUNK", "64")  # two polynomials of 32 per chunk
    log_n = 5
    D = dom(log_n)
    zs = fi.rand_values(2, 800) + [D[3], 0, D[31]]
    polys = [poly(log_n, 810 + j) for j in range(5)]
    check_call(m, polys, zs, log_n)
    check_call(m, polys, zs, log_n, scalar=True)
    monkeypatch.setenv("MSM_POLY_CHUNK", "1")  # a polynomial longer than the chunk is a chunk of its own
    check_call(m, polys[:3], zs[:3], log_n)


def test_device_memory_on_either_side(m, monkeypatch):
    import torch
    monkeypatch.setenv("MSM_POLY_CHUNK", "128")
    log_n, count = 6, 3
    n, D = 1 << log_n, dom(log_n)
    polys = [poly(log_n, 900 + j) for j in range(count)]
    zs = [fi.rand_values(1, 910)[0], D[63], D[1]]
    want_y = fi.pack([expect(f, z, log_n)[0] for f, z in zip(polys, zs)])
    want_q = b"".join(fi.pack(expect(f, z, log_n)[1]) for f, z in zip(polys, zs))
    src, zb = fi.pack([v for f in polys for v in f]), fi.pack(zs)
    dev = torch.device("cuda:0")

    def up(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    def down(t):
        return bytes(t.cpu().numpy())

    d_f, d_z = up(src), up(zb)
    d_y, d_q = torch.zeros(32 * count, dtype=torch.uint8, device=dev), torch.zeros(len(src), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    # device -> host
    y, q = m.fr_eval_quotient(d_f.data_ptr(), d_z.data_ptr(), log_n, count, src_on_device=True)
    assert (y, q) == (want_y, want_q)
    # host -> device
    assert m.fr_eval_quotient(src, zb, log_n, count, y_dst=d_y.data_ptr(), q_dst=d_q.data_ptr()) is None
    torch.cuda.synchronize()
    assert (down(d_y), down(d_q)) == (want_y, want_q)
    # device -> device on a stream, then in place
    d_y.zero_(), d_q.zero_()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        m.fr_eval_quotient(d_f.data_ptr(), d_z.data_ptr(), log_n, count, src_on_device=True, y_dst=d_y.data_ptr(),
                           q_dst=d_q.data_ptr(), stream=s.cuda_stream)
        m.fr_eval_quotient(d_f.data_ptr(), d_z.data_ptr(), log_n, count, src_on_device=True, y_dst=d_y.data_ptr(),
                           q_dst=d_f.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    assert (down(d_y), down(d_q), down(d_f), down(d_z)) == (want_y, want_q, want_q, zb)
    # in place on the host
    buf = (ctypes.c_uint8 * len(src)).from_buffer_copy(src)
    yb = (ctypes.c_uint8 * (32 * count))()
    m.check(m.lib().msm_fr_eval_quotient(0, yb, buf, buf, m._buf(zb), log_n, count, 0, 0, 0, None))
    assert (bytes(yb), bytes(buf)) == (want_y, want_q)
    # the engines are pooled and counted
    live, idle, _ = m.engine_cache_stats()
    assert live >= 1 and idle >= 1


# ------------------------------------------------------------------- KZG ----
@pytest.fixture(scope="module")
def gold(m):
    """the golden's context and its 12 honest tuples as bytes"""
    with open(GOLDEN) as f:
        g = json.load(f)
    log_n = g["log_n"]
    srs, st = m.ps_decode(1, bytes.fromhex("".join(g["srs"])), 1 << log_n)
    tau_g2, st2 = m.ps_decode(2, bytes.fromhex(g["tau_g2"]), 1)
    assert not any(st) and not any(st2)
    ctx = m.KZGContext(log_n, srs, tau_g2)
    polys = ki.golden_polys()
    lag = ki.lagrange_at(ki.TAU, log_n)
    tuples = []  # (polynomial index, z, y, commitment scalar, proof scalar)
    for j, row in enumerate(g["openings"]):
        for o in row:
            z, y = int(o["z"], 16), int(o["y"], 16)
            tuples.append((j, z, y, ki.commit_scalar(polys[j], lag), ki.proof_scalar(polys[j], z, lag, ki.TAU, log_n)[1]))
    yield {"g": g, "ctx": ctx, "polys": polys, "tuples": tuples, "log_n": log_n}
    ctx.close()


def _compressed(m, pts, k):
    return [m.ps_encode(1, pts, k)[48 * i:48 * i + 48].hex() for i in range(k)]


def test_commit_and_open_against_the_golden(m, gold):
    g, ctx, polys = gold["g"], gold["ctx"], gold["polys"]
    flat = fi.pack([v for f in polys for v in f])
    assert _compressed(m, ctx.commit(flat, 3), 3) == g["commitments"]
    rep = fi.pack([v for j, *_ in gold["tuples"] for v in polys[j]])
    zs = fi.pack([t[1] for t in gold["tuples"]])
    proofs, y = ctx.open(rep, zs, 12)
    assert y == fi.pack([t[2] for t in gold["tuples"]])
    assert _compressed(m, proofs, 12) == [o["proof"] for row in g["openings"] for o in row]


@pytest.mark.parametrize("log_n,bitrev", [(10, False), (10, True), (12, False), (12, True)])
def test_commit_and_open_on_a_built_srs(m, log_n, bitrev):
    """SRS = [l_i(tau)]G1 by ps_mult on the generator; a random, a constant (its proof is
    infinity) and the zero polynomial against [f(tau)]G1 and [q(tau)]G1"""
    n, tau = 1 << log_n, ki.TAU
    D = dom(log_n, bitrev)
    lag = cached(("lag", log_n, bitrev), lambda: ki.lagrange_at(tau, log_n, bitrev, D))
    srs = m.ps_mult(1, ei.affine_bytes(1, ei.GEN[1]), fi.pack(lag, scalar=True), n, one_point=True)
    ctx = m.KZGContext(log_n, srs, ki.p2_bytes(ki.g2(tau)), bitrev=bitrev)
    try:
        c = fi.rand_values(1, 1000 + log_n)[0]
        f = poly(log_n, 1010)
        polys = [f, [c] * n, [0] * n]
        zs = [fi.rand_values(1, 1020)[0], D[5], D[n - 1]]
        ftau = ki.eval_at(f, lag)
        y0 = expect(f, zs[0], log_n, bitrev)[0]
        want_c = [ftau, c, 0]
        want_p = [(ftau - y0) * ki.inv0(tau - zs[0]) % R, 0, 0]
        flat = fi.pack([v for p in polys for v in p])
        assert ctx.commit(flat, 3) == b"".join(ki.p1_bytes(ki.g1(k)) for k in want_c)
        proofs, y = ctx.open(flat, fi.pack(zs), 3)
        assert y == fi.pack([y0, c, 0])
        assert proofs == b"".join(ki.p1_bytes(ki.g1(k)) for k in want_p)
        assert proofs[96:] == bytes(192)
    finally:
        ctx.close()


def test_many_polynomials_round_trip(m, gold):
    """more polynomials than the context normalises on the host (1024): the sums go through
    msm_points_to_affine; a few against the oracle, all of them through verify"""
    ctx, log_n = gold["ctx"], gold["log_n"]
    n, k = 1 << log_n, 1030
    vals = fi.rand_values(n * 10, 1300)
    polys = [vals[(j % 10) * n:(j % 10 + 1) * n] for j in range(k)]
    zs = fi.rand_values(k, 1301)
    flat, zb = fi.pack([v for f in polys for v in f]), fi.pack(zs)
    C = ctx.commit(flat, k)
    PI, Y = ctx.open(flat, zb, k)
    lag = ki.lagrange_at(ki.TAU, log_n)
    for j in (0, 9, 1029):
        y, pk = ki.proof_scalar(polys[j], zs[j], lag, ki.TAU, log_n)
        assert C[96 * j:96 * j + 96] == ki.p1_bytes(ki.g1(ki.commit_scalar(polys[j], lag)))
        assert Y[32 * j:32 * j + 32] == fi.fr_bytes(y) and PI[96 * j:96 * j + 96] == ki.p1_bytes(ki.g1(pk))
    assert ctx.verify(C, zb, Y, PI, k) == bytes([1] * k)


def _tuple_bytes(tuples):
    return (b"".join(ki.p1_bytes(ki.g1(t[3])) for t in tuples), fi.pack([t[1] for t in tuples]),
            fi.pack([t[2] for t in tuples]), b"".join(ki.p1_bytes(ki.g1(t[4])) for t in tuples))


def test_verify_each_tuple(m, gold):
    ctx, tuples = gold["ctx"], gold["tuples"]
    C, Z, Y, PI = _tuple_bytes(tuples)
    assert ctx.verify(C, Z, Y, PI, 12) == bytes([1] * 12)
    assert ctx.verify(C, Z, Y, PI, 0) == b""
    # one of C, z, y, pi changed in four different tuples: those fail, and only those
    other = ki.p1_bytes(ki.g1(12345))
    C2 = C[:96] + other + C[192:]
    Z2 = Z[:32 * 4] + fi.fr_bytes(99) + Z[32 * 5:]
    Y2 = Y[:32 * 7] + fi.fr_bytes((tuples[7][2] + 1) % R) + Y[32 * 8:]
    PI2 = PI[:96 * 10] + other + PI[96 * 11:]
    want = [1] * 12
    for i in (1, 4, 7, 10):
        want[i] = 0
    assert ctx.verify(C2, Z2, Y2, PI2, 12) == bytes(want)
    for k, arrays in enumerate(((C2, Z, Y, PI), (C, Z2, Y, PI), (C, Z, Y2, PI), (C, Z, Y, PI2))):
        assert ctx.verify(*arrays, 12) == bytes(0 if i == (1, 4, 7, 10)[k] else 1 for i in range(12))


def test_verify_an_infinity_proof(m, gold):
    """a constant polynomial c opens to infinity: C = [c]G1, y = c holds at every z"""
    ctx = gold["ctx"]
    c = 0x1234567
    C = ki.p1_bytes(ki.g1(c)) * 2 + ki.p1_bytes(ki.g1(c + 1))
    Z = fi.pack([5, ki.domain(gold["log_n"])[3], 5])
    Y = fi.pack([c, c, c])
    assert ctx.verify(C, Z, Y, bytes(96 * 3), 3) == bytes([1, 1, 0])


def test_verify_weighted_batches(m, gold):
    ctx, tuples = gold["ctx"], gold["tuples"]
    five = tuples[:5]
    C, Z, Y, PI = _tuple_bytes(five)
    w = b"".join(v.to_bytes(32, "little")[:8] for v in fi.rand_values(5, 1100))
    offs = [0, 2, 2, 5]
    assert ctx.verify(C, Z, Y, PI, 5, weights=w, nbits=64, batch_offsets=offs) == bytes([1, 1, 1])
    assert ctx.verify(C, Z, Y, PI, 5, weights=w, nbits=64) == bytes([1])
    # one tuple spoiled: its batch fails alone
    bad = PI[:96 * 3] + ki.p1_bytes(ki.g1(777)) + PI[96 * 4:]
    assert ctx.verify(C, Z, Y, bad, 5, weights=w, nbits=64, batch_offsets=offs) == bytes([1, 1, 0])
    bad_y = fi.pack([(five[0][2] + 1) % R]) + Y[32:]
    assert ctx.verify(C, Z, bad_y, PI, 5, weights=w, nbits=64, batch_offsets=offs) == bytes([0, 1, 1])
    # + delta and - delta on two proofs of equal z: the plain sum still balances, a weighted one does not
    a, b = [i for i, t in enumerate(tuples) if t[1] == 0][:2]
    pair = [tuples[a], tuples[b]]
    C, Z, Y, _ = _tuple_bytes(pair)
    delta = 0xdecaf
    PI = ki.p1_bytes(ki.g1(pair[0][4] + delta)) + ki.p1_bytes(ki.g1(pair[1][4] - delta))
    ones = bytes([1, 1])
    assert ctx.verify(C, Z, Y, PI, 2) == bytes([0, 0])
    assert ctx.verify(C, Z, Y, PI, 2, weights=ones, nbits=1) == bytes([1])
    w2 = b"".join(v.to_bytes(32, "little")[:8] for v in fi.rand_values(2, 1101))
    assert ctx.verify(C, Z, Y, PI, 2, weights=w2, nbits=64) == bytes([0])


def test_round_trip_on_one_stream(m, gold):
    """commit and open into device buffers, then verify them there, all on one stream"""
    import torch
    ctx, polys, log_n = gold["ctx"], gold["polys"], gold["log_n"]
    dev = torch.device("cuda:0")
    D = ki.domain(log_n)
    zs = [fi.rand_values(1, 1200)[0], D[2], 0]
    d_f = torch.frombuffer(bytearray(fi.pack([v for f in polys for v in f])), dtype=torch.uint8).to(dev)
    d_z = torch.frombuffer(bytearray(fi.pack(zs)), dtype=torch.uint8).to(dev)
    d_c = torch.zeros(96 * 3, dtype=torch.uint8, device=dev)
    d_p = torch.zeros(96 * 3, dtype=torch.uint8, device=dev)
    d_y = torch.zeros(32 * 3, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        ctx.commit(d_f.data_ptr(), 3, src_on_device=True, dst=d_c.data_ptr(), stream=s.cuda_stream)
        ctx.open(d_f.data_ptr(), d_z.data_ptr(), 3, src_on_device=True, proofs_dst=d_p.data_ptr(), y_dst=d_y.data_ptr(),
                 stream=s.cuda_stream)
        ok = ctx.verify(d_c.data_ptr(), d_z.data_ptr(), d_y.data_ptr(), d_p.data_ptr(), 3, src_on_device=True,
                        stream=s.cuda_stream)
        w = bytes(range(1, 25))
        okw = ctx.verify(d_c.data_ptr(), d_z.data_ptr(), d_y.data_ptr(), d_p.data_ptr(), 3, weights=w, nbits=64,
                         src_on_device=True, stream=s.cuda_stream)
    s.synchronize()
    assert ok == bytes([1, 1, 1]) and okw == bytes([1])
    assert bytes(d_y.cpu().numpy()) == fi.pack([ki.eval_quot(f, z, log_n)[0] for f, z in zip(polys, zs)])
