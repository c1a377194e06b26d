"""Inputs and expected values for the bulk scalar multiplication out[i] = [k_i]P_i,
in plain Python integers (no library arithmetic), shared by the points-mult tests
and tests/golden/make_points_mult_golden.py.  Builds on enc_inputs.py.

  smul(g, pt, k)          [k]pt as (x, y) or None, by double-and-add on enc_inputs'
                          Jacobian formulas: the oracle of truth
  scalar_classes(nbits)   (name, integer) of every special scalar, cut to nbits bits
  gen_scalars(n, seed)    the integers of msm_gen_scalars (SplitMix64, < r)
  small_order_points(g)   (order, point): points of order 3 and 11 (G1), 13 and 23
                          (G2) on the curve outside the prime-order subgroup; a ladder
                          over them meets acc == +-row and infinity at almost every step
  special_batch(g, nbits) (names, points, scalars, in_group flags) of SPECIAL_N entries
  scalar_bytes(ks, stride) / points_bytes(g, pts) the byte layouts of the C ABI
"""
import enc_inputs as ei
from jac_inputs import SplitMix64

R = ei.R
P = ei.P
Z = -0xd201000000010000
assert Z ** 4 - Z ** 2 + 1 == R
# cofactors of E(Fp) and E'(Fp2) (the BLS12 family polynomials)
H = {1: (Z - 1) ** 2 // 3,
     2: (Z ** 8 - 4 * Z ** 7 + 5 * Z ** 6 - 4 * Z ** 4 + 6 * Z ** 3 - 4 * Z ** 2 - 4 * Z + 13) // 9}
SMALL = {1: [(3, 1, 5), (11, 2, 6)], 2: [(13, 2, (1, 1)), (23, 2, (2, 1))]}  # (q, e with q^e || h, x of the source point)
for _g in (1, 2):
    for _q, _e, _ in SMALL[_g]:
        assert H[_g] % _q ** _e == 0 and H[_g] % _q ** (_e + 1) != 0
SPECIAL_N = 200  # G1: crosses three waves of 64 lanes; G2 (lane pairs): six waves of 32 pairs


def _f_inv(g, a):
    if g == 1:
        return pow(a, -1, P)
    n = pow((a[0] * a[0] + a[1] * a[1]) % P, -1, P)
    return (a[0] * n % P, -a[1] * n % P)


def _to_affine(g, j):
    x, y, z = j
    if z == ei.f_zero(g):
        return None
    zi = _f_inv(g, z)
    zi2 = ei.f_mul(g, zi, zi)
    return (ei.f_mul(g, x, zi2), ei.f_mul(g, y, ei.f_mul(g, zi2, zi)))


def smul(g, pt, k):
    """[k]pt for k >= 0; pt = (x, y) or None (infinity)"""
    if pt is None or k == 0:
        return None
    acc = (ei.f_small(g, 1), ei.f_small(g, 1), ei.f_zero(g))
    for bit in bin(k)[2:]:
        acc = ei._jdbl(g, acc)
        if bit == "1":
            acc = ei._jadd_affine(g, acc, pt)
    return _to_affine(g, acc)


def gen_scalars(n, seed):
    """SplitMix64(seed), 4 little-endian words, word 3 >>= 1, values >= r rejected"""
    rng = SplitMix64(seed)
    out = []
    while len(out) < n:
        w = [rng.next() for _ in range(4)]
        w[3] >>= 1
        v = w[0] | w[1] << 64 | w[2] << 128 | w[3] << 192
        if v < R:
            out.append(v)
    return out


def scalar_classes(nbits=255):
    out = [(str(k), k) for k in (0, 1, 2, 3, 7, 8, 9, 15, 16, 17)]
    for j in (4, 5, 63, 64, 65, 127, 128, 254, 255):
        out += [(f"2^{j}", 1 << j), (f"2^{j}-1", (1 << j) - 1)]
    out += [("r-2", R - 2), ("r-1", R - 1), ("r", R), ("r+1", R + 1), ("r+2", R + 2), ("(r-1)/2", (R - 1) // 2),
            ("(r+1)/2", (R + 1) // 2), ("2r", 2 * R), ("2^256-1", (1 << 256) - 1)]
    out += [(f"bytes_{b:02x}", int.from_bytes(bytes([b]) * 32, "little")) for b in (0x88, 0x77, 0xff, 0x0f, 0xf0)]
    # 2r and 2^256 - 1 are for nbits = 256; every other class is cut to nbits (what the kernel's mask does)
    return [(n, k & ((1 << nbits) - 1)) for n, k in out if nbits >= 256 or n not in ("2r", "2^256-1")]


_SMALL = {}


def small_order_points(g):
    """[(q, T)] with T of order exactly q, from the off-group x of enc_inputs.OFF_GROUP"""
    if g not in _SMALL:
        out = []
        for q, e, x in SMALL[g]:
            assert x in ei.OFF_GROUP[g]
            src = (x, ei.f_sqrt(g, ei.curve_rhs(g, x)))
            assert smul(g, src, H[g] * R) is None, "cofactor"
            t = smul(g, src, H[g] * R // q ** e)
            assert t is not None, (g, q, "no component of this order")
            while smul(g, t, q) is not None:
                t = smul(g, t, q)
            out.append((q, t))
        _SMALL[g] = out
    return _SMALL[g]


def special_batch(g, nbits=255):
    """names, points ((x, y) or None), scalars (integers < 2^nbits), in_group flags;
    SPECIAL_N entries: every scalar class on an in-group point (fixed points, the
    generator), infinity inputs between good ones, every small-order point with 0,
    its order, its order +- 1, 2^255 - 1 and a few randoms"""
    fixed = ei.fixed_points(g, 16)
    rnd = gen_scalars(64, 7)
    top = (1 << min(nbits, 255)) - 1
    out = []
    for i, (name, k) in enumerate(scalar_classes(nbits)):
        out.append((name + ("@gen" if i % 5 == 0 else "@fixed"), ei.GEN[g] if i % 5 == 0 else fixed[i % 16], k, True))
    for q, t in small_order_points(g):
        for name, k in [("0", 0), ("q", q), ("q-1", q - 1), ("q+1", q + 1), ("2^255-1", top), ("r", R)] + \
                [(f"random{j}", rnd[j]) for j in range(4)]:
            out.append((f"order{q}*{name}", t, k, False))
        out.append((f"order{q}*random_neg", (t[0], ei.f_neg(g, t[1])), rnd[5], False))
    specials = len(out)
    j = 0
    while len(out) < SPECIAL_N:  # randoms on fixed points, an infinity input every 9th
        i = len(out)
        if i % 9 == 4:
            out.append(("infinity*random", None, rnd[8 + j % 40], True))
        else:
            out.append(("random", fixed[j % 16], rnd[8 + j % 40] & top, True))
        j += 1
    assert specials < SPECIAL_N - 20
    # spread: the filler entries between the special ones (deterministic interleave)
    head, tail = out[:specials], out[specials:]
    mixed, nt = [], len(tail)
    for i in range(SPECIAL_N):
        if (i + 1) * nt // SPECIAL_N > i * nt // SPECIAL_N:
            mixed.append(tail.pop(0))
        else:
            mixed.append(head.pop(0))
    assert not head and not tail
    return ([m[0] for m in mixed], [m[1] for m in mixed], [m[2] for m in mixed], [m[3] for m in mixed])


def scalar_bytes(ks, stride=32, nbytes=None):
    """little-endian scalars `stride` apart; the last one only nbytes long when given"""
    raw = b"".join(k.to_bytes(max(stride, 32), "little")[:stride] for k in ks)
    return raw if nbytes is None or not ks else raw[:(len(ks) - 1) * stride + nbytes]


def points_bytes(g, pts):
    return b"".join(ei.affine_bytes(g, pt) for pt in pts)


_EXPECTED = {}


def expected_batch(g, nbits):
    """special_batch(g, nbits) with the affine bytes smul gives for every entry (computed once)"""
    if (g, nbits) not in _EXPECTED:
        names, pts, ks, ing = special_batch(g, nbits)
        _EXPECTED[(g, nbits)] = (names, pts, ks, ing, [ei.affine_bytes(g, smul(g, p, k)) for p, k in zip(pts, ks)])
    return _EXPECTED[(g, nbits)]
