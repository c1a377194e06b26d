"""ZCash-encoded BLS12-381 points in plain Python integers (no library
arithmetic), shared by the bulk decode tests and tests/golden/make_decode_golden.py.

  encode(group, affine, n, compressed)   blst affine Montgomery bytes -> 48 G / 96 G bytes per point
  decode_entry(group, entry, serialized) one entry -> (status, affine Montgomery bytes), the rules of
                                         blst_p{1,2}_uncompress / _deserialize (status 0 ok, 1 bad
                                         encoding, 2 not on the curve, 3 not in the group: G1 x = 0)
  in_group(group, affine_entry)          [r]P == infinity, by double-and-add on Jacobians
  mixed_batch(group, serialized)         the ~130-entry batch of good and bad entries the tests and
                                         the golden file share (bad entries between good ones)

Encoding: big-endian coordinates (G2: imaginary part first), byte 0 carries
0x80 compressed, 0x40 infinity, 0x20 sign of y (y > (p - 1) / 2; for G2 the
imaginary part decides unless it is zero).
"""
from jac_inputs import AFF, P, R384, fnv  # noqa: F401

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
RINV = pow(R384, -1, P)
HALF = (P - 1) // 2
ENC = {1: 48, 2: 96}  # compressed bytes per point; serialized is twice that
B = {1: 4, 2: (4, 4)}
GEN = {
    1: (0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb,
        0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1),
    2: ((0x024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8,
         0x13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e),
        (0x0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801,
         0x0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be)),
}


# ---------------------------------------------------------------- fields ----
def f_add(g, a, b):
    return (a + b) % P if g == 1 else ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f_sub(g, a, b):
    return (a - b) % P if g == 1 else ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f_mul(g, a, b):
    if g == 1:
        return a * b % P
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f_neg(g, a):
    return -a % P if g == 1 else (-a[0] % P, -a[1] % P)


def f_zero(g):
    return 0 if g == 1 else (0, 0)


def f_small(g, k):
    return k % P if g == 1 else (k % P, 0)


def fp_sqrt(a):
    """a root of a in Fp, or None (p = 3 mod 4)"""
    y = pow(a, (P + 1) // 4, P)
    return y if y * y % P == a % P else None


def f_sqrt(g, a):
    """some root of a, or None.  Fp2: x0^2 = (a0 +- sqrt(a0^2 + a1^2)) / 2, x1 = a1 / (2 x0)"""
    if g == 1:
        return fp_sqrt(a)
    a0, a1 = a
    if a1 == 0:
        s = fp_sqrt(a0)
        if s is not None:
            return (s, 0)
        return (0, fp_sqrt(-a0 % P))  # -1 is a non-residue: one of a0, -a0 has a root
    n = fp_sqrt((a0 * a0 + a1 * a1) % P)
    if n is None:
        return None
    inv2 = (P + 1) // 2
    for s in (n, -n % P):
        x0 = fp_sqrt((a0 + s) * inv2 % P)
        if x0:
            x = (x0, a1 * pow(2 * x0, -1, P) % P)
            if f_mul(2, x, x) == (a0 % P, a1 % P):
                return x
    return None


def curve_rhs(g, x):
    return f_add(g, f_mul(g, f_mul(g, x, x), x), B[g])


def y_sign(g, y):
    """the 0x20 flag of y"""
    if g == 1:
        return y > HALF
    return y[1] > HALF if y[1] else y[0] > HALF


# ----------------------------------------------------------- byte layouts ----
def comps(g, v):
    return [v] if g == 1 else [v[0], v[1]]


def from_comps(g, c):
    return c[0] if g == 1 else (c[0], c[1])


def mont_bytes(g, v):
    """a field element in blst's layout (Montgomery, R = 2^384, little-endian limbs; Fp2: c0 then c1)"""
    return b"".join((c * R384 % P).to_bytes(48, "little") for c in comps(g, v))


def from_mont(g, raw):
    return from_comps(g, [int.from_bytes(raw[48 * k:48 * (k + 1)], "little") * RINV % P for k in range(g)])


def be_bytes(g, v):
    """a field element as the encoding stores it (plain value, big-endian; Fp2: c1 then c0).
    Values up to 2^384 - 1 are representable (the out-of-range cases)."""
    return b"".join(c.to_bytes(48, "big") for c in reversed(comps(g, v)))


def from_be(g, raw):
    return from_comps(g, list(reversed([int.from_bytes(raw[48 * k:48 * (k + 1)], "big") for k in range(g)])))


def affine_bytes(g, pt):
    """pt = (x, y) or None (infinity: all zero)"""
    if pt is None:
        return bytes(AFF[g])
    return mont_bytes(g, pt[0]) + mont_bytes(g, pt[1])


def affine_point(g, raw):
    if not any(raw):
        return None
    co = 48 * g
    return (from_mont(g, raw[:co]), from_mont(g, raw[co:2 * co]))


def with_flags(raw, flags):
    return bytes([raw[0] | flags]) + raw[1:]


def encode_point(g, pt, compressed):
    if pt is None:
        return bytes([0xc0 if compressed else 0x40]) + bytes(ENC[g] * (1 if compressed else 2) - 1)
    if compressed:
        return with_flags(be_bytes(g, pt[0]), 0x80 | (0x20 if y_sign(g, pt[1]) else 0))
    return be_bytes(g, pt[0]) + be_bytes(g, pt[1])


def encode(g, affine, n, compressed=True):
    raw = bytes(affine)
    return b"".join(encode_point(g, affine_point(g, raw[i * AFF[g]:(i + 1) * AFF[g]]), compressed) for i in range(n))


# ------------------------------------------------------------------ decode ----
def _in_range(g, v):
    return all(c < P for c in comps(g, v))


def _uncompress(g, e):
    in0 = e[0]
    if not in0 & 0x80:
        return 1, None
    if in0 & 0x40:
        return (0, None) if in0 == 0xc0 and not any(e[1:ENC[g]]) else (1, None)
    x = from_be(g, bytes([in0 & 0x1f]) + e[1:ENC[g]])
    if not _in_range(g, x):
        return 1, None
    y = f_sqrt(g, curve_rhs(g, x))
    if y is None:
        return 2, None
    if y_sign(g, y) != bool(in0 & 0x20):
        y = f_neg(g, y)
    if g == 1 and x == 0:
        return 3, (x, y)
    return 0, (x, y)


def decode_entry(g, entry, serialized=False):
    """(status, affine bytes); the affine bytes of every failed entry are all zero"""
    e = bytes(entry)
    if not serialized or e[0] & 0x80:
        st, pt = _uncompress(g, e)
    elif e[0] & 0xe0 == 0:
        x, y = from_be(g, e[:ENC[g]]), from_be(g, e[ENC[g]:2 * ENC[g]])
        if not (_in_range(g, x) and _in_range(g, y)):
            st, pt = 1, None
        elif f_mul(g, y, y) != curve_rhs(g, x):
            st, pt = 2, None
        else:
            st, pt = (3 if g == 1 and x == 0 else 0), (x, y)
    else:
        st, pt = (0 if e[0] == 0x40 and not any(e[1:2 * ENC[g]]) else 1), None
    return st, affine_bytes(g, pt if st == 0 else None)


def decode(g, data, n, serialized=False):
    sz = ENC[g] * (2 if serialized else 1)
    out = [decode_entry(g, data[i * sz:(i + 1) * sz], serialized) for i in range(n)]
    return [s for s, _ in out], b"".join(a for _, a in out)


# ------------------------------------------------------------- curve group ----
def _jdbl(g, p):
    x, y, z = p
    if z == f_zero(g):
        return p
    a = f_mul(g, x, x)
    b = f_mul(g, y, y)
    c = f_mul(g, b, b)
    t = f_add(g, x, b)
    d = f_sub(g, f_sub(g, f_mul(g, t, t), a), c)
    d = f_add(g, d, d)
    e = f_add(g, f_add(g, a, a), a)
    f = f_mul(g, e, e)
    x3 = f_sub(g, f, f_add(g, d, d))
    c8 = f_add(g, c, c)
    c8 = f_add(g, c8, c8)
    c8 = f_add(g, c8, c8)
    y3 = f_sub(g, f_mul(g, e, f_sub(g, d, x3)), c8)
    z3 = f_mul(g, f_add(g, y, y), z)
    return (x3, y3, z3)


def _jadd_affine(g, p, q):
    """Jacobian p + affine q (q not infinity)"""
    x1, y1, z1 = p
    if z1 == f_zero(g):
        return (q[0], q[1], f_small(g, 1))
    zz = f_mul(g, z1, z1)
    u2 = f_mul(g, q[0], zz)
    s2 = f_mul(g, q[1], f_mul(g, zz, z1))
    h = f_sub(g, u2, x1)
    r = f_sub(g, s2, y1)
    if h == f_zero(g):
        if r == f_zero(g):
            return _jdbl(g, p)
        return (f_small(g, 1), f_small(g, 1), f_zero(g))
    hh = f_mul(g, h, h)
    hhh = f_mul(g, hh, h)
    v = f_mul(g, x1, hh)
    x3 = f_sub(g, f_sub(g, f_mul(g, r, r), hhh), f_add(g, v, v))
    y3 = f_sub(g, f_mul(g, r, f_sub(g, v, x3)), f_mul(g, y1, hhh))
    return (x3, y3, f_mul(g, z1, h))


def scalar_mul_is_inf(g, pt, k):
    acc = (f_small(g, 1), f_small(g, 1), f_zero(g))
    for bit in bin(k)[2:]:
        acc = _jdbl(g, acc)
        if bit == "1":
            acc = _jadd_affine(g, acc, pt)
    return acc[2] == f_zero(g)


_IN_GROUP = {}


def in_group(g, affine_entry):
    """[r]P == infinity for the affine Montgomery bytes of P (infinity: True)"""
    pt = affine_point(g, bytes(affine_entry))
    if pt is None:
        return True
    key = (g, pt)
    if key not in _IN_GROUP:
        _IN_GROUP[key] = scalar_mul_is_inf(g, pt, R)
    return _IN_GROUP[key]


def _affine_dbl(g, pt):
    x, y = pt
    xx = f_mul(g, x, x)
    num = f_add(g, f_add(g, xx, xx), xx)
    den = f_add(g, y, y)
    if g == 1:
        inv = pow(den, -1, P)
    else:
        nrm = pow((den[0] * den[0] + den[1] * den[1]) % P, -1, P)
        inv = (den[0] * nrm % P, -den[1] * nrm % P)
    lam = f_mul(g, num, inv)
    x3 = f_sub(g, f_mul(g, lam, lam), f_add(g, x, x))
    return (x3, f_sub(g, f_mul(g, lam, f_sub(g, x, x3)), y))


_FIXED = {}


def fixed_points(g, n):
    """P_i = 2^(i+1) G, i < n, as (x, y) (the points msm_blst_amd.fixed_points returns)"""
    pts = _FIXED.setdefault(g, [])
    while len(pts) < n:
        pts.append(_affine_dbl(g, pts[-1] if pts else GEN[g]))
    return pts[:n]


def fixed_affine(g, n):
    return b"".join(affine_bytes(g, pt) for pt in fixed_points(g, n))


# --------------------------------------------------------------- the batch ----
MIXED_N = 131  # crosses two wave boundaries
OFF_CURVE = {1: [1, 2, 3, 7, 13], 2: [(k, 1) for k in (6, 10, 15, 16)]}
OFF_GROUP = {1: [4, 5, 6, 8, 9], 2: [(k, 1) for k in (1, 2, 3, 4, 5)]}


def _compressed_specials(g):
    """(class name, 48 G bytes) of every compressed special case"""
    E = ENC[g]
    out = [("infinity", bytes([0xc0]) + bytes(E - 1)),
           ("infinity_stray_low_bit", bytes([0xc0]) + bytes(E - 2) + b"\x01"),
           ("infinity_stray_byte0", bytes([0xc1]) + bytes(E - 1)),
           ("infinity_stray_later_byte", bytes([0xc0]) + bytes(10) + b"\x04" + bytes(E - 12)),
           ("infinity_sign_bit", bytes([0xe0]) + bytes(E - 1))]
    good = encode_point(g, fixed_points(g, 3)[2], True)
    out.append(("compressed_bit_clear", bytes([good[0] & 0x7f]) + good[1:]))
    out.append(("compressed_bit_clear_no_flags", bytes([good[0] & 0x1f]) + good[1:]))
    out.append(("infinity_bit_alone", bytes([0x40]) + bytes(E - 1)))
    for d in (0, 1):  # x = p and x = p + 1 fit under the three masked bits
        if g == 1:
            out.append((f"x_ge_p_{d}", with_flags(be_bytes(1, P + d), 0x80 | 0x20 * d)))
        else:
            out.append((f"x1_ge_p_{d}", with_flags(be_bytes(2, (5, P + d)), 0x80)))
            out.append((f"x0_ge_p_{d}", with_flags(be_bytes(2, (P + d, 5)), 0xa0)))
    for i, x in enumerate(OFF_CURVE[g]):
        out.append(("off_curve", with_flags(be_bytes(g, x), 0x80 | 0x20 * (i & 1))))
    out.append(("x_zero", with_flags(be_bytes(g, f_zero(g)), 0x80)))
    out.append(("x_zero", with_flags(be_bytes(g, f_zero(g)), 0xa0)))
    for i, x in enumerate(OFF_GROUP[g]):
        out.append(("off_group", with_flags(be_bytes(g, x), 0x80 | 0x20 * (i & 1))))
        if i < 2:
            out.append(("off_group", with_flags(be_bytes(g, x), 0x80 | 0x20 * (1 - (i & 1)))))
    return out


def _serialized_specials(g):
    E = 2 * ENC[g]
    pts = fixed_points(g, 8)
    x, y = pts[5]
    one = f_small(g, 1)
    out = [("infinity", bytes([0x40]) + bytes(E - 1)),
           ("infinity_stray_low_bit", bytes([0x40]) + bytes(E - 2) + b"\x01"),
           ("infinity_stray_in_y", bytes([0x40]) + bytes(ENC[g] + 3) + b"\x80" + bytes(E - ENC[g] - 5)),
           ("sign_flag_alone", bytes([0x20]) + bytes(E - 1)),
           ("sign_flag_on_a_point", with_flags(encode_point(g, pts[4], False), 0x20)),
           ("infinity_and_sign", bytes([0x60]) + bytes(E - 1)),
           ("y_plus_one", be_bytes(g, x) + be_bytes(g, f_add(g, y, one))),
           ("y_negated_is_valid", be_bytes(g, x) + be_bytes(g, f_neg(g, y)))]
    if g == 1:
        out.append(("y_eq_p", be_bytes(1, x) + be_bytes(1, P)))
        out.append(("y_top_bits", be_bytes(1, x) + with_flags(be_bytes(1, y), 0x80)))
        out.append(("x_ge_p", be_bytes(1, P) + be_bytes(1, y)))
        out.append(("x_zero", be_bytes(1, 0) + be_bytes(1, 2)))
        out.append(("x_zero", be_bytes(1, 0) + be_bytes(1, P - 2)))
    else:
        out.append(("y1_eq_p", be_bytes(2, x) + be_bytes(2, (y[0], P))))
        out.append(("y0_eq_p", be_bytes(2, x) + be_bytes(2, (P, y[1]))))
        out.append(("x0_ge_p", be_bytes(2, (P + 1, x[1])) + be_bytes(2, y)))
        out.append(("x_zero", bytes(ENC[2]) + be_bytes(2, (2, 2))))
    for i, xo in enumerate(OFF_GROUP[g][:3]):  # on the curve, outside the subgroup
        yo = f_sqrt(g, curve_rhs(g, xo))
        out.append(("off_group", be_bytes(g, xo) + be_bytes(g, f_neg(g, yo) if i & 1 else yo)))
    out.append(("off_curve", be_bytes(g, OFF_CURVE[g][0]) + be_bytes(g, f_small(g, 3))))
    # entries with the compressed bit set: their first 48 G bytes decode as a compressed point
    filler = bytes((7 * k + 1) & 0xff for k in range(ENC[g]))
    for name, e in _compressed_specials(g):
        if name.startswith("compressed_bit_clear") or name == "infinity_bit_alone":
            continue
        out.append(("compressed_in_serialized_" + name, e + filler))
    out.append(("compressed_in_serialized_good", encode_point(g, pts[6], True) + filler))
    out.append(("compressed_in_serialized_good", encode_point(g, (pts[7][0], f_neg(g, pts[7][1])), True) + filler))
    return out


def mixed_batch(g, serialized=False):
    """(bytes of MIXED_N entries, class name per entry); "good" entries are the
    fixed points 2^(i+1) G and their negatives, so both values of the sign flag occur"""
    specials = _serialized_specials(g) if serialized else _compressed_specials(g)
    n_good = MIXED_N - len(specials)
    assert n_good >= len(specials) // 2 + 2, "more special cases than room between good entries"
    pts = fixed_points(g, (n_good + 1) // 2)
    goods = []
    for k in range(n_good):
        x, y = pts[k // 2]
        goods.append(("good", encode_point(g, (x, f_neg(g, y) if k & 1 else y), not serialized)))
    out = []
    ns = len(specials)
    for i in range(MIXED_N):  # the special cases spread evenly over the batch, good entries between them
        if (i + 1) * ns // MIXED_N > i * ns // MIXED_N:
            out.append(specials.pop(0))
        else:
            out.append(goods.pop(0))
    assert not goods and not specials
    return b"".join(e for _, e in out), [name for name, _ in out]


def expected(g, serialized, check_group):
    """the batch decoded by this module: (statuses, affine bytes with failed entries zeroed)"""
    data, _ = mixed_batch(g, serialized)
    st, aff = decode(g, data, MIXED_N, serialized)
    if check_group:
        A = AFF[g]
        aff = bytearray(aff)
        for i in range(MIXED_N):
            if st[i] == 0 and not in_group(g, aff[i * A:(i + 1) * A]):
                st[i] = 3
                aff[i * A:(i + 1) * A] = bytes(A)
        aff = bytes(aff)
    return st, aff
