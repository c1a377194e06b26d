"""Hash-to-curve for BLS12-381 (RFC 9380: expand_message_xmd with SHA-256,
hash_to_field, simplified SWU onto the isogenous curve, isogeny, cofactor
clearing) in plain Python integers and hashlib, shared by the bulk
hash-to-curve tests and tests/golden/make_hash_to_curve_golden.py.

  dst_prime(dst)                         DST || I2OSP(len, 1) after the oversize rule
  expand_message_xmd(msg, dst, n)        n uniform bytes
  hash_to_field(g, msg, dst, count, aug) count elements of Fp (g = 1) or Fp2 (g = 2)
  sswu(g, u)                             a point of E' (affine)
  iso(g, pt)                             its image on E
  clear_cofactor(g, pt)                  G1: [1 - z]P; G2: the effective cofactor through psi
  map_to_curve(g, us)                    blst_map_to_g{1,2}(u, v or NULL) as an affine point or None
  hash_to_curve(g, msg, dst, aug, encode)
  messages(), special_u(g), map_cases(g), CASES   the inputs the tests and the golden file share

The constants are tools/h2c_constants.py, the project's own table.
"""
import hashlib
import os
import sys

from enc_inputs import (AFF, P, _jadd_affine, _jdbl, affine_bytes, encode_point, f_add, f_mul, f_neg,  # noqa: F401
                        f_small, f_sqrt, f_sub, f_zero, fnv, from_mont, mont_bytes)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import h2c_constants as hc  # noqa: E402

DST = {g: f"BLS_SIG_BLS12381G{g}_XMD:SHA-256_SSWU_RO_NUL_".encode() for g in (1, 2)}
ELEM = {1: 48, 2: 96}  # bytes of a field element in blst's layout


# ------------------------------------------------------------- hash to field ----
def dst_prime(dst):
    if len(dst) > 255:
        dst = hashlib.sha256(b"H2C-OVERSIZE-DST-" + dst).digest()
    return dst + bytes([len(dst)])


def expand_message_xmd(msg, dst, len_in_bytes):
    ell = (len_in_bytes + 31) // 32
    assert ell <= 255 and len_in_bytes < 65536
    dp = dst_prime(dst)
    b0 = hashlib.sha256(bytes(64) + msg + len_in_bytes.to_bytes(2, "big") + b"\0" + dp).digest()
    b = [hashlib.sha256(b0 + b"\1" + dp).digest()]
    for i in range(2, ell + 1):
        b.append(hashlib.sha256(bytes(x ^ y for x, y in zip(b0, b[-1])) + bytes([i]) + dp).digest())
    return b"".join(b)[:len_in_bytes]


def hash_to_field(g, msg, dst, count, aug=b""):
    """count elements; aug is prepended to msg (the reference's argument)"""
    uniform = expand_message_xmd(aug + msg, dst, count * g * 64)
    vals = [int.from_bytes(uniform[64 * k:64 * (k + 1)], "big") % P for k in range(count * g)]
    return vals if g == 1 else [(vals[2 * k], vals[2 * k + 1]) for k in range(count)]


def field_bytes(g, elems):
    return b"".join(mont_bytes(g, e) for e in elems)


# -------------------------------------------------------------------- fields ----
def f_inv(g, a):
    if g == 1:
        return pow(a, -1, P)
    n = pow((a[0] * a[0] + a[1] * a[1]) % P, -1, P)
    return (a[0] * n % P, -a[1] * n % P)


def f_pow(g, a, e):
    r = f_small(g, 1)
    for bit in bin(e)[2:]:
        r = f_mul(g, r, r)
        if bit == "1":
            r = f_mul(g, r, a)
    return r


def sgn0(g, a):
    if g == 1:
        return a & 1
    return (a[0] & 1) | ((a[0] == 0) & (a[1] & 1))


def _rhs(g, x, a, b):
    return f_add(g, f_add(g, f_mul(g, f_mul(g, x, x), x), f_mul(g, a, x)), b)


# ---------------------------------------------------------- the map onto E' ----
def sswu(g, u):
    A, B, Z = hc.A[g], hc.B[g], hc.Z[g]
    zuu = f_mul(g, Z, f_mul(g, u, u))
    tv1 = f_add(g, f_mul(g, zuu, zuu), zuu)
    if tv1 == f_zero(g):
        x1 = f_mul(g, B, f_inv(g, f_mul(g, Z, A)))
    else:
        x1 = f_mul(g, f_mul(g, f_neg(g, B), f_inv(g, A)), f_add(g, f_small(g, 1), f_inv(g, tv1)))
    x = x1
    y = f_sqrt(g, _rhs(g, x, A, B))
    if y is None:
        x = f_mul(g, zuu, x1)
        y = f_sqrt(g, _rhs(g, x, A, B))
        assert y is not None
    if sgn0(g, u) != sgn0(g, y):
        y = f_neg(g, y)
    return (x, y)


def add_affine(g, p, q, a):
    """p + q on y^2 = x^3 + a x + b, affine points or None"""
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if p[1] != q[1] or p[1] == f_zero(g):
            return None
        xx = f_mul(g, p[0], p[0])
        num = f_add(g, f_add(g, f_add(g, xx, xx), xx), a)
        lam = f_mul(g, num, f_inv(g, f_add(g, p[1], p[1])))
    else:
        lam = f_mul(g, f_sub(g, q[1], p[1]), f_inv(g, f_sub(g, q[0], p[0])))
    x3 = f_sub(g, f_sub(g, f_mul(g, lam, lam), p[0]), q[0])
    return (x3, f_sub(g, f_mul(g, lam, f_sub(g, p[0], x3)), p[1]))


def _poly(g, coeffs, x):
    acc = f_zero(g)
    for c in reversed(coeffs):
        acc = f_add(g, f_mul(g, acc, x), c if g == 2 else c % P)
    return acc


def iso(g, pt):
    """the 11-isogeny E1' -> E1 / the 3-isogeny E2' -> E2"""
    if pt is None:
        return None
    xn, xd, yn, yd = (_poly(g, c, pt[0]) for c in hc.ISO[g])
    if xd == f_zero(g) or yd == f_zero(g):
        return None
    return (f_mul(g, xn, f_inv(g, xd)), f_mul(g, pt[1], f_mul(g, yn, f_inv(g, yd))))


# ------------------------------------------------------------- the curve E ----
def neg_pt(g, p):
    return None if p is None else (p[0], f_neg(g, p[1]))


def add_pt(g, p, q):
    return add_affine(g, p, q, f_zero(g))


def to_affine(g, j):
    if j[2] == f_zero(g):
        return None
    zi = f_inv(g, j[2])
    zi2 = f_mul(g, zi, zi)
    return (f_mul(g, j[0], zi2), f_mul(g, j[1], f_mul(g, zi2, zi)))


def smul(g, pt, k):
    if pt is None or k == 0:
        return None
    acc = (f_small(g, 1), f_small(g, 1), f_zero(g))
    for bit in bin(k)[2:]:
        acc = _jdbl(g, acc)
        if bit == "1":
            acc = _jadd_affine(g, acc, pt)
    return to_affine(g, acc)


_PSI = {}


def psi(pt):
    """the untwist-Frobenius-twist endomorphism of E2"""
    if pt is None:
        return None
    if not _PSI:
        base = f_inv(2, (1, 1))
        _PSI["x"] = f_pow(2, base, (P - 1) // 3)
        _PSI["y"] = f_pow(2, base, (P - 1) // 2)
    conj = lambda a: (a[0], -a[1] % P)  # noqa: E731
    return (f_mul(2, conj(pt[0]), _PSI["x"]), f_mul(2, conj(pt[1]), _PSI["y"]))


def clear_cofactor(g, pt):
    z = hc.Z_ABS  # the curve parameter is -z
    if g == 1:
        return smul(1, pt, z + 1)
    # Budroni-Pintore: [z^2 - z - 1]P + [z - 1]psi(P) + psi^2(2P), with -z = |z|
    t1 = neg_pt(2, psi(pt))
    out = add_pt(2, add_pt(2, psi(psi(add_pt(2, pt, pt))), neg_pt(2, pt)), t1)
    t0 = add_pt(2, add_pt(2, smul(2, pt, z), pt), t1)
    return add_pt(2, out, smul(2, t0, z))


def map_to_curve(g, us):
    """blst_map_to_g{1,2}(us[0], us[1] if given): affine point or None"""
    q = sswu(g, us[0])
    if len(us) == 2:
        q = add_affine(g, q, sswu(g, us[1]), hc.A[g])
    return clear_cofactor(g, iso(g, q))


def hash_to_curve(g, msg, dst, aug=b"", encode=False):
    return map_to_curve(g, hash_to_field(g, msg, dst, 1 if encode else 2, aug))


def on_curve(g, pt, a, b):
    return pt is None or f_mul(g, pt[1], pt[1]) == _rhs(g, pt[0], a, b)


def entry(g, pt):
    """what the fixture stores per point: the compressed encoding and an FNV of the affine bytes"""
    return {"c": encode_point(g, pt, True).hex(), "fnv": fnv(affine_bytes(g, pt))}


# ------------------------------------------------------------------ inputs ----
MIXED_N = 131  # every SHA block-boundary residue, two wave boundaries


def _bytes(n, salt):
    return bytes((salt * 131 + 7 * j + (j * j >> 3) + 1) & 0xff for j in range(n))


def messages():
    """message i has i bytes for i < 130, the last one 1000"""
    return [_bytes(i, i) for i in range(MIXED_N - 1)] + [_bytes(1000, 130)]


def distinct_messages(n):
    return [b"msg-%06d" % i + _bytes(i % 37, i) for i in range(n)]


# the 8-message cases: name -> (messages, DST, aug bytes per message or None, fixed length)
def _case(dst_len=None, aug_len=0, fixed=False, g=1):
    msgs = [_bytes(32, 200 + i) for i in range(8)] if fixed else [_bytes(40 + i, 40 + i) for i in range(8)]
    dst = DST[g] if dst_len is None else _bytes(dst_len, 250)
    aug = [_bytes(aug_len, 220 + i) for i in range(8)] if aug_len else None
    return msgs, dst, aug, fixed


CASES = {"dst0": dict(dst_len=0), "dst255": dict(dst_len=255), "dst256": dict(dst_len=256),
         "dst300": dict(dst_len=300), "aug48": dict(aug_len=48), "aug96": dict(aug_len=96), "fixed32": dict(fixed=True)}


def case(g, name):
    return _case(g=g, **CASES[name])


def special_u(g):
    """0, 1, p - 1, the values with xd == 0, a few random ones.  xd = -A (Z^2 u^4 + Z u^2)
    vanishes at u = 0 and at u^2 = -1 / Z: over Fp that is +-sqrt(-1/11); over Fp2
    -1 / Z = 1 / (2 + i) is a non-square, so no such u exists for G2."""
    from jac_inputs import SplitMix64
    rng = SplitMix64(0x68326331 + g)
    minus_inv_z = f_neg(g, f_inv(g, hc.Z[g]))
    root = f_sqrt(g, minus_inv_z)
    if g == 1:
        assert root is not None
        out = [0, 1, P - 1, root, P - root] + [rng.fp() for _ in range(4)]
    else:
        assert root is None, "-1/Z is a non-square in Fp2"
        out = [(0, 0), (1, 0), (P - 1, 0), (0, 1), (0, P - 1), (P - 1, P - 1)] + [(rng.fp(), rng.fp()) for _ in range(4)]
    return out


def map_cases(g):
    """(the count = 1 inputs, the count = 2 pairs): every special u alone and beside its
    neighbour, a pair u == v (the doubling on E') and a pair u == -v (infinity)"""
    us = special_u(g)
    pairs = [(us[k], us[(k + 1) % len(us)]) for k in range(len(us))]
    pairs += [(us[-1], us[-1]), (us[-2], f_neg(g, us[-2])), (us[1], us[1]), (us[3], f_neg(g, us[3]))]
    return us, pairs
