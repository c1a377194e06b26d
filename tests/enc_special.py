"""Inputs of the bulk encoder's tests (msm_points_encode) in plain Python
integers, shared by tests/test_encode_host.py, tests/test_gpu_encode.py and
tests/golden/make_encode_golden.py.

  affine_batch(group)     (raw affine bytes of SPECIAL_N entries, class name per entry): points,
                          coordinate pairs that are no points on every decision boundary of the
                          encoder, infinity runs, limbs at and above p
  jacobian_batch(group)   (raw Jacobian bytes of JAC_N entries, class name per entry): random Z,
                          Z = 1, Z = 0 with X and Y left in place
  jacobian_zero(group)    JAC_ZERO_N Jacobians, every Z = 0
  expected(group, raw, n, compressed, jacobian)   the entries the reference writes, by
                          enc_inputs.encode_point (Jacobians normalised here first)
  signed_points(group, n) the fixed points 2^(i+1) G, each followed by its negative (both sign
                          flags), as (x, y) pairs

The reference answers every entry of every batch (tests/golden/encode.json pins
the Python encoder to it), so no test skips any.
"""
import enc_inputs as ei
import jac_inputs as ji

P, HALF, R384 = ei.P, ei.HALF, ji.R384
SPECIAL_N = 131  # crosses two wave boundaries (G2, lane pairs: four)
JAC_N = 101      # 13 groups of eight, the last one partial
JAC_ZERO_N = 17


def _mont(v):
    return v * R384 % P


def _raw(g, x, y, add_x=0, add_y=0):
    """affine bytes of the pair (x, y); add_*: a multiple of p added to every stored limb set"""
    out = b""
    for v, add in ((x, add_x), (y, add_y)):
        for c in ei.comps(g, v):
            out += (_mont(c) + add).to_bytes(48, "little")
    return out


def _small(g, k):
    return k if g == 1 else (k, k + 1)


def signed_points(g, n):
    pts = ei.fixed_points(g, (n + 1) // 2)
    return [(pts[i // 2][0], ei.f_neg(g, pts[i // 2][1]) if i & 1 else pts[i // 2][1]) for i in range(n)]


def on_curve_finite(g, n):
    """n finite points of the curve: signed fixed points, then the OFF_GROUP points with both roots"""
    out = []
    for x in ei.OFF_GROUP[g]:
        y = ei.f_sqrt(g, ei.curve_rhs(g, x))
        out += [(x, y), (x, ei.f_neg(g, y))]
    return (signed_points(g, n - len(out)) + out)[:n]


def _specials(g):
    """(class name, raw affine bytes) of every special entry but the infinity runs"""
    out = []
    if g == 1:
        out.append(("x_zero_y_two", _raw(1, 0, 2)))
    else:
        out.append(("x_zero_y_two", _raw(2, (0, 0), (2, 2))))
    for x in ei.OFF_CURVE[g]:
        out.append(("off_curve", _raw(g, x, _small(g, 3))))
    for x in ei.OFF_GROUP[g]:
        y = ei.f_sqrt(g, ei.curve_rhs(g, x))
        out.append(("off_group", _raw(g, x, y)))
        out.append(("off_group", _raw(g, x, ei.f_neg(g, y))))
    x5 = _small(g, 5)
    if g == 1:
        for y in (0, 1, HALF, HALF + 1, P - 1):
            out.append(("y_boundary", _raw(1, x5, y)))
        for x in (0, P - 1):
            out.append(("x_boundary", _raw(1, x, 7)))
    else:
        for c in (0, 1, HALF, HALF + 1, P - 1):
            out.append(("y_re_only", _raw(2, x5, (c, 0))))   # the real part decides
            out.append(("y_im_only", _raw(2, x5, (0, c))))   # c = 0: y = (0, 0), x non-zero
            for d in (1, HALF, HALF + 1, P - 1):
                out.append(("y_im_decides", _raw(2, x5, (c, d))))
        for x in ((0, 0), (0, 1), (1, 0), (P - 1, P - 1), (0, P - 1), (P - 1, 0)):
            out.append(("x_boundary", _raw(2, x, (7, 8))))
    # limbs at and above p: the stored value plus p still fits 384 bits (2p < 2^382)
    pt = signed_points(g, 4)
    out.append(("x_plus_p", _raw(g, pt[2][0], pt[2][1], add_x=P)))
    out.append(("y_plus_p", _raw(g, pt[3][0], pt[3][1], add_y=P)))
    out.append(("both_plus_p", _raw(g, pt[1][0], pt[1][1], add_x=P, add_y=P)))
    out.append(("limbs_of_p", _raw(g, ei.f_zero(g), ei.f_zero(g), add_x=P, add_y=P)))
    out.append(("x_limbs_of_p", _raw(g, ei.f_zero(g), _small(g, 9), add_x=P)))
    out.append(("y_limbs_of_p", _raw(g, x5, ei.f_zero(g), add_y=P)))
    out.append(("y_half_plus_p", _raw(g, x5, ei.f_small(g, HALF + 1) if g == 1 else (0, HALF + 1), add_y=P)))
    # stored limbs that are a non-zero multiple of p: the value is zero, the sign flag is set
    xr = _raw(g, x5, ei.f_zero(g))[:48 * g]
    limbs = lambda *ls: b"".join(l.to_bytes(48, "little") for l in ls)  # noqa: E731
    if g == 1:
        out.append(("y_limbs_of_2p", xr + limbs(2 * P)))
        out.append(("y_limbs_of_9p", xr + limbs(9 * P)))
        out.append(("x_limbs_of_9p", limbs(9 * P) + limbs(_mont(3))))
    else:
        out.append(("y_im_limbs_of_p", xr + limbs(_mont(3), P)))
        out.append(("y_im_limbs_of_p_re_zero", xr + limbs(0, P)))
        out.append(("y_re_limbs_of_p", xr + limbs(P, 0)))
        out.append(("y_re_limbs_of_p", xr + limbs(9 * P, _mont(HALF))))
        out.append(("y_limbs_of_2p_p", xr + limbs(2 * P, P)))
        out.append(("x_limbs_of_9p", limbs(9 * P, 2 * P) + limbs(_mont(3), _mont(4))))
    return out


_AFFINE = {}


def affine_batch(g):
    if g not in _AFFINE:
        A = ei.AFF[g]
        inf = ("infinity", bytes(A))
        sp = _specials(g)
        run_at = 40  # nine in a row: a whole group of eight and one more, inside one wave
        n_good = SPECIAL_N - len(sp) - 2 - 9
        assert n_good >= 20, "more special cases than room"
        goods = [("good", ei.affine_bytes(g, pt)) for pt in signed_points(g, n_good)]
        body = []
        ns = len(sp)
        nb = SPECIAL_N - 2 - 9
        for i in range(nb):  # the special entries spread evenly between the good ones
            if (i + 1) * ns // nb > i * ns // nb:
                body.append(sp.pop(0))
            else:
                body.append(goods.pop(0))
        assert not sp and not goods
        out = [inf] + body[:run_at] + [inf] * 9 + body[run_at:] + [inf]
        assert len(out) == SPECIAL_N
        _AFFINE[g] = (b"".join(r for _, r in out), [nm for nm, _ in out])
    return _AFFINE[g]


_JAC = {}


def jacobian_batch(g):
    if g not in _JAC:
        pts = on_curve_finite(g, JAC_N)
        aff = b"".join(ei.affine_bytes(g, pt) for pt in pts)
        jac = ji.jacobians(g, aff, JAC_N, 0xe2c0de + g)
        names = ["random_z"] * JAC_N
        z1 = ji.affine_to_jacobian_z1(g, aff, JAC_N)
        J = ji.JAC[g]
        for i in (16, 17, 50, 63, 64, JAC_N - 2):  # Z = 1: no special path, the same bytes
            jac = jac[:i * J] + z1[i * J:(i + 1) * J] + jac[(i + 1) * J:]
            names[i] = "z_one"
        for i in [0, JAC_N - 1] + list(range(8, 16)):  # Z = 0, X and Y left as they were
            jac = ji.with_z(g, jac, i, bytes(48 * g))
            names[i] = "z_zero"
        _JAC[g] = (jac, names)
    return _JAC[g]


def jacobian_zero(g):
    aff = b"".join(ei.affine_bytes(g, pt) for pt in signed_points(g, JAC_ZERO_N))
    jac = ji.jacobians(g, aff, JAC_ZERO_N, 0x2e50 + g)
    for i in range(JAC_ZERO_N):
        jac = ji.with_z(g, jac, i, bytes(48 * g))
    return jac


def _f_inv(g, a):
    if g == 1:
        return pow(a, -1, P)
    n = pow((a[0] * a[0] + a[1] * a[1]) % P, -1, P)
    return (a[0] * n % P, -a[1] * n % P)


def jacobian_point(g, raw):
    """one blst Jacobian (Montgomery bytes) -> (x, y), or None when Z = 0"""
    co = 48 * g
    X, Y, Z = (ei.from_mont(g, raw[k * co:(k + 1) * co]) for k in range(3))
    if Z == ei.f_zero(g):
        return None
    zi = _f_inv(g, Z)
    zi2 = ei.f_mul(g, zi, zi)
    return (ei.f_mul(g, X, zi2), ei.f_mul(g, Y, ei.f_mul(g, zi2, zi)))


def affine_entry(g, raw, compressed):
    """One affine point as the reference encodes it.  enc_inputs.encode_point on the
    values mod p, but for the sign flag: the reference takes it from the Montgomery
    reduction of the stored y limbs before the last subtraction
    (sgn0_pty_mont_384[x]), and non-zero limbs that are a multiple of p reduce to p
    itself there -- non-zero and larger than (p - 1) / 2."""
    pt = ei.affine_point(g, raw)
    out = ei.encode_point(g, pt, compressed)
    if pt is None or not compressed:
        return out
    co = 48 * g
    ys = [int.from_bytes(raw[co + 48 * k:co + 48 * (k + 1)], "little") for k in range(g)]
    y = [P if (l and l % P == 0) else l * ei.RINV % P for l in ys]
    sign = ei.y_sign(g, y[0] if g == 1 else (y[0], y[1]))
    return bytes([(out[0] & 0xdf) | (0x20 if sign else 0)]) + out[1:]


def expected(g, raw, n, compressed, jacobian=False):
    raw = bytes(raw)
    if not jacobian:
        A = ei.AFF[g]
        return b"".join(affine_entry(g, raw[i * A:(i + 1) * A], compressed) for i in range(n))
    J = ji.JAC[g]
    return b"".join(ei.encode_point(g, jacobian_point(g, raw[i * J:(i + 1) * J]), compressed) for i in range(n))


FORMS = ("affine", "jacobian", "jacobian_zero")


def batch(g, form):
    """(raw source bytes, entries, is Jacobian) of a named batch"""
    if form == "affine":
        return affine_batch(g)[0], SPECIAL_N, False
    if form == "jacobian":
        return jacobian_batch(g)[0], JAC_N, True
    return jacobian_zero(g), JAC_ZERO_N, True
