"""Jacobian inputs with a known affine form, in plain Python integers (no
library arithmetic), shared by the bulk to-affine tests and the golden script.

From n affine points (blst Montgomery layout, R = 2^384; e.g.
msm_blst_amd.fixed_points(group, n)) and SplitMix64 values lambda_i != 0 (in
Fp for G1, in Fp2 for G2) it builds the Jacobians
    (X', Y', Z') = (x lambda^2, y lambda^3, lambda)
in the same layout: with x_mont = x R the stored X' is x_mont lambda^2 mod p
(Montgomery form is linear in the value) and the stored Z' is lambda R mod p.
The affine form of every such point is the input affine point itself, byte for
byte (canonical coordinates are unique), so the expected output of a
to-affine routine is known without the code under test and without the
reference.
"""
P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R384 = (1 << 384) % P
M64 = (1 << 64) - 1
AFF = {1: 96, 2: 192}
JAC = {1: 144, 2: 288}


class SplitMix64:
    def __init__(self, seed):
        self.s = seed & M64

    def next(self):
        self.s = (self.s + 0x9e3779b97f4a7c15) & M64
        z = self.s
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
        return z ^ (z >> 31)

    def fp(self):
        v = 0
        for k in range(6):
            v |= self.next() << (64 * k)
        return v % P


def _mul(g, a, b):
    """product in Fp (g = 1, ints) or Fp2 = Fp[i]/(i^2 + 1) (g = 2, pairs)"""
    if g == 1:
        return a * b % P
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def _load(g, raw, off):
    c = [int.from_bytes(raw[off + 48 * k:off + 48 * (k + 1)], "little") for k in range(g)]
    return c[0] if g == 1 else tuple(c)


def _store(g, v):
    if g == 1:
        return v.to_bytes(48, "little")
    return v[0].to_bytes(48, "little") + v[1].to_bytes(48, "little")


def lambdas(group, n, seed):
    """n nonzero field elements (plain values, not Montgomery)"""
    rng = SplitMix64(seed)
    out = []
    while len(out) < n:
        v = rng.fp() if group == 1 else (rng.fp(), rng.fp())
        if v != 0 and v != (0, 0):
            out.append(v)
    return out


def jacobians(group, affine, n, seed):
    """bytes of n blst_p1 / blst_p2 Jacobians whose affine forms are affine[:n]"""
    raw = bytes(affine)
    assert len(raw) >= n * AFF[group]
    out = bytearray()
    co = 48 * group  # bytes per coordinate
    for i, lam in enumerate(lambdas(group, n, seed)):
        x = _load(group, raw, i * AFF[group])
        y = _load(group, raw, i * AFF[group] + co)
        l2 = _mul(group, lam, lam)
        l3 = _mul(group, l2, lam)
        z = lam * R384 % P if group == 1 else (lam[0] * R384 % P, lam[1] * R384 % P)
        out += _store(group, _mul(group, x, l2)) + _store(group, _mul(group, y, l3)) + _store(group, z)
    return bytes(out)


def with_z(group, jac, index, z_mont_bytes):
    """jac with the stored Z of point `index` replaced (X, Y untouched)"""
    co = 48 * group
    off = index * JAC[group] + 2 * co
    assert len(z_mont_bytes) == co
    return jac[:off] + z_mont_bytes + jac[off + co:]


def affine_to_jacobian_z1(group, affine, n):
    """the same points as Jacobians with Z = 1 (stored R mod p)"""
    raw = bytes(affine)
    one = R384.to_bytes(48, "little") + (b"\0" * 48 if group == 2 else b"")
    return b"".join(raw[i * AFF[group]:(i + 1) * AFF[group]] + one for i in range(n))


def fnv(data):
    h = 1469598103934665603
    for b in data:
        h ^= b
        h = (h * 1099511628211) & M64
    return f"{h:016x}"
