"""Plain-Python oracle of the Fr layer (msm_fr_op, msm_fr_ntt): the two byte forms,
the elementwise ops, an iterative radix-2 NTT, coset shifts and the inputs the CPU
and GPU tests share.  tests/golden/fr_ops.json pins it to the reference.
Test infrastructure only."""
import mult_inputs as mi

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
MONT = 1 << 256
MONT_INV = pow(MONT, -1, R)
OMEGA = pow(7, (R - 1) >> 32, R)  # order 2^32
assert OMEGA == 0x16a2a19edfe81f20d09b681922c813b4b63683508c2280b93829971f439f0d2b
assert pow(OMEGA, 1 << 31, R) == R - 1
OPS = ("add", "sub", "mul", "sqr", "neg", "inv", "from_scalar", "to_scalar")
BINARY = ("add", "sub", "mul")
SEED = 2718  # of the SplitMix64 values among the special ones


# ---- the two byte forms ----
def fr_bytes(a):
    """blst_fr of a: four little-endian 64-bit limbs of a 2^256 mod r"""
    return (a % R * MONT % R).to_bytes(32, "little")


def fr_int(b):
    return int.from_bytes(b, "little") * MONT_INV % R


def scalar_bytes(a):
    return a.to_bytes(32, "little")


def pack(vals, scalar=False):
    return b"".join(scalar_bytes(v) if scalar else fr_bytes(v) for v in vals)


def unpack(data, scalar=False):
    out = []
    for i in range(0, len(data), 32):
        out.append(int.from_bytes(data[i:i + 32], "little") if scalar else fr_int(data[i:i + 32]))
    return out


# ---- elementwise (on blst bytes, as the reference's calls) ----
def op_bytes(op, a, b=None):
    """what blst_fr_<op> gives for the blst_fr bytes a (and b); from_scalar takes a
    blst_scalar, to_scalar gives one"""
    if op == "from_scalar":
        return fr_bytes(int.from_bytes(a, "little"))
    x = fr_int(a)
    if op == "to_scalar":
        return scalar_bytes(x)
    y = fr_int(b) if op in BINARY else None
    v = {"add": lambda: x + y, "sub": lambda: x - y, "mul": lambda: x * y, "sqr": lambda: x * x,
         "neg": lambda: -x, "inv": lambda: pow(x, R - 2, R)}[op]()
    return fr_bytes(v % R)


def special_values():
    vals = [0, 1, 2, R - 1, R - 2, (R + 1) // 2, (R - 1) // 2, 1 << 32, (1 << 255) % R, (1 << 256) % R,
            OMEGA, pow(OMEGA, -1, R), 7]
    return vals + mi.gen_scalars(3, SEED)


def rand_values(n, seed):
    return mi.gen_scalars(n, seed)


# ---- transforms ----
def root(log_n):
    return pow(OMEGA, 1 << (32 - log_n), R)


def ntt(x, inverse=False, shift=None):
    """natural order in and out; forward: X[k] = sum_j (s^j x[j]) w^(jk); inverse: x[j]
    = s^-j n^-1 sum_k X[k] w^(-jk)"""
    n = len(x)
    log_n = n.bit_length() - 1
    assert 1 << log_n == n
    w = root(log_n)
    if inverse:
        w = pow(w, -1, R)
    a = list(x)
    if shift is not None and not inverse:
        p = 1
        for j in range(n):
            a[j] = a[j] * p % R
            p = p * shift % R
    # bit reversal, then decimation in time
    j = 0
    for i in range(1, n):
        bit = n >> 1
        while j & bit:
            j ^= bit
            bit >>= 1
        j |= bit
        if i < j:
            a[i], a[j] = a[j], a[i]
    length = 2
    while length <= n:
        wl = pow(w, n // length, R)
        for i in range(0, n, length):
            t = 1
            for k in range(length // 2):
                u, v = a[i + k], a[i + k + length // 2] * t % R
                a[i + k], a[i + k + length // 2] = (u + v) % R, (u - v) % R
                t = t * wl % R
        length <<= 1
    if inverse:
        ninv = pow(n, -1, R)
        sinv = pow(shift, -1, R) if shift is not None else 1
        p = ninv
        for j in range(n):
            a[j] = a[j] * p % R
            p = p * sinv % R
    return a


def ntt_slow(x):
    """the O(n^2) sum, as the golden generator runs it on the reference"""
    n = len(x)
    w = root(n.bit_length() - 1)
    return [sum(x[j] * pow(w, j * k, R) for j in range(n)) % R for k in range(n)]


def ntt_batch(vals, log_n, batch, **kw):
    n = 1 << log_n
    out = []
    for b in range(batch):
        out += ntt(vals[b * n:(b + 1) * n], **kw)
    return out


NTT_HASH_SEED = 31  # the 2^10 inputs whose forward transform the golden hashes
