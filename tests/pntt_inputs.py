"""Oracle and inputs of the NTT over group elements (msm_points_ntt / ps_ntt;
msm_points_ntt_model / ntt_model), shared by the CPU and GPU tests and by
tests/golden/make_points_ntt_golden.py.

A transform of points P_j = [a_j]G is the transform of the scalars a_j in Fr on
the generator: the expected result is [ntt(a)_k]G, with fr_inputs.ntt in plain
integers.  On the GPU both sides are multiples of the generator by ps_mult (pinned
to the reference by its own goldens); an a_j = 0 is an infinity input.
Test infrastructure only."""
import enc_inputs as ei
import fr_inputs as fi
import mult_inputs as mi

R = fi.R
GOLDEN_LOG_N = 3
GOLDEN_SEED = 2929


def brev(i, bits):
    return int(format(i, f"0{bits}b")[::-1], 2) if bits else 0


def ntt_scalars(a, log_n, batch=1, inverse=False, bitrev=False):
    """the scalars of the result of `batch` transforms under the flags of ps_ntt"""
    n = 1 << log_n
    assert len(a) == batch * n
    out = []
    for b in range(batch):
        x = a[b * n:(b + 1) * n]
        if bitrev and not inverse:  # the forward transform reads its element j at bitrev(j)
            x = [x[brev(j, log_n)] for j in range(n)]
        y = fi.ntt(x, inverse=inverse)
        if bitrev and inverse:  # the inverse writes result j at bitrev(j)
            y = [y[brev(q, log_n)] for q in range(n)]
        out += y
    return out


def golden_scalars():
    """the golden's a_j: random, one zero (an infinity input) and a one"""
    a = fi.rand_values(1 << GOLDEN_LOG_N, GOLDEN_SEED)
    a[3], a[6] = 0, 1
    return a


def gen_mults(m, group, ks):
    """[k]G for every k as affine bytes, by the library's fixed-base ps_mult"""
    if not ks:
        return b""
    return m.ps_mult(group, ei.affine_bytes(group, ei.GEN[group]), mi.scalar_bytes([k % R for k in ks]), len(ks),
                     one_point=True)


def point_at(data, group, i):
    s = ei.AFF[group]
    return data[s * i:s * (i + 1)]


def diff(got, want, group):
    """the indices at which two arrays of affine points differ"""
    s = ei.AFF[group]
    return [i for i in range(max(len(got), len(want)) // s) if got[s * i:s * i + s] != want[s * i:s * i + s]]
