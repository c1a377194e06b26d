"""GPU checks of the single-chain Montgomery columns (fp.hpp MulChain), G1.

  msm_fp_form_ops   probe.hip k_form_ops: one fp_mul, fp_sqr, fp_mul2, xyzz_madd
                    and xyzz_add per lane, compiled once with the split columns
                    and once with the single chain.  Both must write the same
                    bytes on 256 lanes (the same sums in another order), and the
                    three products must be the Montgomery products of the inputs.
  the library as built (the G1 accumulation takes the single-chain madd, kernels.hpp
  MSM_ACC_CHAIN; the segment sums keep the split add, ches_kernels.hpp MSM_SEGSUM_CHAIN):
    CHESContext.mult / MSMContext.mult   one CHES and one plain Pippenger MSM at
                    n = 2^10 against the reference's golden value
    ps_sum_segments segments of 1, 2, 8 and 9 points, a doubled first pair and a
                    sum through infinity (the index lists and oracle sums of
                    tests/test_gpu_xyzz_add.py, computed once there)
"""
import ctypes
import random

import pytest

from test_gpu_xyzz_add import SEGMENTS, case

pytestmark = pytest.mark.gpu

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
NL = 14
M28 = (1 << 28) - 1
RINV = pow(1 << 392, -1, P)
LANES = 256


@pytest.fixture(scope="module")
def m():
    import msm_blst_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible")
    return m


def _val(w):
    return sum(int(x) << (28 * i) for i, x in enumerate(w))


def _form_ops(m, form, words):
    L = m.lib()
    L.msm_fp_form_ops.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.msm_fp_form_ops.restype = ctypes.c_int
    inp = (ctypes.c_uint32 * len(words))(*words)
    out = (ctypes.c_uint32 * (LANES * 11 * NL))()
    assert L.msm_fp_form_ops(0, form, inp, LANES, out) == 0, L.msm_last_error()
    return list(out)


def test_per_op_kernels_identical_bytes(m):
    rnd = random.Random(2501)
    words = []
    for lane in range(LANES):
        for k in range(8):
            # normalized limbs; top limb below 2^16: canonical (< p), so a legal affine row,
            # xyzz coordinate (class S, x in class X) and product operand alike
            words += [rnd.randrange(1 << 28) for _ in range(NL - 1)] + [rnd.randrange(1 << 16)]
    # lane 0: zero and one as product operands; lane 1: an xyzz point at infinity (ZZ = 0)
    words[0:NL] = [0] * NL
    words[NL:2 * NL] = [1] + [0] * (NL - 1)
    base = 1 * 8 * NL
    words[base + 3 * NL:base + 4 * NL] = [0] * NL
    split, chain = _form_ops(m, 0, words), _form_ops(m, 1, words)
    assert split == chain
    assert any(chain)
    for lane in range(0, LANES, 17):
        a = [_val(words[(lane * 8 + k) * NL:(lane * 8 + k + 1) * NL]) for k in range(4)]
        o = [_val(chain[(lane * 11 + k) * NL:(lane * 11 + k + 1) * NL]) for k in range(3)]
        assert o[0] % P == a[0] * a[1] * RINV % P
        assert o[1] % P == a[0] * a[0] * RINV % P
        assert o[2] % P == (a[0] * a[1] + a[2] * a[3]) * RINV % P
        assert all(x < 2 * P for x in o)
    L = m.lib()
    assert L.msm_fp_form_ops(0, 2, (ctypes.c_uint32 * 1)(), 1, (ctypes.c_uint32 * 1)()) != 0


def test_msms_n10_against_golden(m, golden, points):
    n = 1024
    want = {c["seed"]: c["compressed"] for c in golden("msm_g1.json")["cases"]
            if c["n"] == n and c["case"] == "rand" and c["nbits"] == 255}
    assert set(want) >= {1, 2}
    pts = points(1, n)
    ches = m.CHESContext(1, 0, n_exp=10)
    try:
        ches.build_table(pts, n)
        for seed in (1, 2):
            assert m.compress(1, ches.mult(m.gen_scalars(n, seed))).hex() == want[seed], seed
    finally:
        ches.close()
    pip = m.MSMContext(1, 0, 10)
    try:
        pip.set_points(pts, n)
        for seed in (1, 2):
            assert m.compress(1, pip.mult(m.gen_scalars(n, seed), 255)).hex() == want[seed], seed
    finally:
        pip.close()


@pytest.mark.parametrize("piece", [None, "8"])
def test_segment_sums(m, piece, monkeypatch):
    monkeypatch.delenv("MSM_POINTS_SEGMENTS_CHUNK", raising=False)
    if piece is None:
        monkeypatch.delenv("MSM_POINTS_SEGMENTS_PIECE", raising=False)
    else:
        monkeypatch.setenv("MSM_POINTS_SEGMENTS_PIECE", piece)
    c = case(m, 1)
    assert [len(s) for s in SEGMENTS[:4]] == [1, 2, 8, 9] and SEGMENTS[4][0] == SEGMENTS[4][1]
    offsets = [0]
    for s in c["segs"]:
        offsets.append(offsets[-1] + len(s))
    got = m.ps_sum_segments(1, b"".join(e for s in c["segs"] for e in s), offsets)
    bad = [j for j in range(len(SEGMENTS)) if got[j * 96:(j + 1) * 96] != c["aff"][j]]
    assert not bad, f"differing segments {bad}"
    assert not any(got[7 * 96:8 * 96]) and any(got[5 * 96:6 * 96])  # P - P + Q + R is not infinity, P - P is
