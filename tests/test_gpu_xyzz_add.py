"""GPU parity of the regrouped general add (ec.hpp xyzz_add) through the entry
points whose reductions are made of it, G1 and G2, at the smallest shapes that
reach every path:

  ps_sum_segments   point_segments.hip: with a few dozen points every point is its
                    own piece, so every segment is summed by the pairwise merge tree
                    of xyzz_add alone; at a piece of 8 the pieces are summed by
                    xyzz_madd and a segment of 9 is one merge of two partials
  ps_add            blst_p{1,2}s_add: one point per bucket of weight 1, summed by the
                    weighted reducer (k_segsum level 0 in chunks of <= 8, then the
                    tails)
  CHESContext.mult  one MSM at n = 2^10 per group against the reference's golden
                    value: the bucket plan (top-digit copies) and its reduction

The points come from an index list into 24 fixed points: segments of 1, 2, 8 and
9 (a level-0 chunk and a piece hold <= 8, so 9 crosses into a second one), a
segment whose first two entries are equal (the doubling branch), one that sums
to infinity and then continues, one that holds infinity entries, and one that
cancels.  Every result is compared with the oracle's canonical encoding
(oracle/msm_oracle.c: the naive sum, made affine or compressed).
"""
import ctypes

import pytest

import oracle_ffi as of

pytestmark = pytest.mark.gpu

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
# k > 0: fixed point k - 1, k < 0: its negative, 0: infinity (the all-zero affine point)
SEGMENTS = [
    [1],
    [2, 3],
    [4, 5, 6, 7, 8, 9, 10, 11],
    [12, 13, 14, 15, 16, 17, 18, 19, 20],
    [21, 21, 22],                 # the first two entries equal: P + P
    [6, -6, 7, 8],                # infinity, then the sum goes on
    [0, 9, 0, 0, 10],             # infinity entries first, inside and side by side
    [5, -5],                      # the result is infinity
]
_CACHE = {}


@pytest.fixture(scope="module")
def m():
    import msm_blst_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device visible")
    return m


def _neg(group, pt):
    """-P of an affine point in the 6 x 64-bit Montgomery layout (x | y; G2: c0 | c1 each)"""
    h = len(pt) // 2
    y = b"".join(((P - int.from_bytes(pt[h + o:h + o + 48], "little")) % P).to_bytes(48, "little")
                 for o in range(0, h, 48))
    return pt[:h] + y


def _entry(group, base, k):
    A = 96 * group
    if k == 0:
        return bytes(A)
    pt = base[(abs(k) - 1) * A:abs(k) * A]
    return pt if k > 0 else _neg(group, pt)


def _oracle_sum(group, entries):
    """the oracle's sum of these affine points as a Jacobian point (infinity entries left out)"""
    pts = b"".join(e for e in entries if any(e))
    n = len(pts) // (96 * group)
    ones = b"".join((1).to_bytes(32, "little") for _ in range(n))
    Pb = (ctypes.c_uint8 * max(len(pts), 1)).from_buffer_copy(pts or b"\0")
    Sb = (ctypes.c_uint8 * max(len(ones), 1)).from_buffer_copy(ones or b"\0")
    return of.msm(group, Pb, Sb, n, 255, "naive")


def case(m, group):
    """entries and the oracle's answers per segment; computed once, never modified"""
    if group not in _CACHE:
        base = bytes(m.fixed_points(group, 24))
        segs = [[_entry(group, base, k) for k in s] for s in SEGMENTS]
        jac = [_oracle_sum(group, s) for s in segs]
        aff = []
        for j in jac:
            out = of.buf(96 * group)
            getattr(of.lib(), f"or_p{group}_to_affine")(out, j)
            aff.append(bytes(out))
        whole = _oracle_sum(group, [e for s in segs for e in s])
        _CACHE[group] = {"segs": segs, "aff": aff, "cmp": [of.compress(group, j) for j in jac],
                         "whole": of.compress(group, whole)}
    return _CACHE[group]


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("piece", [None, "8"])
def test_segment_sums_every_branch(m, group, piece, monkeypatch):
    monkeypatch.delenv("MSM_POINTS_SEGMENTS_CHUNK", raising=False)
    if piece is None:
        monkeypatch.delenv("MSM_POINTS_SEGMENTS_PIECE", raising=False)
    else:
        monkeypatch.setenv("MSM_POINTS_SEGMENTS_PIECE", piece)
    c = case(m, group)
    A = 96 * group
    offsets = [0]
    for s in c["segs"]:
        offsets.append(offsets[-1] + len(s))
    if piece is None:  # every point its own piece: the sums are xyzz_add merges only
        assert len(m.segments_plan(offsets, 1)) == offsets[-1]
    got = m.ps_sum_segments(group, b"".join(e for s in c["segs"] for e in s), offsets)
    bad = [j for j in range(len(SEGMENTS)) if got[j * A:(j + 1) * A] != c["aff"][j]]
    assert not bad, f"differing segments {bad}"
    assert not any(got[7 * A:8 * A]) and any(got[5 * A:6 * A])   # P - P is the all-zero point; P - P + Q + R is not


@pytest.mark.parametrize("group", [1, 2])
def test_bulk_sums_every_branch(m, group):
    """the same index lists through blst_p{1,2}s_add, one list per call, then all 34
    points in one call (five level-0 chunks and the levels above them)"""
    c = case(m, group)
    for j, s in enumerate(c["segs"]):
        got = m.ps_add(group, b"".join(s), len(s))
        assert m.compress(group, got).hex() == c["cmp"][j], j
    flat = [e for s in c["segs"] for e in s]
    assert len(flat) == 34
    assert m.compress(group, m.ps_add(group, b"".join(flat), len(flat))).hex() == c["whole"]


@pytest.mark.parametrize("group", [1, 2])
def test_ches_n10_against_golden(m, group, golden, points):
    n = 1024
    want = {c["seed"]: c["compressed"] for c in golden(f"msm_g{group}.json")["cases"]
            if c["n"] == n and c["case"] == "rand" and c["nbits"] == 255}
    assert set(want) >= {1, 2}
    ctx = m.CHESContext(group, 0, n_exp=10)
    try:
        ctx.build_table(points(group, n), n)
        for seed in (1, 2):
            assert m.compress(group, ctx.mult(m.gen_scalars(n, seed))).hex() == want[seed], seed
    finally:
        ctx.close()
