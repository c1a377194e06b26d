"""Inputs and expected values for the segmented sums and MSMs
out[j] = sum_{o[j] <= i < o[j+1]} [k_i] P_i (msm_points_msm_segments), in plain Python
integers, shared by the points-segments tests and
tests/golden/make_points_segments_golden.py.  Builds on mult_inputs.py (smul) and
the Jacobian addition of enc_inputs.py.

  offsets_of(lengths, first=0)      the offsets of segments of these lengths
  segment_sum(g, pts, ks)           sum [k_i] P_i as (x, y) or None; ks None: every k_i = 1
  expected(g, pts, ks, offsets)     the affine bytes of every segment (infinity: all zero)
  neg(g, pt)                        -pt
  batch(g, n, seed, nbits)          n fixed points 2^(i+1) G with SplitMix64 scalars cut to nbits
  golden_batch(g)                   the batch of tests/golden/points_segments.json
  pieces(offsets, L)                the cut the host plan must make, in plain Python
"""
import enc_inputs as ei
import mult_inputs as mi

EDGE_LENGTHS = [0, 1, 0, 2, 3, 7, 8, 9, 17, 0]  # around a piece of 8, empty segments first, inside and last
_SMUL = {}


def offsets_of(lengths, first=0):
    o = [first]
    for n in lengths:
        o.append(o[-1] + n)
    return o


def neg(g, pt):
    return None if pt is None else (pt[0], ei.f_neg(g, pt[1]))


def _smul(g, pt, k):
    key = (g, pt, k)
    if key not in _SMUL:
        _SMUL[key] = mi.smul(g, pt, k)
    return _SMUL[key]


def segment_sum(g, pts, ks=None):
    acc = (ei.f_small(g, 1), ei.f_small(g, 1), ei.f_zero(g))
    for i, pt in enumerate(pts):
        q = pt if ks is None else _smul(g, pt, ks[i])
        if q is not None:
            acc = ei._jadd_affine(g, acc, q)
    return mi._to_affine(g, acc)


def expected(g, pts, ks, offsets):
    return b"".join(ei.affine_bytes(g, segment_sum(g, pts[a:b], None if ks is None else ks[a:b]))
                    for a, b in zip(offsets, offsets[1:]))


def batch(g, n, seed, nbits=64):
    return ei.fixed_points(g, n), [k & ((1 << nbits) - 1) for k in mi.gen_scalars(n, seed)]


GOLDEN_LENGTHS = [0, 1, 0, 2, 3, 7, 8, 9, 2, 5]
GOLDEN_NBITS = 255


def golden_batch(g):
    """(points, scalars, offsets, in_group flag per segment): fixed points and the
    generator with 255-bit scalars, an infinity input, scalars 0, 1 and r - 1, a
    pair that cancels, and one segment with a point outside the subgroup (not
    recorded: the reference's answer there is not to be trusted)"""
    o = offsets_of(GOLDEN_LENGTHS)
    n = o[-1]
    pts, ks = batch(g, n, 31, GOLDEN_NBITS)
    pts = list(pts)
    pts[3] = ei.GEN[g]
    pts[5] = None          # infinity inside the segment of 3
    ks[6], ks[7], ks[8] = 0, 1, mi.R - 1
    pts[14] = pts[13]      # [k]P + [r - k]P inside the segment of 8
    ks[14] = mi.R - ks[13]
    q, t = mi.small_order_points(g)[0]
    pts[o[8]] = t
    ing = [True] * len(GOLDEN_LENGTHS)
    ing[8] = False
    return pts, ks, o, ing


def pieces(offsets, L):
    out = []
    for j, (a, b) in enumerate(zip(offsets, offsets[1:])):
        for s in range(a, b, L):
            out.append((s, min(L, b - s), j))
    return out
