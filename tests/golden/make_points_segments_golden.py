#!/usr/bin/env python3
"""Golden fixture for the segmented sums and MSMs (a loop over the reference's MSM /
bulk addition per point set), written from the REFERENCE itself:
oracle/_ref/libblst_ref.so (built by oracle/Makefile) is called through ctypes, one
point at a time -- blst_p{1,2}_from_affine, blst_p{1,2}_mult, then
blst_p{1,2}_add_or_double into the running sum of the segment, and
blst_p{1,2}_to_affine at its end.  Runs only in the build container, on the CPU.

Writes tests/golden/points_segments.json: per group, for the batch
seg_inputs.golden_batch(group) (nbits 255), the indices of the segments whose points
all lie in the subgroup, the compressed sum of each, and the FNV-1a 64 of their
affine sums in order.  The segment with a point of small order is left out: the
reference's multiplication is not to be trusted there (make_points_mult_golden.py);
its expected value comes from seg_inputs.expected alone.  While writing, the script
asserts that seg_inputs.expected agrees with the reference on every recorded segment.
Test infrastructure only; data, no reference source text.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))

import enc_inputs as ei  # noqa: E402
import seg_inputs as si  # noqa: E402

vp = ctypes.c_void_p


def ref_segment(L, g, pts, ks, nbits):
    """the reference's sum of [k_i] P_i as affine bytes (infinity: all zero)"""
    A, J = ei.AFF[g], 144 * g
    for name in ("from_affine", "to_affine"):
        getattr(L, f"blst_p{g}_{name}").argtypes = [vp, vp]
        getattr(L, f"blst_p{g}_{name}").restype = None
    mult = getattr(L, f"blst_p{g}_mult")
    mult.argtypes = [vp, vp, vp, ctypes.c_size_t]
    mult.restype = None
    add = getattr(L, f"blst_p{g}_add_or_double")
    add.argtypes = [vp, vp, vp]
    add.restype = None
    acc = (ctypes.c_uint8 * J)()  # Z = 0: infinity
    for pt, k in zip(pts, ks):
        if pt is None:
            continue
        a = (ctypes.c_uint8 * A).from_buffer_copy(ei.affine_bytes(g, pt))
        j, t = (ctypes.c_uint8 * J)(), (ctypes.c_uint8 * J)()
        sc = (ctypes.c_uint8 * 32).from_buffer_copy(k.to_bytes(32, "little"))
        getattr(L, f"blst_p{g}_from_affine")(j, a)
        mult(t, j, sc, nbits)
        add(acc, acc, t)
    if not any(bytes(acc)[2 * (J // 3):]):  # Z == 0
        return bytes(A)
    res = (ctypes.c_uint8 * A)()
    getattr(L, f"blst_p{g}_to_affine")(res, acc)
    return bytes(res)


def main():
    L = ctypes.CDLL(os.path.join(REPO, "oracle", "_ref", "libblst_ref.so"))
    cases = []
    for g in (1, 2):
        A = ei.AFF[g]
        pts, ks, o, ing = si.golden_batch(g)
        want = si.expected(g, pts, ks, o)
        idx = [j for j in range(len(o) - 1) if ing[j]]
        outs = []
        for j in idx:
            r = ref_segment(L, g, pts[o[j]:o[j + 1]], ks[o[j]:o[j + 1]], si.GOLDEN_NBITS)
            assert r == want[j * A:(j + 1) * A], (g, j, "seg_inputs.expected differs from the reference")
            outs.append(r)
        cases.append({"group": g, "nbits": si.GOLDEN_NBITS, "lengths": si.GOLDEN_LENGTHS, "in_group": idx,
                      "compressed": [ei.encode_point(g, ei.affine_point(g, r), True).hex() for r in outs],
                      "fnv": ei.fnv(b"".join(outs))})
        print({k: v for k, v in cases[-1].items() if k != "compressed"}, flush=True)
    with open(os.path.join(HERE, "points_segments.json"), "w") as f:
        json.dump({"source": "reference libblst (oracle/_ref/libblst_ref.so) blst_p{1,2}_from_affine + blst_p{1,2}_mult + "
                             "blst_p{1,2}_add_or_double + blst_p{1,2}_to_affine, one point at a time, on the segments of "
                             "tests/seg_inputs.py golden_batch(group) whose points all lie in the subgroup; fnv = FNV-1a 64 "
                             "of the affine sums, infinity as the all-zero point",
                   "segments": cases}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
