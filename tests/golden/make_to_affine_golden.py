#!/usr/bin/env python3
"""Golden fixture for the bulk Jacobian -> affine normalisation (ref
src/multi_scalar.c:17-62), written from the REFERENCE itself:
oracle/_ref/libblst_ref.so (built by oracle/Makefile) is called through ctypes
-- blst_p{1,2}s_to_affine on the Jacobians tests/jac_inputs.py builds from the
reference's own fixed points (P_i = 2^(i+1) G via blst_p{1,2}_double +
blst_p{1,2}_to_affine).  Runs only in the build container, on the CPU.

Writes tests/golden/to_affine.json: per case {group, n, seed, fnv} with fnv the
FNV-1a 64 of the reference's output bytes.  The sizes cross the reference's
shared-inversion stride (1536 points for G1, 768 for G2).  Finite points only
(a Z = 0 input corrupts the reference's whole stride, its comment at
multi_scalar.c:14-16).  While writing, the script asserts that the reference's
output equals the affine points the Jacobians were built from.
Test infrastructure only; data, no reference source text.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))

import jac_inputs as ji  # noqa: E402

CASES = [(1, 1000, 11), (1, 4099, 12), (2, 500, 13), (2, 1000, 14)]  # (group, n, seed)


def ref_fixed_points(L, group, n):
    g = f"p{group}"
    aff, jac = ji.AFF[group], ji.JAC[group]
    gen = getattr(L, f"blst_{g}_generator")
    gen.restype = ctypes.c_void_p
    dbl = getattr(L, f"blst_{g}_double")
    to_aff = getattr(L, f"blst_{g}_to_affine")
    acc = (ctypes.c_uint8 * jac).from_buffer_copy(ctypes.string_at(gen(), jac))
    pts = (ctypes.c_uint8 * (aff * n))()
    for i in range(n):
        dbl(acc, acc)
        to_aff(ctypes.byref(pts, i * aff), acc)
    return bytes(pts)


def ref_ps_to_affine(L, group, jac, n):
    f = getattr(L, f"blst_p{group}s_to_affine")
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    f.restype = None
    src = (ctypes.c_uint8 * len(jac)).from_buffer_copy(jac)
    dst = (ctypes.c_uint8 * (ji.AFF[group] * n))()
    pp = (ctypes.c_void_p * 2)(ctypes.cast(src, ctypes.c_void_p), None)
    f(dst, pp, n)
    return bytes(dst)


def main():
    L = ctypes.CDLL(os.path.join(REPO, "oracle", "_ref", "libblst_ref.so"))
    cases = []
    for group, n, seed in CASES:
        aff = ref_fixed_points(L, group, n)
        out = ref_ps_to_affine(L, group, ji.jacobians(group, aff, n, seed), n)
        assert out == aff, f"reference output differs from the input affine points (G{group} n={n})"
        cases.append({"group": group, "n": n, "seed": seed, "fnv": ji.fnv(out)})
        print(cases[-1], flush=True)
    with open(os.path.join(HERE, "to_affine.json"), "w") as f:
        json.dump({"source": "reference libblst (oracle/_ref/libblst_ref.so) blst_p{1,2}s_to_affine on the Jacobians "
                             "(x l^2, y l^3, l) of tests/jac_inputs.py: points 2^(i+1) G, SplitMix64 l from seed; "
                             "fnv = FNV-1a 64 of the output bytes (equal to the input affine points)",
                   "cases": cases}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
