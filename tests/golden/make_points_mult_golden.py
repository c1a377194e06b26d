#!/usr/bin/env python3
"""Golden fixture for the bulk scalar multiplication (a loop over ref
src/e1.c:505-533 blst_p1_mult, src/e2.c, src/ec_mult.h), written from the
REFERENCE itself: oracle/_ref/libblst_ref.so (built by oracle/Makefile) is called
through ctypes -- blst_p{1,2}_from_affine, blst_p{1,2}_mult, blst_p{1,2}_to_affine,
one point at a time.  Runs only in the build container, on the CPU.

Writes tests/golden/points_mult.json:
  special   per group and nbits (255, 256), for the in-group entries of
            mult_inputs.special_batch: their indices, the compressed result of
            each, and the FNV-1a 64 of their affine results in order
  bulk      per group, n = 1000 at nbits = 255 with gen_scalars(1000, 1): the FNV of
            the affine results on the fixed points 2^(i+1) G, and of the one-point
            twin on the generator
The entries on points of small order are left out: the reference builds its
table with an addition that does not know doubling (ec_mult.h:89-92), so its
answers there are not to be trusted; their expected values come from
mult_inputs.smul alone.  While writing, the script asserts that smul agrees with
the reference on every in-group entry.
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
import mult_inputs as mi  # noqa: E402


def ref_mult(L, g, affine, k, nbits):
    """the reference's [k]P as affine bytes (infinity: all zero, as this library writes it)"""
    A, J = ei.AFF[g], 144 * g
    if not any(affine):
        return bytes(A)
    for name in ("from_affine", "to_affine"):
        getattr(L, f"blst_p{g}_{name}").argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        getattr(L, f"blst_p{g}_{name}").restype = None
    mult = getattr(L, f"blst_p{g}_mult")
    mult.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    mult.restype = None
    a = (ctypes.c_uint8 * A).from_buffer_copy(affine)
    j, out = (ctypes.c_uint8 * J)(), (ctypes.c_uint8 * J)()
    sc = (ctypes.c_uint8 * 32).from_buffer_copy(k.to_bytes(32, "little"))
    res = (ctypes.c_uint8 * A)()
    getattr(L, f"blst_p{g}_from_affine")(j, a)
    mult(out, j, sc, nbits)
    if not any(bytes(out)[2 * (J // 3):]):  # Z == 0
        return bytes(A)
    getattr(L, f"blst_p{g}_to_affine")(res, out)
    return bytes(res)


def main():
    L = ctypes.CDLL(os.path.join(REPO, "oracle", "_ref", "libblst_ref.so"))
    special, bulk = [], []
    for g in (1, 2):
        A = ei.AFF[g]
        for nbits in (255, 256):
            names, pts, ks, ing, exp = mi.expected_batch(g, nbits)
            idx = [i for i in range(len(ks)) if ing[i]]
            outs = []
            for i in idx:
                r = ref_mult(L, g, ei.affine_bytes(g, pts[i]), ks[i], nbits)
                assert r == exp[i], (g, nbits, i, names[i], "smul differs from the reference")
                outs.append(r)
            special.append({"group": g, "nbits": nbits, "n": len(ks), "in_group": idx,
                            "compressed": [ei.encode_point(g, ei.affine_point(g, r), True).hex() for r in outs],
                            "fnv": ei.fnv(b"".join(outs))})
            print({k: v for k, v in special[-1].items() if k not in ("in_group", "compressed")}, len(idx), flush=True)
        n = 1000
        ks = mi.gen_scalars(n, 1)
        fixed = ei.fixed_points(g, n)
        per = b"".join(ref_mult(L, g, ei.affine_bytes(g, fixed[i]), ks[i], 255) for i in range(n))
        one = b"".join(ref_mult(L, g, ei.affine_bytes(g, ei.GEN[g]), ks[i], 255) for i in range(n))
        for i in (0, 1, 499, 999):  # (smul on all 2000 would take minutes for nothing: the special batch covers it)
            assert per[i * A:(i + 1) * A] == ei.affine_bytes(g, mi.smul(g, fixed[i], ks[i]))
            assert one[i * A:(i + 1) * A] == ei.affine_bytes(g, mi.smul(g, ei.GEN[g], ks[i]))
        bulk.append({"group": g, "n": n, "nbits": 255, "seed": 1, "fnv": ei.fnv(per), "fnv_one_point": ei.fnv(one)})
        print(bulk[-1], flush=True)
    with open(os.path.join(HERE, "points_mult.json"), "w") as f:
        json.dump({"source": "reference libblst (oracle/_ref/libblst_ref.so) blst_p{1,2}_from_affine + blst_p{1,2}_mult + "
                             "blst_p{1,2}_to_affine, one point at a time, on the in-group entries of "
                             "tests/mult_inputs.py special_batch(group, nbits) and on n fixed points 2^(i+1) G (one-point "
                             "twin: the generator) with the SplitMix64 scalars of seed 1; fnv = FNV-1a 64 of the affine "
                             "results, infinity as the all-zero point",
                   "special": special, "bulk": bulk}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
