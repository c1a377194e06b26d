#!/usr/bin/env python3
"""Golden fixture for the KZG layer (msm_kzg_*), written from the REFERENCE itself:
oracle/_ref/libblst_ref.so (built by oracle/Makefile) is called through ctypes --
blst_p{1,2}_from_affine, blst_p{1,2}_mult on the generators, blst_p{1,2}_to_affine.
Runs only in the build container, on the CPU.

Writes tests/golden/kzg.json, for n = 16 in natural order with kzg_inputs.TAU and
the polynomials and points of kzg_inputs.golden_polys() / golden_points():
  srs          the 16 points [l_i(tau)]G1, compressed
  tau_g2       [tau]G2, compressed
  commitments  [f_j(tau)]G1 of the 3 polynomials, compressed
  openings     per polynomial and point: z, y (hex integers) and the proof
               [(f_j(tau) - y) / (tau - z)]G1, compressed
The scalars come from the Python oracle (tests/kzg_inputs.py); every point is the
reference's multiple of the generator, and the script asserts that the oracle's own
scalar multiplication agrees while writing.
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
import kzg_inputs as ki  # noqa: E402


def ref_gen_mult(L, g, k):
    """the reference's [k]G as affine bytes (infinity: all zero)"""
    A, J = ei.AFF[g], 144 * g
    for name in ("from_affine", "to_affine"):
        getattr(L, f"blst_p{g}_{name}").argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        getattr(L, f"blst_p{g}_{name}").restype = None
    mult = getattr(L, f"blst_p{g}_mult")
    mult.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    mult.restype = None
    a = (ctypes.c_uint8 * A).from_buffer_copy(ei.affine_bytes(g, ei.GEN[g]))
    j, out = (ctypes.c_uint8 * J)(), (ctypes.c_uint8 * J)()
    sc = (ctypes.c_uint8 * 32).from_buffer_copy((k % ki.R).to_bytes(32, "little"))
    res = (ctypes.c_uint8 * A)()
    getattr(L, f"blst_p{g}_from_affine")(j, a)
    mult(out, j, sc, 255)
    if not any(bytes(out)[2 * (J // 3):]):  # Z == 0
        return bytes(A)
    getattr(L, f"blst_p{g}_to_affine")(res, out)
    return bytes(res)


def main():
    L = ctypes.CDLL(os.path.join(REPO, "oracle", "_ref", "libblst_ref.so"))
    log_n, tau = ki.GOLDEN_LOG_N, ki.TAU

    def point(g, k):
        raw = ref_gen_mult(L, g, k)
        want = ki.g1(k) if g == 1 else ki.g2(k)
        assert raw == ei.affine_bytes(g, want), (g, hex(k), "the oracle's multiple differs from the reference")
        return ei.encode_point(g, ei.affine_point(g, raw), True).hex()

    lag = ki.lagrange_at(tau, log_n)
    polys, points = ki.golden_polys(), ki.golden_points()
    out = {"source": "reference libblst (oracle/_ref/libblst_ref.so) blst_p{1,2}_from_affine + blst_p{1,2}_mult + "
                     "blst_p{1,2}_to_affine on the generators, by the scalars of tests/kzg_inputs.py (TAU, "
                     "golden_polys, golden_points); points compressed, z and y hex integers",
           "log_n": log_n, "tau": hex(tau),
           "srs": [point(1, l) for l in lag],
           "tau_g2": point(2, tau),
           "commitments": [point(1, ki.commit_scalar(f, lag)) for f in polys],
           "openings": []}
    for f, zs in zip(polys, points):
        row = []
        for z in zs:
            y, k = ki.proof_scalar(f, z, lag, tau, log_n)
            row.append({"z": hex(z), "y": hex(y), "proof": point(1, k)})
        out["openings"].append(row)
    with open(os.path.join(HERE, "kzg.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(len(out["srs"]), "srs points,", sum(len(r) for r in out["openings"]), "openings")


if __name__ == "__main__":
    main()
