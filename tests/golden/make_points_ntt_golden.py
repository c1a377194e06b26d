#!/usr/bin/env python3
"""Golden fixture for the NTT over group elements (msm_points_ntt), written from the
REFERENCE itself: oracle/_ref/libblst_ref.so (built by oracle/Makefile) is called
through ctypes.  Runs only in the build container, on the CPU.

Writes tests/golden/points_ntt.json, for n = 8, G1 and G2, forward and inverse, in
natural order, with the scalars a_j of pntt_inputs.golden_scalars():
  inputs   the reference's [a_j]G (blst_p{1,2}_mult on the generator), compressed
  forward  out[k] = sum_j [omega^(j k)] P_j, computed BY THE REFERENCE AS SUMS:
           blst_p{1,2}_mult of each input by omega^(j k), blst_p{1,2}_add_or_double
           over j, blst_p{1,2}_to_affine; compressed
  inverse  out[j] = [n^-1] sum_k [omega^(-j k)] P_k, the same way, the sum multiplied
           by n^-1 with one more blst_p{1,2}_mult
While writing, the script asserts that every sum equals [ntt(a)_k]G of the Python
oracle (tests/pntt_inputs.py on tests/fr_inputs.py).
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
import fr_inputs as fi  # noqa: E402
import mult_inputs as mi  # noqa: E402
import pntt_inputs as pi  # noqa: E402

R = fi.R
vp = ctypes.c_void_p


class Ref:
    """the reference's Jacobian calls of one group, on ctypes buffers"""

    def __init__(self, L, g):
        self.g, self.A, self.J = g, ei.AFF[g], 144 * g
        for name, args in (("from_affine", [vp, vp]), ("to_affine", [vp, vp]), ("mult", [vp, vp, vp, ctypes.c_size_t]),
                           ("add_or_double", [vp, vp, vp])):
            f = getattr(L, f"blst_p{g}_{name}")
            f.argtypes, f.restype = args, None
            setattr(self, name, f)

    def jac(self, affine):
        j = (ctypes.c_uint8 * self.J)()  # all zero: infinity (Z == 0)
        if any(affine):
            self.from_affine(j, (ctypes.c_uint8 * self.A).from_buffer_copy(affine))
        return j

    def mul(self, j, k):
        out = (ctypes.c_uint8 * self.J)()
        self.mult(out, j, (ctypes.c_uint8 * 32).from_buffer_copy((k % R).to_bytes(32, "little")), 255)
        return out

    def add(self, a, b):
        out = (ctypes.c_uint8 * self.J)()
        self.add_or_double(out, a, b)
        return out

    def affine(self, j):
        if not any(bytes(j)[2 * (self.J // 3):]):  # Z == 0
            return bytes(self.A)
        res = (ctypes.c_uint8 * self.A)()
        self.to_affine(res, j)
        return bytes(res)


def main():
    L = ctypes.CDLL(os.path.join(REPO, "oracle", "_ref", "libblst_ref.so"))
    log_n = pi.GOLDEN_LOG_N
    n, w = 1 << log_n, fi.root(log_n)
    a = pi.golden_scalars()
    out = {"source": "reference libblst (oracle/_ref/libblst_ref.so): inputs blst_p{1,2}_mult on the generators by "
                     "pntt_inputs.golden_scalars(); outputs as sums of blst_p{1,2}_mult by omega^(+-jk) with "
                     "blst_p{1,2}_add_or_double (inverse: the sum times n^-1), blst_p{1,2}_to_affine; points compressed",
           "log_n": log_n, "scalars": [hex(v) for v in a], "groups": {}}
    for g in (1, 2):
        ref = Ref(L, g)
        gen = ref.jac(ei.affine_bytes(g, ei.GEN[g]))

        def comp(raw):
            return ei.encode_point(g, ei.affine_point(g, raw), True).hex()

        def gen_point(k):
            return ei.affine_bytes(g, mi.smul(g, ei.GEN[g], k % R))

        pts = [ref.affine(ref.mul(gen, v)) for v in a]
        assert pts == [gen_point(v) for v in a], "the oracle's multiples differ from the reference's"
        assert not any(pts[3]), "the infinity input"
        jacs = [ref.jac(p) for p in pts]
        entry = {"inputs": [comp(p) for p in pts]}
        for name, inverse in (("forward", False), ("inverse", True)):
            base = pow(w, -1, R) if inverse else w
            want = pi.ntt_scalars(a, log_n, inverse=inverse)
            res = []
            for k in range(n):
                acc = (ctypes.c_uint8 * ref.J)()
                for j in range(n):
                    acc = ref.add(acc, ref.mul(jacs[j], pow(base, j * k, R)))
                if inverse:
                    acc = ref.mul(acc, pow(n, -1, R))
                raw = ref.affine(acc)
                assert raw == gen_point(want[k]), (g, name, k, "the reference's sum differs from [ntt(a)_k]G")
                res.append(comp(raw))
            entry[name] = res
        out["groups"][str(g)] = entry
    with open(os.path.join(HERE, "points_ntt.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("n =", n, "for G1 and G2, forward and inverse")


if __name__ == "__main__":
    main()
