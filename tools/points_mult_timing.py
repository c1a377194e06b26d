"""Bulk scalar multiplication (msm_points_mult) of n = 2^lg device-resident
points at nbits = 255, G1 and G2, with per-point bases and in one-point mode:
the device time (device events around the call on its stream), the reference's
own blst_p{1,2}_mult on one CPU thread of the same box (through
oracle/_ref/libblst_ref.so when that file is present; a 2^12 sample, scaled) and
the VALU prediction -- the field products per point as built (products_as_built
below) over the Fp-mul rate that msm_valu_probe measures in this run -- each
next to what it is compared against.  The points are a tile of 2^14 distinct
fixed points, repeated; the scalars are SplitMix64 values below r.  The first
2^12 outputs are checked against the reference's (or, without it, the one-point
outputs against the per-point call on copies of the point).
Prints one JSON line.

usage: python tools/points_mult_timing.py [lg=20] [--out file.json]   (default profiles/points_mult_timing.json)"""
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import enc_inputs as ei  # noqa: E402

WARMUP, SAMPLES = 2, 7
TILE_LG, REF_LG = 14, 12
NBITS = 255
CPU_THREADS = 16  # what a caller without the GPU could use on these machines
CHUNK = 1 << 18


def products_as_built(group, one_point, n, nbits=NBITS):
    """Fp products per point of csrc/points_mult.hip (+ the shared tree of
    to_affine.hip), an fp_mul2 (two products, one reduction) priced 1.5 and an
    fp_mul4 2.5 Fp products; G2 counts both lanes of a pair (Fp2 product 3, square
    2, a b - c d 5)."""
    mul, sqr, mulsub, lanes = (1, 1, 1.5, 1) if group == 1 else (3, 2, 5, 2)
    dbl = 4 * mul + 3 * sqr + mulsub
    madd = 6 * mul + 2 * sqr + mulsub
    nw = nbits // 4 + 1
    ladder = (nw - 1) * 4 * dbl + nw * (15 / 16) * madd  # a Booth digit is zero for 2 of 32 patterns

    def tree(elems):  # up, prefix, back-substitution (2), the levels above, the leaf inversions (~570 each)
        lv, e = [], elems
        while e:
            e = (e + 7) // 8
            lv.append(e)
            if e <= 256:
                break
        return mul * (4 + sum(4 * v for v in lv[:-1]) / elems) + lanes * 575 * lv[-1] / elems

    c = min(n, CHUNK)
    out = ladder + tree(c) + (2 * mul + sqr) + lanes * 2  # 1/Z, 1/ZZ, x, y, and the two products into blst form
    if one_point:
        return out
    table = lanes * 2 + (2 * mul + 2 * sqr + dbl) + 6 * madd  # the points into internal form, 2P by the doubling branch, 3P .. 8P
    rows = 7 * (tree(7 * c) + 3 * mul + sqr)
    return out + table + rows


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    lg = int(args[0]) if args else 20
    out_path = (sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv
                else os.path.join(REPO, "profiles", "points_mult_timing.json"))
    n = 1 << lg
    tile = min(n, 1 << TILE_LG)
    nref = min(n, 1 << REF_LG)
    import torch
    torch.cuda.init()  # before the engine's library initialises HIP (tests/conftest.py: torch found no device after it)
    import msm_blst_amd as m
    L = m.lib()
    probe = (ctypes.c_double * 4)()
    m.check(L.msm_valu_probe(0, probe))
    fpmul_rate = probe[1]
    ref_path = os.path.join(REPO, "oracle", "_ref", "libblst_ref.so")
    ref = ctypes.CDLL(ref_path) if os.path.exists(ref_path) else None
    out = {"n": n, "nbits": NBITS, "fp_mul_per_s": fpmul_rate, "warmup": WARMUP, "samples": SAMPLES, "input_tile": tile,
           "cpu_threads_compared": CPU_THREADS}
    dev = torch.device("cuda:0")
    sc = bytes(m.gen_scalars(n, 1))
    d_sc = torch.frombuffer(bytearray(sc), dtype=torch.uint8).to(dev)
    all_ok = True
    for group in (1, 2):
        A, J = ei.AFF[group], 144 * group
        aff_tile = bytes(m.fixed_points(group, tile))
        gen = ei.affine_bytes(group, ei.GEN[group])
        d_pts = torch.frombuffer(bytearray(aff_tile * (n // tile)), dtype=torch.uint8).to(dev)
        d_gen = torch.frombuffer(bytearray(gen), dtype=torch.uint8).to(dev)
        d_dst = torch.zeros(n * A, dtype=torch.uint8, device=dev)
        st = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        heads = {}
        for one in (0, 1):
            g = {"products_per_point_as_built": round(products_as_built(group, one, n), 1)}
            src = d_gen if one else d_pts
            ts = []
            for s in range(WARMUP + SAMPLES):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(st):
                    e0.record(st)
                    m.check(L.msm_points_mult(group, 0, d_dst.data_ptr(), src.data_ptr(), d_sc.data_ptr(), n, NBITS, 32,
                                              one, 1, 1, st.cuda_stream))
                    e1.record(st)
                st.synchronize()
                if s >= WARMUP:
                    ts.append(e0.elapsed_time(e1))
            heads[one] = bytes(d_dst[:nref * A].cpu().numpy())
            g["device_resident_ms"] = round(statistics.median(ts), 3)
            g["predicted_valu_ms"] = round(n * g["products_per_point_as_built"] / fpmul_rate * 1e3, 3)
            g["device_resident_over_predicted"] = round(g["device_resident_ms"] / g["predicted_valu_ms"], 2)
            if ref is not None:  # the reference, one point at a time, one CPU thread
                fa, mult, ta = (getattr(ref, f"blst_p{group}_{f}") for f in ("from_affine", "mult", "to_affine"))
                fa.argtypes = ta.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
                mult.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
                fa.restype = mult.restype = ta.restype = None
                src_aff = (ctypes.c_uint8 * (nref * A)).from_buffer_copy(gen * nref if one else aff_tile[:nref * A])
                jac, res = (ctypes.c_uint8 * (nref * J))(), (ctypes.c_uint8 * (nref * J))()
                aff = (ctypes.c_uint8 * (nref * A))()
                h_sc = (ctypes.c_uint8 * (nref * 32)).from_buffer_copy(sc[:nref * 32])
                pa, pj, pr, po, ps = (ctypes.addressof(b) for b in (src_aff, jac, res, aff, h_sc))
                for i in range(nref):
                    fa(pj + i * J, pa + i * A)
                t = time.perf_counter()
                for i in range(nref):
                    mult(pr + i * J, pj + i * J, ps + i * 32, NBITS)
                ms = (time.perf_counter() - t) * 1e3 * (n / nref)
                for i in range(nref):
                    ta(po + i * A, pr + i * J)
                ok = bytes(aff) == heads[one]
                g["reference_cpu_1thread_ms"] = round(ms, 1)
                g["reference_sample"] = nref
                g["reference_over_device_resident"] = round(ms / g["device_resident_ms"], 1)
                g[f"device_resident_beats_{CPU_THREADS}_cpu_threads"] = bool(ms / CPU_THREADS > g["device_resident_ms"])
            else:
                g["reference_cpu_1thread_ms"] = "not measured"
                ok = True
                if one:  # the per-point call on copies of the generator
                    ok = heads[1] == m.ps_mult(group, gen * nref, sc[:nref * 32], nref)
            g["outputs_equal_expected"] = bool(ok)
            all_ok = all_ok and ok
            out[f"g{group}_{'one_point' if one else 'per_point'}"] = g
        del d_pts, d_dst
    line = json.dumps(out)
    print(line)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")
    if not all_ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
