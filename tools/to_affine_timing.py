"""Bulk Jacobian -> affine (msm_points_to_affine) at n = 2^lg, G1 and G2: the
device-resident time (device events around the calls on their stream), the
host-to-host time from pageable and from pinned memory, the reference's own
blst_p{1,2}s_to_affine on one CPU thread of the same box (through
oracle/_ref/libblst_ref.so when that file is present), and the VALU
prediction -- 9 field products per point over the Fp-mul rate that
msm_valu_probe measures in this run (an Fp2 product priced as 3 Fp products:
1176 vs 392 multiply-adds, fp.hpp) -- each next to what it is compared
against.  Checks the outputs against the expected bytes at that size.
Prints one JSON line.

usage: python tools/to_affine_timing.py [lg=20] [--out file.json]"""
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import jac_inputs as ji  # noqa: E402

WARMUP, SAMPLES = 3, 7


def median_ms(fn, warmup, samples):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(samples):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(ts), 3)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    lg = int(args[0]) if args else 20
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    n = 1 << lg
    import torch
    torch.cuda.init()  # before the engine's library initialises HIP (tests/conftest.py: torch found no device after it)
    import msm_blst_amd as m
    inputs = {}
    for group in (1, 2):  # (x l^2, y l^3, l) in plain Python integers: the expected output is aff
        aff = bytes(m.fixed_points(group, n))
        inputs[group] = (aff, ji.jacobians(group, aff, n, 1000 + group))
    L = m.lib()
    probe = (ctypes.c_double * 4)()
    m.check(L.msm_valu_probe(0, probe))
    fpmul_rate = probe[1]
    ref_path = os.path.join(REPO, "oracle", "_ref", "libblst_ref.so")
    ref = ctypes.CDLL(ref_path) if os.path.exists(ref_path) else None
    out = {"n": n, "fp_mul_per_s": fpmul_rate, "levels": m.to_affine_levels(n), "warmup": WARMUP, "samples": SAMPLES,
           "products_per_point_priced": 9}
    dev = torch.device("cuda:0")
    for group in (1, 2):
        aff, jac = inputs[group]
        J, A = ji.JAC[group], ji.AFF[group]
        d_src = torch.frombuffer(bytearray(jac), dtype=torch.uint8).to(dev)
        d_dst = torch.zeros(n * A, dtype=torch.uint8, device=dev)
        st = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()

        def resident():
            m.check(L.msm_points_to_affine(group, 0, d_dst.data_ptr(), d_src.data_ptr(), n, 1, 1, st.cuda_stream))

        reps = 10  # a sample is 10 calls: several ms, not a fraction of one
        ts = []
        for s in range(WARMUP + SAMPLES):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(st):
                e0.record(st)
                for _ in range(reps):
                    resident()
                e1.record(st)
            st.synchronize()
            if s >= WARMUP:
                ts.append(e0.elapsed_time(e1) / reps)
        ok = bytes(d_dst.cpu().numpy()) == aff
        g = {"device_resident_ms": round(statistics.median(ts), 4), "device_resident_reps_per_sample": reps}
        # host to host: pageable and pinned
        src_pg = (ctypes.c_uint8 * len(jac)).from_buffer_copy(jac)
        dst_pg = (ctypes.c_uint8 * (n * A))()
        g["host_pageable_ms"] = median_ms(
            lambda: m.check(L.msm_points_to_affine(group, 0, dst_pg, src_pg, n, 0, 0, None)), 1, SAMPLES)
        ok = ok and bytes(dst_pg) == aff
        src_pin = torch.frombuffer(bytearray(jac), dtype=torch.uint8).pin_memory()
        dst_pin = torch.zeros(n * A, dtype=torch.uint8).pin_memory()
        g["host_pinned_ms"] = median_ms(
            lambda: m.check(L.msm_points_to_affine(group, 0, dst_pin.data_ptr(), src_pin.data_ptr(), n, 0, 0, None)),
            1, SAMPLES)
        ok = ok and bytes(dst_pin.numpy()) == aff
        g["outputs_equal_expected"] = bool(ok)
        # the reference on one CPU thread
        if ref is not None:
            f = getattr(ref, f"blst_p{group}s_to_affine")
            f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
            f.restype = None
            pp = (ctypes.c_void_p * 2)(ctypes.addressof(src_pg), None)
            dst_ref = (ctypes.c_uint8 * (n * A))()
            g["reference_cpu_1thread_ms"] = median_ms(lambda: f(dst_ref, pp, n), 1, 3)
            g["reference_output_equal"] = bytes(dst_ref) == aff
            g["reference_over_device_resident"] = round(g["reference_cpu_1thread_ms"] / g["device_resident_ms"], 1)
            g["reference_over_host_pageable"] = round(g["reference_cpu_1thread_ms"] / g["host_pageable_ms"], 2)
        else:
            g["reference_cpu_1thread_ms"] = "not measured"
        g["predicted_valu_ms"] = round(n * 9 * (1 if group == 1 else 3) / fpmul_rate * 1e3, 4)
        g["device_resident_over_predicted"] = round(g["device_resident_ms"] / g["predicted_valu_ms"], 2)
        out[f"g{group}"] = g
        del d_src, d_dst, src_pin, dst_pin
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")
    if not all(out[f"g{g}"]["outputs_equal_expected"] for g in (1, 2)):
        sys.exit(1)


if __name__ == "__main__":
    main()
