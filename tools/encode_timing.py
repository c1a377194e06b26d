"""Bulk point encoding (msm_points_encode) of n = 2^lg points, G1 and G2,
compressed and serialized: the device-resident time from affine points and from
Jacobians (device events around the calls on their stream), the host-to-host
time from pageable and from pinned memory (affine source), and next to them
what they are compared against, measured in the same run:
  * a device-to-device copy that moves the same bytes as the affine kernel (it
    reads `in` and writes `out` bytes; a copy of (in + out) / 2 bytes reads and
    writes as many in total);
  * msm_points_to_affine on the same Jacobians (the same tree, affine output),
    with the spread of its samples;
  * the reference's one-point calls on one CPU thread (through
    oracle/_ref/libblst_ref.so when that file is present; a 2^14 sample,
    scaled), with a check that the outputs are equal.
The input is a tile of 2^14 distinct fixed points (Jacobians: random Z,
tests/jac_inputs.py), repeated; the outputs are checked against the plain-Python
encoder (tests/enc_inputs.py).  Prints one JSON line.

usage: python tools/encode_timing.py [lg=20] [--out file.json]   (default profiles/encode_timing.json)"""
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
import jac_inputs as ji  # noqa: E402

WARMUP, SAMPLES = 2, 9
TILE_LG = 14


def spread(ts):
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


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
    out_path = (sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv
                else os.path.join(REPO, "profiles", "encode_timing.json"))
    n = 1 << lg
    tile = min(n, 1 << TILE_LG)
    import torch
    torch.cuda.init()  # before the engine's library initialises HIP (tests/conftest.py: torch found no device after it)
    import msm_blst_amd as m
    L = m.lib()
    ref_path = os.path.join(REPO, "oracle", "_ref", "libblst_ref.so")
    ref = ctypes.CDLL(ref_path) if os.path.exists(ref_path) else None
    out = {"n": n, "warmup": WARMUP, "samples": SAMPLES, "input_tile": tile}
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)
    all_ok = True

    def timed(fn):
        ts = []
        for s in range(WARMUP + SAMPLES):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(st):
                e0.record(st)
                fn()
                e1.record(st)
            st.synchronize()
            if s >= WARMUP:
                ts.append(e0.elapsed_time(e1))
        return ts

    for group in (1, 2):
        A, J = ei.AFF[group], ji.JAC[group]
        aff_tile = bytes(m.fixed_points(group, tile))
        jac_tile = ji.jacobians(group, aff_tile, tile, 0xe2c + group)
        reps = n // tile
        d_aff = torch.frombuffer(bytearray(aff_tile * reps), dtype=torch.uint8).to(dev)
        d_jac = torch.frombuffer(bytearray(jac_tile * reps), dtype=torch.uint8).to(dev)
        d_aff_out = torch.zeros(n * A, dtype=torch.uint8, device=dev)
        src_pg = (ctypes.c_uint8 * (n * A)).from_buffer_copy(aff_tile * reps)
        src_pin = torch.frombuffer(bytearray(aff_tile * reps), dtype=torch.uint8).pin_memory()
        torch.cuda.synchronize()
        # the parent's tree on the same Jacobians
        ta = timed(lambda: m.check(L.msm_points_to_affine(group, 0, d_aff_out.data_ptr(), d_jac.data_ptr(), n, 1, 1,
                                                          st.cuda_stream)))
        ta_ok = bytes(d_aff_out[:tile * A].cpu().numpy()) == aff_tile
        all_ok = all_ok and ta_ok
        for enc in (0, 1):
            E = ei.ENC[group] * (1 + enc)
            want_tile = ei.encode(group, aff_tile, tile, enc == 0)
            want = want_tile * reps
            g = {"bytes_in_affine": n * A, "bytes_in_jacobian": n * J, "bytes_out": n * E,
                 "products_per_point_affine": 2 * group, "to_affine_ms": spread(ta), "to_affine_output_ok": ta_ok}
            d_dst = torch.zeros(n * E, dtype=torch.uint8, device=dev)
            ts = timed(lambda: m.check(L.msm_points_encode(group, 0, d_dst.data_ptr(), d_aff.data_ptr(), n, 0, enc, 0,
                                                           1, 1, st.cuda_stream)))
            ok = bytes(d_dst.cpu().numpy()) == want
            g["device_resident_affine_ms"] = spread(ts)
            d_dst.zero_()
            ts = timed(lambda: m.check(L.msm_points_encode(group, 0, d_dst.data_ptr(), d_jac.data_ptr(), n, 1, enc, 0,
                                                           1, 1, st.cuda_stream)))
            ok = ok and bytes(d_dst.cpu().numpy()) == want
            g["device_resident_jacobian_ms"] = spread(ts)
            g["jacobian_over_to_affine"] = round(g["device_resident_jacobian_ms"]["median"] / g["to_affine_ms"]["median"], 3)
            # a copy that moves the same bytes as the affine kernel
            half = (n * A + n * E) // 2
            c_src = torch.zeros(half, dtype=torch.uint8, device=dev)
            c_dst = torch.empty(half, dtype=torch.uint8, device=dev)
            ts = timed(lambda: c_dst.copy_(c_src, non_blocking=True))
            g["d2d_copy_same_bytes_ms"] = spread(ts)
            g["affine_over_copy"] = round(g["device_resident_affine_ms"]["median"] / g["d2d_copy_same_bytes_ms"]["median"], 2)
            g["affine_gbytes_per_s"] = round((n * A + n * E) / g["device_resident_affine_ms"]["median"] / 1e6, 1)
            del c_src, c_dst
            dst_pg = (ctypes.c_uint8 * (n * E))()
            g["host_pageable_ms"] = median_ms(
                lambda: m.check(L.msm_points_encode(group, 0, dst_pg, src_pg, n, 0, enc, 0, 0, 0, None)), 1, SAMPLES)
            ok = ok and bytes(dst_pg) == want
            dst_pin = torch.zeros(n * E, dtype=torch.uint8).pin_memory()
            g["host_pinned_ms"] = median_ms(
                lambda: m.check(L.msm_points_encode(group, 0, dst_pin.data_ptr(), src_pin.data_ptr(), n, 0, enc, 0, 0,
                                                    0, None)), 1, SAMPLES)
            ok = ok and bytes(dst_pin.numpy()) == want
            g["outputs_equal_expected"] = bool(ok)
            all_ok = all_ok and ok
            if ref is not None:  # the reference, one point at a time, one CPU thread
                for form, name, src_tile, sz in (("affine", "affine_", aff_tile, A), ("jacobian", "", jac_tile, J)):
                    f = getattr(ref, f"blst_p{group}_{name}{'serialize' if enc else 'compress'}")
                    f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_void_p], None
                    src_ref = (ctypes.c_uint8 * len(src_tile)).from_buffer_copy(src_tile)
                    dst_ref = (ctypes.c_uint8 * (tile * E))()
                    bi, bo = ctypes.addressof(src_ref), ctypes.addressof(dst_ref)
                    t = time.perf_counter()
                    for i in range(tile):
                        f(bo + i * E, bi + i * sz)
                    ms = (time.perf_counter() - t) * 1e3 * (n / tile)
                    g[f"reference_cpu_1thread_{form}_ms"] = round(ms, 1)
                    g[f"reference_{form}_output_equal"] = bytes(dst_ref) == want_tile
                    all_ok = all_ok and g[f"reference_{form}_output_equal"]
                    g[f"reference_over_device_resident_{form}"] = round(
                        ms / g[f"device_resident_{form}_ms"]["median"], 1)
                g["reference_sample"] = tile
            else:
                g["reference_cpu_1thread_affine_ms"] = "not measured"
            out[f"g{group}_{'serialized' if enc else 'compressed'}"] = g
            del d_dst, dst_pin
        del d_aff, d_jac, d_aff_out, src_pin
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")
    if not all_ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
