"""Bulk point decoding (msm_points_decode) of n = 2^lg compressed entries, G1
and G2, with and without the subgroup check: the device-resident time (device
events around the calls on their stream), the host-to-host time from pageable
and from pinned memory, the reference's own blst_p{1,2}_uncompress (+
blst_p{1,2}_affine_in_g{1,2}) on one CPU thread of the same box (through
oracle/_ref/libblst_ref.so when that file is present; a 2^14 sample, scaled)
and the VALU prediction -- the field products per point as built
(products_as_built below) over the Fp-mul rate that msm_valu_probe measures in
this run -- each next to what it is compared against.  The input is a tile of
2^14 distinct fixed points, encoded in plain Python (tests/enc_inputs.py) and
repeated; the outputs are checked against the affine points they encode.
Prints one JSON line.

usage: python tools/decode_timing.py [lg=20] [--out file.json]   (default profiles/decode_timing.json)"""
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
TILE_LG = 14
CPU_THREADS = 16  # what a caller without the GPU could use on these machines


def products_as_built(group, check_group):
    """Fp products per point of csrc/decode.hip, an fp_mul2 (two products, one
    reduction: 588 multiply-adds) priced 1.5 and an fp_mul4 2.5 Fp products."""
    e = (ei.P - 3) // 4
    windows = [(e >> (2 * k)) & 3 for k in range(190)]
    chain = 2 + 2 * 189 + sum(1 for w in windows if w)  # a^2, a^3, squarings, products of nonzero windows
    if group == 1:
        dec = 1 + 2 + chain + 1 + 1 + 1 + 1 + 2  # parse, x^3, chain, y, y^2, ==, sign, output
        dbl, madd = 7 + 1.5, 8 + 1.5
        grp = 127 * dbl + (bin(0xd201000000010000 ** 2).count("1") - 1) * madd + 7
        return dec + (grp if check_group else 0)
    # per lane of a pair (Fp2 square 1, Fp2 product 1.5, a b - c d 2.5), two lanes per point
    dec = 1 + 1 + 1.5 + (2 + chain + 1 + 2) + (chain + 1 + 2 + 1 + 1) + 1 + 1 + 1 + 2
    dbl, madd = 3 + 4 * 1.5 + 2.5, 2 * 1.5 + 1 + 4 * 1.5 + 1 + 2.5
    grp = 63 * dbl + 5 * madd + 10
    return 2 * (dec + (grp if check_group else 0))


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
                else os.path.join(REPO, "profiles", "decode_timing.json"))
    n = 1 << lg
    tile = min(n, 1 << TILE_LG)
    import torch
    torch.cuda.init()  # before the engine's library initialises HIP (tests/conftest.py: torch found no device after it)
    import msm_blst_amd as m
    L = m.lib()
    probe = (ctypes.c_double * 4)()
    m.check(L.msm_valu_probe(0, probe))
    fpmul_rate = probe[1]
    ref_path = os.path.join(REPO, "oracle", "_ref", "libblst_ref.so")
    ref = ctypes.CDLL(ref_path) if os.path.exists(ref_path) else None
    out = {"n": n, "encoding": "compressed", "fp_mul_per_s": fpmul_rate, "warmup": WARMUP, "samples": SAMPLES,
           "input_tile": tile, "cpu_threads_compared": CPU_THREADS}
    dev = torch.device("cuda:0")
    all_ok = True
    for group in (1, 2):
        aff_tile = bytes(m.fixed_points(group, tile))
        enc_tile = ei.encode(group, aff_tile, tile, True)
        aff, enc = aff_tile * (n // tile), enc_tile * (n // tile)
        A = ei.AFF[group]
        d_src = torch.frombuffer(bytearray(enc), dtype=torch.uint8).to(dev)
        d_dst = torch.zeros(n * A, dtype=torch.uint8, device=dev)
        src_pg = (ctypes.c_uint8 * len(enc)).from_buffer_copy(enc)
        dst_pg = (ctypes.c_uint8 * (n * A))()
        st_pg = (ctypes.c_uint8 * n)()
        src_pin = torch.frombuffer(bytearray(enc), dtype=torch.uint8).pin_memory()
        dst_pin = torch.zeros(n * A, dtype=torch.uint8).pin_memory()
        st_pin = torch.zeros(n, dtype=torch.uint8).pin_memory()
        st = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        for check in (0, 1):
            g = {"products_per_point_as_built": round(products_as_built(group, check), 1)}

            def resident():
                m.check(L.msm_points_decode(group, 0, d_dst.data_ptr(), None, None, d_src.data_ptr(), n, 0, check, 1, 1,
                                            st.cuda_stream))

            ts = []
            for s in range(WARMUP + SAMPLES):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(st):
                    e0.record(st)
                    resident()
                    e1.record(st)
                st.synchronize()
                if s >= WARMUP:
                    ts.append(e0.elapsed_time(e1))
            ok = bytes(d_dst.cpu().numpy()) == aff
            g["device_resident_ms"] = round(statistics.median(ts), 3)
            g["host_pageable_ms"] = median_ms(
                lambda: m.check(L.msm_points_decode(group, 0, dst_pg, st_pg, None, src_pg, n, 0, check, 0, 0, None)),
                1, SAMPLES)
            ok = ok and bytes(dst_pg) == aff and bytes(st_pg) == bytes(n)
            g["host_pinned_ms"] = median_ms(
                lambda: m.check(L.msm_points_decode(group, 0, dst_pin.data_ptr(), st_pin.data_ptr(), None,
                                                    src_pin.data_ptr(), n, 0, check, 0, 0, None)), 1, SAMPLES)
            ok = ok and bytes(dst_pin.numpy()) == aff and not bool(st_pin.any())
            g["outputs_equal_expected"] = bool(ok)
            all_ok = all_ok and ok
            g["predicted_valu_ms"] = round(n * g["products_per_point_as_built"] / fpmul_rate * 1e3, 3)
            g["device_resident_over_predicted"] = round(g["device_resident_ms"] / g["predicted_valu_ms"], 2)
            if ref is not None:  # the reference, one entry at a time, one CPU thread
                unc = getattr(ref, f"blst_p{group}_uncompress")
                unc.argtypes, unc.restype = [ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int
                ing = getattr(ref, f"blst_p{group}_affine_in_g{group}")
                ing.argtypes, ing.restype = [ctypes.c_void_p], ctypes.c_int
                E = ei.ENC[group]
                base_in, dst_ref = ctypes.addressof(src_pg), (ctypes.c_uint8 * (tile * A))()
                base_out = ctypes.addressof(dst_ref)

                def ref_run():
                    bad = 0
                    for i in range(tile):
                        bad += unc(base_out + i * A, base_in + i * E)
                        if check:
                            bad += 1 - ing(base_out + i * A)
                    return bad

                t = time.perf_counter()
                bad = ref_run()
                ms = (time.perf_counter() - t) * 1e3 * (n / tile)
                g["reference_cpu_1thread_ms"] = round(ms, 1)
                g["reference_sample"] = tile
                g["reference_output_equal"] = bad == 0 and bytes(dst_ref) == aff_tile
                g["reference_over_device_resident"] = round(ms / g["device_resident_ms"], 1)
                g[f"device_resident_beats_{CPU_THREADS}_cpu_threads"] = bool(ms / CPU_THREADS > g["device_resident_ms"])
            else:
                g["reference_cpu_1thread_ms"] = "not measured"
            out[f"g{group}_{'checked' if check else 'unchecked'}"] = g
        del d_src, d_dst, src_pin, dst_pin, st_pin
    line = json.dumps(out)
    print(line)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")
    if not all_ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
