"""Bulk hash-to-curve (msm_points_hash) of n = 2^lg messages of 32 bytes, device
resident, G1 and G2, hash (count 2) and encode (count 1): the time between device
events around the call on its stream; msm_hash_to_field alone and msm_points_map
alone on its output, so that the SHA-256 share is visible; the reference's own
blst_hash_to_g{1,2} on one CPU thread of the same box (through
oracle/_ref/libblst_ref.so when that file is present; a 2^12 sample, scaled) and
the VALU prediction -- the field products per point as built (products_as_built
below; the SHA-256 kernel and the final batch inversion are not counted) over the
Fp-mul rate that msm_valu_probe measures in this run -- each next to what it is
compared against.  The input is a tile of 2^12 distinct messages, repeated; its
first eight are the "fixed32" case of tests/golden/hash_to_curve.json, whose
recorded points the hashed output is checked against, and map(field(msgs)) must
equal hash(msgs).  Prints one JSON line.

usage: python tools/hash_to_curve_timing.py [lg=20] [--out file.json]   (default profiles/hash_to_curve_timing.json)"""
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import h2c_inputs as h  # noqa: E402

WARMUP, SAMPLES = 2, 5
TILE_LG = 12
CPU_THREADS = 16  # what a caller without the GPU could use on these machines


def products_as_built(group, count):
    """Fp products per point of csrc/hash_to_curve.hip by stage (sswu, iso, clear), an
    fp_mul2 (two products, one reduction) priced 1.5 and an fp_mul4 2.5 Fp products; G2
    counts both lanes of a pair.  The (p-3)/4 chain as in tools/decode_timing.py."""
    e = (h.P - 3) // 4
    chain = 2 + 2 * 189 + sum(1 for k in range(190) if (e >> (2 * k)) & 3)
    if group == 1:
        sswu = 29 + chain
        add = 14
        iso = (3 * (11 + 10 + 15 + 15) - 4) + 10
        dbl, full = 8.5, 13.5
        clear = 63 * dbl + 6 * full
    else:
        sswu = 2 * (48.5 + 4 * chain)
        add = 2 * 20
        iso = 2 * (11 * 4.5 - 4 * 1.5 + 14.5)
        dbl, full = 11.5, 19.5
        clear = 2 * (127 * dbl + 15 * full + 5 * 3)
    return {"sswu": count * sswu, "iso": (add if count == 2 else 0) + iso, "clear": clear,
            "total": count * sswu + (add if count == 2 else 0) + iso + clear}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    lg = int(args[0]) if args else 20
    out_path = (sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv
                else os.path.join(REPO, "profiles", "hash_to_curve_timing.json"))
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
    with open(os.path.join(REPO, "tests", "golden", "hash_to_curve.json")) as f:
        fixture = json.load(f)["groups"]
    out = {"n": n, "msg_len": 32, "fp_mul_per_s": fpmul_rate, "warmup": WARMUP, "samples": SAMPLES, "input_tile": tile,
           "cpu_threads_compared": CPU_THREADS}
    dev = torch.device("cuda:0")
    msgs_tile = b"".join(h._bytes(32, 200 + i) for i in range(tile))
    msgs = msgs_tile * (n // tile)
    d_msgs = torch.frombuffer(bytearray(msgs), dtype=torch.uint8).to(dev)
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
        return round(statistics.median(ts), 3)

    for group in (1, 2):
        A, E = h.AFF[group], h.ELEM[group]
        tag = h.DST[group]
        d_dst = torch.zeros(n * A, dtype=torch.uint8, device=dev)
        d_map = torch.zeros(n * A, dtype=torch.uint8, device=dev)
        d_el = torch.zeros(n * 2 * E, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        for encode in (0, 1):
            count = 1 if encode else 2
            g = {"products_per_point_as_built": {k: round(v, 1) for k, v in products_as_built(group, count).items()}}
            g["device_resident_ms"] = timed(lambda: m.check(L.msm_points_hash(
                group, 0, d_dst.data_ptr(), d_msgs.data_ptr(), None, 32, None, 0, n, tag, len(tag), encode, 1, 1,
                st.cuda_stream)))
            g["hash_to_field_ms"] = timed(lambda: m.check(L.msm_hash_to_field(
                group, 0, d_el.data_ptr(), d_msgs.data_ptr(), None, 32, None, 0, n, tag, len(tag), count, 1, 1,
                st.cuda_stream)))
            g["map_to_curve_ms"] = timed(lambda: m.check(L.msm_points_map(
                group, 0, d_map.data_ptr(), d_el.data_ptr(), n, count, 1, 1, st.cuda_stream)))
            got = bytes(d_dst[:tile * A].cpu().numpy())
            ok = bool(torch.equal(d_dst, d_map)) and bytes(d_dst[-tile * A:].cpu().numpy()) == got
            if not encode:
                want = fixture[str(group)]["cases"]["fixed32"]
                ok = ok and all(h.fnv(got[i * A:(i + 1) * A]) == want[i]["fnv"] for i in range(8))
            g["outputs_equal_expected"] = bool(ok)
            all_ok = all_ok and ok
            g["predicted_valu_ms"] = round(n * g["products_per_point_as_built"]["total"] / fpmul_rate * 1e3, 3)
            g["map_over_predicted"] = round(g["map_to_curve_ms"] / g["predicted_valu_ms"], 2)
            g["sha_share"] = round(g["hash_to_field_ms"] / g["device_resident_ms"], 3)
            if ref is not None:  # the reference, one message at a time, one CPU thread
                f = getattr(ref, f"blst_{'encode' if encode else 'hash'}_to_g{group}")
                f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                              ctypes.c_void_p, ctypes.c_size_t]
                f.restype = None
                toa = getattr(ref, f"blst_p{group}_to_affine")
                toa.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
                src = (ctypes.c_uint8 * len(msgs_tile)).from_buffer_copy(msgs_tile)
                jac = (ctypes.c_uint8 * (144 * group))()
                dst_ref = (ctypes.c_uint8 * (tile * A))()
                base_in, base_out = ctypes.addressof(src), ctypes.addressof(dst_ref)
                t = time.perf_counter()
                for i in range(tile):
                    f(jac, base_in + 32 * i, 32, tag, len(tag), None, 0)
                    toa(base_out + i * A, jac)
                ms = (time.perf_counter() - t) * 1e3 * (n / tile)
                g["reference_cpu_1thread_ms"] = round(ms, 1)
                g["reference_sample"] = tile
                g["reference_output_equal"] = bytes(dst_ref) == got
                all_ok = all_ok and g["reference_output_equal"]
                g["reference_over_device_resident"] = round(ms / g["device_resident_ms"], 1)
                g[f"device_resident_beats_{CPU_THREADS}_cpu_threads"] = bool(ms / CPU_THREADS > g["device_resident_ms"])
            else:
                g["reference_cpu_1thread_ms"] = "not measured"
            out[f"g{group}_{'encode' if encode else 'hash'}"] = g
        del d_dst, d_map, d_el
    line = json.dumps(out)
    print(line)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")
    if not all_ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
