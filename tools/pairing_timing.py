"""Bulk pairings (msm_pairing_segments, msm_fp12_final_exp) of n = 2^lg pairs, device
resident: single pairings, the same pairs in segments of 2 and of 64, and the final
exponentiation alone: the time between device events around the call on its stream
(median of 5 after 2 warm-ups); the reference's own blst_miller_loop + blst_final_exp
on one CPU thread of the same box (through oracle/_ref/libblst_ref.so when that
file is present; a small sample, scaled) and the VALU prediction -- the field
products per pair and per final exponentiation as built (products_as_built below)
over the Fp-mul rate that msm_valu_probe measures in this run -- each next to what
it is compared against.  The input is the 24 seeded pairs of tests/pairing_inputs.py,
repeated; the outputs are checked against tests/golden/pairing.json.  Prints one
JSON line.

usage: python tools/pairing_timing.py [lg=16] [--out file.json]   (default profiles/pairing_timing.json)"""
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import pairing_inputs as pi  # noqa: E402

WARMUP, SAMPLES = 2, 5
REF_SAMPLE = 256
G = pi.FP12_BYTES


def products_as_built(piece=1):
    """Fp products of csrc/pairing.hip per pair (Miller loop, pieces of `piece` pairs) and
    per final exponentiation, both lanes of a pair counted: an Fp2 product is one fp_mul2
    per lane (two products, one reduction, priced 1.5), an Fp2 square and a product by an
    Fp factor one fp_mul per lane.  The Fermat chain of the one Fp inversion as fp_inv
    builds it (2-bit windows of p - 2)."""
    mul2, sqr2, scale2 = 3.0, 2.0, 2.0
    mul6, xy0, oy0 = 6 * mul2, 5 * mul2, 3 * mul2
    mul12, sqr12, sparse = 3 * mul6, 2 * mul6, 2 * xy0 + oy0
    dbl = 8 * sqr2 + 3 * mul2 + 2 * scale2
    add = 4 * sqr2 + 9 * mul2 + 2 * scale2
    miller = 63 * (dbl + sparse) + 5 * (add + sparse) + 62 * sqr12 / piece
    cyc = 9 * sqr2
    e = pi.P - 2
    chain = 2 * (2 + 2 * ((e.bit_length() + 1) // 2 - 1) + sum(1 for k in range(191) if (e >> (2 * k)) & 3))
    inv12 = 4 * mul6 + 3 * sqr2 + 9 * mul2 + chain + 2 * 2
    n_csqr = 4 * 63 + 62 + 1
    n_mul = 5 * 5 + 2 + 8
    fe = n_mul * mul12 + n_csqr * cyc + 5 * 6 * mul2 + inv12 + 6 * 2 * 2
    return {"miller_per_pair": round(miller, 1), "final_exp": round(fe, 1), "fp12_mul": mul12, "fp12_sqr": sqr12,
            "sparse_mul": sparse, "line_dbl": dbl, "line_add": add, "cyclotomic_sqr": cyc, "inversion": round(inv12, 1)}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    lg = int(args[0]) if args else 16
    out_path = (sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv
                else os.path.join(REPO, "profiles", "pairing_timing.json"))
    n = 1 << lg
    import torch
    torch.cuda.init()  # before the engine's library initialises HIP
    import msm_blst_amd as m
    L = m.lib()
    probe = (ctypes.c_double * 4)()
    m.check(L.msm_valu_probe(0, probe))
    rate = probe[1]
    with open(os.path.join(REPO, "tests", "golden", "pairing.json")) as f:
        fixture = json.load(f)
    tile = pi.N_RANDOM
    idx = [i % tile for i in range(n)]
    p, q = pi.pair_bytes(list(range(tile)))
    reps = (n + tile - 1) // tile
    dev = torch.device("cuda:0")
    d_p = torch.frombuffer(bytearray((p * reps)[:n * 96]), dtype=torch.uint8).to(dev)
    d_q = torch.frombuffer(bytearray((q * reps)[:n * 192]), dtype=torch.uint8).to(dev)
    d_out = torch.zeros(n * G, dtype=torch.uint8, device=dev)
    d_ml = torch.zeros(n * G, dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()

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

    def segments(seg_len, flags=0, dst=None):
        k = n // seg_len
        o = (ctypes.c_size_t * (k + 1))(*range(0, n + 1, seg_len)) if seg_len > 1 else None
        return lambda: m.check(L.msm_pairing_segments(0, (dst if dst is not None else d_out).data_ptr(), None, None,
                                                      d_p.data_ptr(), d_q.data_ptr(), o, k, flags, 1, 1, st.cuda_stream))

    out = {"n": n, "fp_mul_per_s": rate, "warmup": WARMUP, "samples": SAMPLES, "input_tile": tile}
    all_ok = True
    pred = products_as_built(1)
    out["products_as_built"] = pred
    r = {"device_resident_ms": timed(segments(1))}
    got = bytes(d_out[:tile * G].cpu().numpy())
    ok = all((got[i * G:(i + 1) * G].hex() if i < 8 else pi.fnv(got[i * G:(i + 1) * G])) == fixture["pairs"][i]["e"]
             for i in range(tile))
    ok = ok and bytes(d_out[(n - n % tile - tile) * G:(n - n % tile) * G].cpu().numpy()) == got
    r["outputs_equal_expected"] = bool(ok)
    all_ok = all_ok and ok
    r["predicted_valu_ms"] = round(n * (pred["miller_per_pair"] + pred["final_exp"]) / rate * 1e3, 3)
    r["measured_over_predicted"] = round(r["device_resident_ms"] / r["predicted_valu_ms"], 2)
    r["miller_only_ms"] = timed(segments(1, m.PAIRING_MILLER_ONLY, d_ml))
    r["miller_predicted_valu_ms"] = round(n * pred["miller_per_pair"] / rate * 1e3, 3)
    r["miller_over_predicted"] = round(r["miller_only_ms"] / r["miller_predicted_valu_ms"], 2)
    out["single"] = r
    r = {"final_exp_ms": timed(lambda: m.check(L.msm_fp12_final_exp(0, d_out.data_ptr(), None, None, d_ml.data_ptr(), n, 1,
                                                                     1, st.cuda_stream)))}
    ok = bytes(d_out[:tile * G].cpu().numpy()) == got
    r["outputs_equal_expected"] = bool(ok)
    all_ok = all_ok and ok
    r["predicted_valu_ms"] = round(n * pred["final_exp"] / rate * 1e3, 3)
    r["measured_over_predicted"] = round(r["final_exp_ms"] / r["predicted_valu_ms"], 2)
    out["final_exp"] = r
    ps = pi.pairs()
    for seg_len in (2, 64):
        k = n // seg_len
        piece = L.msm_pairing_piece(n)
        r = {"segments": k, "piece": piece, "device_resident_ms": timed(segments(seg_len))}
        first = bytes(d_out[:G].cpu().numpy())
        want = pi.fp12_bytes(pi.pairing_product([ps[i] for i in idx[:seg_len]]))
        r["outputs_equal_expected"] = first == want
        all_ok = all_ok and first == want
        pr = products_as_built(piece)
        r["predicted_valu_ms"] = round((n * pr["miller_per_pair"] + (n - k) * pr["fp12_mul"] / max(piece, 1)
                                        + k * pr["final_exp"]) / rate * 1e3, 3)
        r["measured_over_predicted"] = round(r["device_resident_ms"] / r["predicted_valu_ms"], 2)
        r["us_per_pair"] = round(r["device_resident_ms"] * 1e3 / n, 3)
        out[f"segments_of_{seg_len}"] = r
    out["single"]["us_per_pair"] = round(out["single"]["device_resident_ms"] * 1e3 / n, 3)
    ref_path = os.path.join(REPO, "oracle", "_ref", "libblst_ref.so")
    if os.path.exists(ref_path):  # the reference, one pair at a time, one CPU thread
        ref = ctypes.CDLL(ref_path)
        for f in (ref.blst_miller_loop, ref.blst_final_exp):
            f.restype = None
        ref.blst_miller_loop.argtypes = [ctypes.c_void_p] * 3
        ref.blst_final_exp.argtypes = [ctypes.c_void_p] * 2
        pb = (ctypes.c_uint8 * len(p)).from_buffer_copy(p)
        qb = (ctypes.c_uint8 * len(q)).from_buffer_copy(q)
        ml, e = (ctypes.c_uint8 * G)(), (ctypes.c_uint8 * (G * tile))()
        bp, bq, be = ctypes.addressof(pb), ctypes.addressof(qb), ctypes.addressof(e)
        t = time.perf_counter()
        for i in range(REF_SAMPLE):
            j = i % tile
            ref.blst_miller_loop(ml, bq + 192 * j, bp + 96 * j)
            ref.blst_final_exp(be + G * j, ml)
        ms = (time.perf_counter() - t) * 1e3 * (n / REF_SAMPLE)
        out["reference_cpu_1thread_ms"] = round(ms, 1)
        out["reference_sample"] = REF_SAMPLE
        out["reference_output_equal"] = bytes(e) == got
        all_ok = all_ok and out["reference_output_equal"]
        out["reference_over_device_resident"] = round(ms / out["single"]["device_resident_ms"], 1)
    else:
        out["reference_cpu_1thread_ms"] = "not measured"
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")
    if not all_ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
