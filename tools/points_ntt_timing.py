"""NTTs over group elements (msm_points_ntt) on device-resident points: the device
time of `batch` transforms of n = 2^log_n points (device events around the call on
its stream; median of 5 after 2 warm-ups), forward and inverse, for
  G1  256 x 2^12, 1 x 2^12, 1 x 2^16, 1 x 2^20        G2  1 x 2^12, 1 x 2^16
and beside each
  - the VALU prediction: the field products as built (products_as_built below) over
    the Fp-mul rate that msm_valu_probe measures in the same process;
  - msm_points_mult on batch n / 2 device-resident points, measured in the same
    process, times the number of laddered levels (an inverse's n^-1 pass counts as
    two): what a caller stitching the transform from the existing calls would pay
    for the multiplications alone.
The inputs are distinct points [k_i]G (SplitMix64 scalars below r, by ps_mult on the
generator: a repeated tile would make the first levels' differences infinity).  Each
case is checked: the inverse of the forward result is the input, byte for byte.

Every case runs in a child process of its own under `timeout`; the parent (which
never opens the GPU) stops at the first failure.  Prints one JSON line.

usage: python tools/points_ntt_timing.py [--out file.json]   (default profiles/points_ntt_timing.json)
       python tools/points_ntt_timing.py --case <group> <batch> <log_n>   (one case, one JSON line)"""
import ctypes
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

WARMUP, SAMPLES = 2, 5
CASES = [(1, 256, 12), (1, 1, 12), (1, 1, 16), (1, 1, 20), (2, 1, 12), (2, 1, 16)]
CASE_TIMEOUT_S = 240
CHUNK, SLICE = 1 << 20, 1 << 18


def _tree(elems, mul, lanes):
    """the shared inversion tree per element (tools/points_mult_timing.py)"""
    lv, e = [], elems
    while e:
        e = (e + 7) // 8
        lv.append(e)
        if e <= 256:
            break
    return mul * (4 + sum(4 * v for v in lv[:-1]) / elems) + lanes * 575 * lv[-1] / elems


def products_as_built(group, batch, log_n, inverse):
    """Fp products of one call of csrc/points_ntt.hip (+ the shared tree of
    to_affine.hip), priced as tools/points_mult_timing.py prices them: an fp_mul2 1.5;
    G2 counts both lanes of a pair (Fp2 product 3, square 2, a b - c d 5)."""
    mul, sqr, mulsub, lanes = (1, 1, 1.5, 1) if group == 1 else (3, 2, 5, 2)
    dbl = 4 * mul + 3 * sqr + mulsub
    madd = 6 * mul + 2 * sqr + mulsub
    add = 6 * mul + 2 * sqr + 3 * mulsub  # the regrouped general add
    nw = 255 // 4 + 1
    ladder = (nw - 1) * 4 * dbl + nw * (15 / 16) * madd
    n = 1 << log_n
    points = batch * n
    c = min(points, max(CHUNK, n))
    per_point = lanes * 2 + _tree(c, mul, lanes) + (2 * mul + sqr) + lanes * 2  # in, and out through the tree
    s = min(batch * n // 2, SLICE) if log_n else 0
    mult = dbl + 6 * add + 8 * (_tree(8 * max(s, 1), mul, lanes) + 3 * mul + sqr) + ladder  # table, rows, ladder
    bfly = 2 * add
    levels = log_n
    laddered = max(log_n - 1, 0)
    total = points * per_point + (points // 2) * (levels * bfly + laddered * mult)
    if inverse and log_n:
        total += points * mult
    return total


def laddered_half_levels(log_n, inverse):
    """ladders of the call in units of batch n / 2 points"""
    return max(log_n - 1, 0) + (2 if inverse and log_n else 0)


def run_case(group, batch, log_n):
    import torch
    torch.cuda.init()  # before the engine's library initialises HIP
    import enc_inputs as ei
    import msm_blst_amd as m
    L = m.lib()
    probe = (ctypes.c_double * 4)()
    m.check(L.msm_valu_probe(0, probe))
    rate = probe[1]
    n = 1 << log_n
    cnt, A = batch * n, ei.AFF[group]
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)
    gen = ei.affine_bytes(group, ei.GEN[group])
    d_sc = torch.frombuffer(bytearray(bytes(m.gen_scalars(cnt, 1))), dtype=torch.uint8).to(dev)
    d_gen = torch.frombuffer(bytearray(gen), dtype=torch.uint8).to(dev)
    d_src = torch.zeros(cnt * A, dtype=torch.uint8, device=dev)
    d_fwd = torch.zeros(cnt * A, dtype=torch.uint8, device=dev)
    d_inv = torch.zeros(cnt * A, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    m.check(L.msm_points_mult(group, 0, d_src.data_ptr(), d_gen.data_ptr(), d_sc.data_ptr(), cnt, 255, 32, 1, 1, 1, None))
    torch.cuda.synchronize()

    def timed(call):
        ts = []
        for s in range(WARMUP + SAMPLES):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(st):
                e0.record(st)
                call()
                e1.record(st)
            st.synchronize()
            if s >= WARMUP:
                ts.append(e0.elapsed_time(e1))
        return statistics.median(ts)

    out = {"group": group, "batch": batch, "log_n": log_n, "fp_mul_per_s": rate, "warmup": WARMUP, "samples": SAMPLES}
    half = cnt // 2
    mult_ms = timed(lambda: m.check(L.msm_points_mult(group, 0, d_inv.data_ptr(), d_src.data_ptr(), d_sc.data_ptr(), half,
                                                      255, 32, 0, 1, 1, st.cuda_stream)))
    out["ps_mult_half_ms"] = round(mult_ms, 3)
    for name, flags, src, dst in (("forward", 0, d_src, d_fwd), ("inverse", 1, d_fwd, d_inv)):
        ms = timed(lambda: m.check(L.msm_points_ntt(group, 0, dst.data_ptr(), src.data_ptr(), log_n, batch, flags, 1, 1,
                                                    st.cuda_stream)))
        prods = products_as_built(group, batch, log_n, bool(flags))
        pred = prods / rate * 1e3
        stitched = mult_ms * laddered_half_levels(log_n, bool(flags))
        out[name] = {"device_resident_ms": round(ms, 3), "products_as_built": round(prods),
                     "predicted_valu_ms": round(pred, 3), "device_resident_over_predicted": round(ms / pred, 2),
                     "ps_mult_stitched_ms": round(stitched, 3),
                     "device_resident_over_ps_mult_stitched": round(ms / stitched, 2) if stitched else None}
    ok = bool(torch.equal(d_inv, d_src))
    out["inverse_of_forward_is_the_input"] = ok
    print(json.dumps(out))
    return 0 if ok else 1


def main():
    if "--case" in sys.argv:
        i = sys.argv.index("--case")
        sys.exit(run_case(int(sys.argv[i + 1]), int(sys.argv[i + 2]), int(sys.argv[i + 3])))
    out_path = (sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv
                else os.path.join(REPO, "profiles", "points_ntt_timing.json"))
    out = {"warmup": WARMUP, "samples": SAMPLES, "cases": [],
           "not_measured": "sizes above 2^20, host-memory sources and destinations, MSM_POINTS_NTT_CHUNK / _SLICE overrides"}
    for group, batch, log_n in CASES:
        cmd = ["timeout", "-k", "10", str(CASE_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--case", str(group),
               str(batch), str(log_n)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:  # stop at the first failure: nothing more is started on the GPU
            print(f"case G{group} {batch} x 2^{log_n} failed with status {r.returncode}\n{r.stdout}\n{r.stderr}",
                  file=sys.stderr)
            sys.exit(r.returncode or 1)
        out["cases"].append(json.loads(r.stdout.strip().splitlines()[-1]))
    line = json.dumps(out)
    print(line)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
