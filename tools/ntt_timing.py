"""Device-resident Fr transforms (msm_fr_ntt) at log_n 16, 20 and 24, batch sized to
2^24 elements in total, forward and inverse, and MSM_FR_MUL / MSM_FR_INV
(msm_fr_op) over 2^24 elements: the device time (device events around the call on
its stream) and, beside each,
  predicted_valu_ms   the Fr products as built (products_as_built below: half n
                      log_n butterflies less the ones with twiddle one, plus the
                      inter-pass twiddles and the 1 / n of an inverse) at the rate
                      msm_fr_probe measures in this run
  hbm_floor_ms        passes x 64 B x elements at the rate of a device copy of the
                      same bytes, timed in this run
  over_larger         the measured time over the larger of the two
The CPU comparison is the reference's blst_fr_mul / add / sub on one thread as
tools/gen_fr_golden.py recorded it (tests/golden/fr_ops.json "cpu": a 2^12 sample
called through ctypes, so it includes the call overhead; scaled, not gated).
The first transform of each output is checked against tests/fr_inputs.py at log_n
16; larger sizes are checked by transforming back.
Prints one JSON line.

usage: python tools/ntt_timing.py [total_lg=24] [--out file.json]   (default profiles/ntt_timing.json)"""
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import fr_inputs as fi  # noqa: E402

WARMUP, SAMPLES = 2, 5
EL = 32


def products_as_built(log_n, plan, inverse):
    """Fr products per transform of csrc/fr_ntt.hip"""
    n = 1 << log_n
    p = 0.0
    for k in plan:
        p += n * k / 2              # one per butterfly
        p -= n * (3 / 4 if k >= 2 else 1 / 2)  # the last step's twiddles that are one
    p += (len(plan) - 1) * n * (2 if log_n > 13 else 1)  # inter-pass twiddles (two-level table above 2^13)
    if inverse:
        p += n
    return p


def timed(torch, st, fn):
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
    return statistics.median(ts)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    total_lg = int(args[0]) if args else 24
    out_path = (sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv
                else os.path.join(REPO, "profiles", "ntt_timing.json"))
    total = 1 << total_lg
    import torch
    torch.cuda.init()  # before the engine's library initialises HIP
    import msm_blst_amd as m
    rate, probe_ms = m.fr_probe()
    with open(os.path.join(REPO, "tests", "golden", "fr_ops.json")) as f:
        cpu = json.load(f)["cpu"]
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)
    tile = 1 << 16
    src = fi.pack(fi.rand_values(tile, 1))
    d_src = torch.frombuffer(bytearray(src * (total // tile)), dtype=torch.uint8).to(dev)
    d_dst = torch.zeros(total * EL, dtype=torch.uint8, device=dev)
    d_back = torch.zeros(total * EL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    copy_ms = timed(torch, st, lambda: d_dst.copy_(d_src, non_blocking=True))
    out = {"elements": total, "fr_mul_per_s": rate, "probe_ms": round(probe_ms, 3), "copy_ms": round(copy_ms, 3),
           "copy_GBps": round(2 * total * EL / copy_ms / 1e6, 1), "warmup": WARMUP, "samples": SAMPLES,
           "reference_cpu_ns_per_call_ctypes": cpu}
    ok = True
    for log_n in (16, 20, 24):
        if log_n > total_lg:
            continue
        batch = total >> log_n
        plan = m.ntt_plan(log_n)
        for inverse in (False, True):
            ms = timed(torch, st, lambda: m.fr_ntt(d_src.data_ptr(), log_n, batch, inverse=inverse, src_on_device=True,
                                                   dst=d_dst.data_ptr(), stream=st.cuda_stream))
            prods = products_as_built(log_n, plan, inverse) * batch
            g = {"batch": batch, "plan": plan, "device_resident_ms": round(ms, 3),
                 "products_as_built": int(prods), "predicted_valu_ms": round(prods / rate * 1e3, 3),
                 "hbm_floor_ms": round(len(plan) * copy_ms, 3)}
            g["over_larger"] = round(ms / max(g["predicted_valu_ms"], g["hbm_floor_ms"]), 2)
            # one thread of the reference: a product and two add / sub per butterfly
            g["reference_cpu_1thread_ms"] = round(batch * (1 << log_n) * log_n / 2 * (cpu["mul_ns_ctypes"] +
                                                  cpu["add_ns_ctypes"] + cpu["sub_ns_ctypes"]) / 1e6, 1)
            if not inverse:  # back again; at 2^16 the first transform against the oracle too
                m.fr_ntt(d_dst.data_ptr(), log_n, batch, inverse=True, src_on_device=True, dst=d_back.data_ptr(),
                         stream=st.cuda_stream)
                st.synchronize()
                good = bool(torch.equal(d_back, d_src))
                if log_n == 16:
                    head = bytes(d_dst[:tile * EL].cpu().numpy())
                    good = good and head == fi.pack(fi.ntt(fi.unpack(src)))
                g["outputs_equal_expected"] = good
                ok = ok and good
            out[f"ntt_{log_n}_{'inverse' if inverse else 'forward'}"] = g
    for op, per_elem, copies in (("mul", 2.0, 1.5), ("inv", 5.0 + 4 / 7 + 4 / 49, 2.5)):
        # products per element as built (inv: up, prefix, two of back-substitution, the change of
        # form, and the levels above); bytes moved as multiples of a copy of the array (mul: two
        # reads and a write; inv: level 0 is read three times and written once, plus the levels)
        ms = timed(torch, st, lambda: m.fr_op(op, d_src.data_ptr(), d_src.data_ptr(), total, src_on_device=True,
                                              dst=d_dst.data_ptr(), stream=st.cuda_stream))
        g = {"device_resident_ms": round(ms, 3), "products_per_element_as_built": round(per_elem, 2),
             "predicted_valu_ms": round(total * per_elem / rate * 1e3, 3), "hbm_floor_ms": round(copies * copy_ms, 3)}
        g["over_larger"] = round(ms / max(g["predicted_valu_ms"], g["hbm_floor_ms"]), 2)
        g["reference_cpu_1thread_ms"] = round(total * cpu["mul_ns_ctypes"] / 1e6, 1) if op == "mul" else "not measured"
        head = fi.unpack(bytes(d_dst[:64 * EL].cpu().numpy()))
        a = fi.unpack(src[:64 * EL])
        good = head == [x * x % fi.R if op == "mul" else pow(x, fi.R - 2, fi.R) for x in a]
        g["outputs_equal_expected"] = good
        ok = ok and good
        out[f"fr_{op}"] = g
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
