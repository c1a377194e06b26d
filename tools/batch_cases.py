"""One MSM batch case in this process: G1 at 2^12 and G2 at 2^10, each call between
two device synchronisations and twice on one context (so every ring is reused),
every result compared with the synchronous mult of its set.

The batch knobs (csrc/batch_plan.hpp BatchKnobs) are read once per process, so a
knob setting is the environment of one run of this script.  Run under
`rocprofv3 --hip-runtime-trace --output-format json` it gives the trace that
tools/hip_trace_compare.py compares between two builds; the GPU test
tests/test_gpu_batch_schedules.py runs it plain.

Kind `sync` is no batch: one synchronous mult each of CHES G1 2^12 and G2 2^10,
BGMW95 G1, the plain engine G1 and blst_p1s_mult_pippenger through the drop-in,
each against the plain engine's result.

usage: batch_cases.py <repo> ches|plain|segments|profile|sync [K] [device|pinned|pageable ...]
prints one line per call and OK or MISMATCH last; exit status 1 on a mismatch."""
import ctypes
import sys

sys.path.insert(0, sys.argv[1])
import numpy as np  # noqa: E402
import torch  # noqa: E402

import msm_blst_amd as m  # noqa: E402

SHAPES = [(1, 12), (2, 10)]  # group, log2 n


def scalar_sets(n, K, where):
    raw = b"".join(m.gen_scalars(n, 1 if k == 0 else 900 + k) for k in range(K))
    if where == "pageable":
        return raw, raw, False
    t = torch.frombuffer(bytearray(raw), dtype=torch.uint8)
    t = t.to("cuda:0") if where == "device" else t.pin_memory()
    return raw, t, where == "device"


def batch_twice(ctx, group, raw, src, on_device, K, n, **kw):
    """two batches on one context, each between two synchronisations, against the synchronous MSM"""
    want = [m.compress(group, ctx.mult(raw[k * 32 * n:(k + 1) * 32 * n], **kw)) for k in range(K)]
    ok = True
    for _ in range(2):
        torch.cuda.synchronize()
        got = ctx.mult_batch(src if isinstance(src, bytes) else src.data_ptr(), K, on_device=on_device, **kw)
        torch.cuda.synchronize()
        ok &= [m.compress(group, g) for g in got] == want
    return ok


def sync_cases():
    """one synchronous MSM per engine; every result equal to the plain engine's"""
    ok = True
    for group, lg in SHAPES:
        n = 1 << lg
        pts, sc = m.fixed_points(group, n), m.gen_scalars(n, 1)
        ref = m.MSMContext(group, 0, 10)
        ref.set_points(pts, n)
        want = m.compress(group, ref.mult(sc, nbits=255))
        ref.close()
        got = {}
        ches = m.CHESContext(group, 0, n_exp=lg)
        ches.build_table(pts, n)
        got["ches"] = m.compress(group, ches.mult(sc))
        ches.close()
        if group == 1:
            bgmw = m.BGMWContext(group, 0, n_exp=lg)
            bgmw.build_table(pts, n)
            got["bgmw"] = m.compress(group, bgmw.mult(sc))
            bgmw.close()
            S = (ctypes.c_uint8 * len(sc)).from_buffer_copy(bytes(sc))
            pp = (ctypes.c_void_p * 2)(ctypes.cast(pts, ctypes.c_void_p), None)
            sp = (ctypes.c_void_p * 2)(ctypes.cast(S, ctypes.c_void_p), None)
            r = (ctypes.c_uint8 * 144)()
            m.lib().blst_p1s_mult_pippenger(r, pp, n, sp, 255, None)
            got["dropin"] = m.compress(group, r)
        for name, g in got.items():
            print(f"CALL sync {name} G{group} n=2^{lg} {'ok' if g == want else 'MISMATCH'}", flush=True)
            ok &= g == want
    return ok


def main():
    kind = sys.argv[2]
    if kind == "sync":
        torch.cuda.init()
        ok = sync_cases()
        print("OK" if ok else "MISMATCH")
        return 0 if ok else 1
    K = int(sys.argv[3]) if len(sys.argv) > 3 else 19
    wheres = sys.argv[4:] or ["device", "pinned"]
    ok = True
    torch.cuda.init()  # torch's HIP runtime before the engine's (tests/conftest.py)
    for group, lg in SHAPES:
        n = 1 << lg
        if kind == "plain":
            ctx = m.MSMContext(group, 0, 10)
            ctx.set_points(m.fixed_points(group, n), n)
            kw = {"nbits": 255}
        elif kind == "segments":  # two shards on one device: two segments per set
            ctx = m.CHESContext(group, n_exp=lg - 1, devices=[0, 0])
            ctx.build_table(m.fixed_points(group, n), n)
            kw = {}
        else:
            ctx = m.CHESContext(group, 0, n_exp=lg)
            ctx.build_table(m.fixed_points(group, n), n)
            kw = {}
            if kind == "profile":
                ctx.set_profiling(True)
        for where in wheres:
            if kind == "segments" and where == "device":
                continue  # a sharded context takes its scalars from host memory
            raw, src, on_device = scalar_sets(n, K, where)
            good = batch_twice(ctx, group, raw, src, on_device, K, n, **kw)
            lanes = ctx.batch_lanes() if kind != "plain" else 2
            print(f"CALL {kind} G{group} n=2^{lg} K={K} {where} lanes={lanes} {'ok' if good else 'MISMATCH'}", flush=True)
            ok &= good
        ctx.close()
    print("OK" if ok else "MISMATCH")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
