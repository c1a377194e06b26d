"""Device-resident timing of the evaluation-form polynomial call and the KZG layer
(msm_fr_eval_quotient, msm_kzg_*) at n = 2^12 x 256 polynomials and n = 2^20 x 1:
the device time (device events around the call on its stream, median of 5 after 2
warm-ups) of
  eval_quotient        with and without q, each beside
      predicted_valu_ms   the Fr products as built (products_per_element below) at the
                          rate msm_fr_probe measures in this run
      hbm_floor_ms        the bytes it moves (f read; with q also d written, then f and d
                          read and q written) at the rate of a device copy timed in
                          this run
      over_larger         the measured time over the larger of the two
  commit, open         and, beside open, the stitched chain it replaces:
                       fr_eval_quotient into a device buffer, then MSMContext.mult_batch
                       on the same scalars; eval_quotient_share = the kernel's part of it;
                       the batch MSM alone is timed before commit and after the chain
  verify               2^12 honest tuples (made here by commit / open on an n = 16 SRS),
                       one by one and as one weighted batch
The SRS at 2^12 is a real one ([l_i(tau)]G1 by ps_mult from tests/kzg_inputs.py) and the
first results are checked against the oracle; the 2^20 SRS is 2^20 multiples of the
generator by random scalars, enough for timing.  What a sitting does not measure
is written as "not measured".  Prints one JSON line.

usage: python tools/kzg_timing.py [--out file.json]   (default profiles/kzg_timing.json)"""
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import enc_inputs as ei  # noqa: E402
import fr_inputs as fi  # noqa: E402
import kzg_inputs as ki  # noqa: E402

WARMUP, SAMPLES = 2, 5
EL, P1 = 32, 96
FERMAT = 256 + bin(fi.R - 2).count("1")  # the chain as built: a squaring per bit of four words, a product per set bit


def products_per_element(log_n, with_q):
    """Fr products per element of csrc/fr_poly.hip at the default tile (2^10, four per lane):
    prefix 3/4, back-substitution 6/4, the two sums 2, the tree over 256 lanes up and down
    765 / 1024, the Fermat chain once per tile, the two-level domain table above 2^12,
    the quotient"""
    tile = min(1 << log_n, 1024)
    return 3 / 4 + 6 / 4 + 2 + 765 / 1024 + FERMAT / tile + (1 if log_n > 12 else 0) + (1 if with_q else 0)


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


def window_for(n):
    """the bucket window msm_kzg_ctx_create picks (csrc/abi.cpp auto_window)"""
    lg = n.bit_length() - 1
    return 8 if lg <= 8 else 10 if lg <= 10 else 12 if lg <= 12 else 13 if lg == 13 else 14 if lg <= 16 else 16


def main():
    out_path = (sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv
                else os.path.join(REPO, "profiles", "kzg_timing.json"))
    import torch
    torch.cuda.init()  # before the engine's library initialises HIP
    import msm_blst_amd as m
    rate, probe_ms = m.fr_probe()
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)
    gen = ei.affine_bytes(1, ei.GEN[1])
    tau_g2 = ki.p2_bytes(ki.g2(ki.TAU))

    def up(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    out = {"fr_mul_per_s": rate, "probe_ms": round(probe_ms, 3), "warmup": WARMUP, "samples": SAMPLES,
           "fermat_chain_products": FERMAT}
    ok = True
    for log_n, count in ((12, 256), (20, 1)):
        n = 1 << log_n
        total = n * count
        # distinct values everywhere (repeated scalars would pile into a few buckets of the MSM):
        # SplitMix64 scalars below r, turned into blst_fr on the device
        raw = bytes(m.gen_scalars(total, 7))
        base = fi.unpack(raw[:n * EL], scalar=True)
        d_f = up(raw)
        m.fr_op("from_scalar", d_f.data_ptr(), None, total, src_on_device=True, dst=d_f.data_ptr())
        zs = fi.rand_values(count, 8)
        d_z = up(fi.pack(zs))
        d_y = torch.zeros(count * EL, dtype=torch.uint8, device=dev)
        d_q = torch.zeros(total * EL, dtype=torch.uint8, device=dev)
        d_p = torch.zeros(count * P1, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        copy_ms = timed(torch, st, lambda: d_q.copy_(d_f, non_blocking=True))
        g = {"log_n": log_n, "polynomials": count, "copy_ms": round(copy_ms, 3),
             "copy_GBps": round(2 * total * EL / copy_ms / 1e6, 1)}
        for with_q, copies in ((False, 0.5), (True, 2.5)):
            ms = timed(torch, st, lambda: m.fr_eval_quotient(
                d_f.data_ptr(), d_z.data_ptr(), log_n, count, want_q=with_q, dst_scalar=True, src_on_device=True,
                y_dst=d_y.data_ptr(), q_dst=d_q.data_ptr(), stream=st.cuda_stream))
            per = products_per_element(log_n, with_q)
            e = {"device_resident_ms": round(ms, 3), "products_per_element_as_built": round(per, 2),
                 "predicted_valu_ms": round(total * per / rate * 1e3, 3), "hbm_floor_ms": round(copies * copy_ms, 3)}
            e["over_larger"] = round(ms / max(e["predicted_valu_ms"], e["hbm_floor_ms"]), 2)
            g["eval_quotient_with_q" if with_q else "eval_quotient_y_only"] = e
        if log_n == 12:  # the first polynomial against the oracle (y, and the quotient's scalars)
            wy, wq = ki.eval_quot(base, zs[0], log_n)
            good = bytes(d_y[:EL].cpu().numpy()) == fi.fr_bytes(wy) and \
                bytes(d_q[:n * EL].cpu().numpy()) == fi.pack(wq, scalar=True)
            g["outputs_equal_expected"] = good
            ok = ok and good
            lag = ki.lagrange_at(ki.TAU, log_n)
            srs = m.ps_mult(1, gen, fi.pack(lag, scalar=True), n, one_point=True)
        else:
            srs = m.ps_mult(1, gen, bytes(m.gen_scalars(n, 3)), n, one_point=True)
        d_srs = up(srs)
        torch.cuda.synchronize()
        ctx = m.KZGContext(log_n, d_srs.data_ptr(), tau_g2, srs_on_device=True)
        plain = m.MSMContext(1, 0, window_for(n))
        plain.set_points(d_srs.data_ptr(), n, on_device=True)
        # the batch MSM alone, before and after the calls built on it: the spread between the two
        # is the drift of the sitting (clocks, the box), not a property of either call
        g["msm_batch_alone_before_ms"] = round(timed(torch, st, lambda: plain.mult_batch(
            d_f.data_ptr(), count, on_device=True, stream=st.cuda_stream)), 3)
        g["commit_ms"] = round(timed(torch, st, lambda: ctx.commit(
            d_f.data_ptr(), count, src_on_device=True, dst=d_p.data_ptr(), stream=st.cuda_stream)), 3)
        g["open_ms"] = round(timed(torch, st, lambda: ctx.open(
            d_f.data_ptr(), d_z.data_ptr(), count, src_on_device=True, proofs_dst=d_p.data_ptr(), y_dst=d_y.data_ptr(),
            stream=st.cuda_stream)), 3)
        if log_n == 12:
            k = (ki.eval_at(base, lag) - wy) * ki.inv0(ki.TAU - zs[0]) % fi.R
            good = bytes(d_p[:P1].cpu().numpy()) == ki.p1_bytes(ki.g1(k))
            g["proof_equals_expected"] = good
            ok = ok and good

        def chain():
            m.fr_eval_quotient(d_f.data_ptr(), d_z.data_ptr(), log_n, count, dst_scalar=True, src_on_device=True,
                               y_dst=d_y.data_ptr(), q_dst=d_q.data_ptr(), stream=st.cuda_stream)
            plain.mult_batch(d_q.data_ptr(), count, on_device=True, stream=st.cuda_stream)

        g["stitched_chain_ms"] = round(timed(torch, st, chain), 3)
        g["msm_batch_alone_ms"] = round(timed(torch, st, lambda: plain.mult_batch(
            d_q.data_ptr(), count, on_device=True, stream=st.cuda_stream)), 3)
        g["eval_quotient_share_of_open"] = round(g["eval_quotient_with_q"]["device_resident_ms"] / g["open_ms"], 3)
        ctx.close()
        plain.close()
        out[f"n_2^{log_n}_x_{count}"] = g

    # ---- verify: 2^12 honest tuples on an n = 16 SRS ----
    k, log_n = 1 << 12, 4
    lag = ki.lagrange_at(ki.TAU, log_n)
    ctx = m.KZGContext(log_n, m.ps_mult(1, gen, fi.pack(lag, scalar=True), 16, one_point=True), tau_g2)
    polys = fi.pack(fi.rand_values(16 * 64, 9)) * (k // 64)
    zs = fi.pack(fi.rand_values(k, 10))
    d_f, d_z = up(polys), up(zs)
    d_c = torch.zeros(k * P1, dtype=torch.uint8, device=dev)
    d_p = torch.zeros(k * P1, dtype=torch.uint8, device=dev)
    d_y = torch.zeros(k * EL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.commit(d_f.data_ptr(), k, src_on_device=True, dst=d_c.data_ptr(), stream=st.cuda_stream)
    ctx.open(d_f.data_ptr(), d_z.data_ptr(), k, src_on_device=True, proofs_dst=d_p.data_ptr(), y_dst=d_y.data_ptr(),
             stream=st.cuda_stream)
    st.synchronize()
    w = bytes(m.gen_scalars(k, 11))
    res = {}

    def each():
        res["each"] = ctx.verify(d_c.data_ptr(), d_z.data_ptr(), d_y.data_ptr(), d_p.data_ptr(), k, src_on_device=True,
                                 stream=st.cuda_stream)

    def batch():
        res["batch"] = ctx.verify(d_c.data_ptr(), d_z.data_ptr(), d_y.data_ptr(), d_p.data_ptr(), k, weights=w,
                                  nbits=64, stride=32, src_on_device=True, stream=st.cuda_stream)

    v = {"tuples": k, "each_ms": round(timed(torch, st, each), 3), "one_weighted_batch_ms": round(timed(torch, st, batch), 3)}
    v["all_hold"] = res["each"] == bytes([1] * k) and res["batch"] == bytes([1])
    ok = ok and v["all_hold"]
    ctx.close()
    out["verify"] = v
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
