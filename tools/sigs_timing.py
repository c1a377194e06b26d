"""Bulk signature verification (msm_sigs_verify, msm_sigs_batch_verify) of n = 2^lg
min-pk signatures, device resident: the individual checks (affine and compressed
inputs), the same signatures as ONE batch and as batches of 64 with 64-bit weights,
and the stitched chain of the separate calls on the same inputs in the same run
(msm_points_decode of keys and signatures with the group check, msm_points_hash, the
interleaving of the pairs with torch, msm_pairing_segments for the verdicts) -- the
comparison that matters.  Times are between device events around the call(s) on their
stream (median of 5 after 2 warm-ups).  The Fp-mul rate is what msm_valu_probe measures
in this run; the Fp products per signature as built are derived from the counts of the
engines' own timing tools (decode, hash-to-curve, points_mult, point_segments,
pairing) and stand beside the measurement.  The signatures are made by the library
(ps_mult on the hashed messages) from seeded keys.  Prints one JSON line.

usage: python tools/sigs_timing.py [lg=16] [--out file.json]   (default profiles/sigs_timing.json)"""
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import decode_timing  # noqa: E402
import hash_to_curve_timing  # noqa: E402
import pairing_timing  # noqa: E402
import points_segments_timing  # noqa: E402

WARMUP, SAMPLES = 2, 5
MSG_LEN, WBITS, BATCH = 32, 64, 64
TAG = b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_NUL_"


def products_as_built(n, piece, sum_piece=64):
    """Fp products per signature (min-pk) of each form, from the engines' own counts"""
    screen = {1: decode_timing.products_as_built(1, True) - decode_timing.products_as_built(1, False),
              2: decode_timing.products_as_built(2, True) - decode_timing.products_as_built(2, False)}
    dec = {g: decode_timing.products_as_built(g, False) for g in (1, 2)}
    h2c = hash_to_curve_timing.products_as_built(2, 2)["total"]
    pr = pairing_timing.products_as_built(piece)
    ml, fe, mul12 = pr["miller_per_pair"], pr["final_exp"], pr["fp12_mul"]
    mult_g1 = points_segments_timing.mult_products(1, n, WBITS)

    def sig_sum(seg):
        return points_segments_timing.products_as_built(2, n, seg, max(1, min(seg, sum_piece)), WBITS)

    front = screen[1] + screen[2] + h2c
    out = {"screen_g1": screen[1], "screen_g2": screen[2], "decode_g1": dec[1], "decode_g2": dec[2], "hash_g2": h2c,
           "miller_per_pair": ml, "final_exp": fe, "mult_g1_64bit": mult_g1,
           "individual": front + 2 * ml + mul12 + fe,
           "individual_encoded": front + dec[1] + dec[2] + 2 * ml + mul12 + fe}
    for name, seg in (("one_batch", n), (f"batches_of_{BATCH}", BATCH)):
        k = n // seg
        out[name] = front + mult_g1 + sig_sum(seg) + ((n + k) * ml + n * mul12 / max(piece, 1) + k * fe) / n
    return {k: round(v, 1) for k, v in out.items()}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    lg = int(args[0]) if args else 16
    out_path = (sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv
                else os.path.join(REPO, "profiles", "sigs_timing.json"))
    n = 1 << lg
    import torch
    torch.cuda.init()  # before the engine's library initialises HIP
    import msm_blst_amd as m
    import enc_inputs as ei
    L = m.lib()
    probe = (ctypes.c_double * 4)()
    m.check(L.msm_valu_probe(0, probe))
    rate = probe[1]
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0x5167)
    up = lambda t: t.to(dev)  # noqa: E731
    d_sk = up(torch.randint(0, 256, (n, 32), dtype=torch.uint8, generator=gen))
    d_sk[:, 31] &= 0x3f  # below r
    d_msgs = up(torch.randint(0, 256, (n * MSG_LEN,), dtype=torch.uint8, generator=gen))
    d_w = up(torch.randint(0, 256, (n, WBITS // 8), dtype=torch.uint8, generator=gen))
    d_w[:, 0] |= 1
    d_g1 = up(torch.frombuffer(bytearray(ei.affine_bytes(1, ei.GEN[1])), dtype=torch.uint8))
    neg = ei.affine_bytes(1, (ei.GEN[1][0], -ei.GEN[1][1] % ei.P))
    d_neg = up(torch.frombuffer(bytearray(neg), dtype=torch.uint8))
    z = lambda *shape: torch.zeros(*shape, dtype=torch.uint8, device=dev)  # noqa: E731
    d_pk, d_hm, d_sig = z(n * 96), z(n * 192), z(n * 192)
    d_pkc, d_sigc = z(n * 48), z(n * 96)
    d_pk2, d_sig2 = z(n * 96), z(n * 192)
    d_p, d_q = z(n, 2, 96), z(n, 2, 192)
    st = torch.cuda.Stream(device=dev)
    s = st.cuda_stream
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        m.ps_mult(1, d_g1.data_ptr(), d_sk.data_ptr(), n, one_point=True, src_on_device=True, dst=d_pk.data_ptr(), stream=s)
        m.ps_hash_to_curve(2, d_msgs.data_ptr(), dst_tag=TAG, msg_len=MSG_LEN, n=n, src_on_device=True,
                           dst=d_hm.data_ptr(), stream=s)
        m.ps_mult(2, d_hm.data_ptr(), d_sk.data_ptr(), n, src_on_device=True, dst=d_sig.data_ptr(), stream=s)
        m.ps_encode(1, d_pk.data_ptr(), n, src_on_device=True, dst=d_pkc.data_ptr(), stream=s)
        m.ps_encode(2, d_sig.data_ptr(), n, src_on_device=True, dst=d_sigc.data_ptr(), stream=s)
    st.synchronize()
    status = (ctypes.c_uint8 * n)()
    nfail = ctypes.c_size_t(0)

    def timed(fn):
        ts = []
        for k in range(WARMUP + SAMPLES):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(st):
                e0.record(st)
                fn()
                e1.record(st)
            st.synchronize()
            if k >= WARMUP:
                ts.append(e0.elapsed_time(e1))
        return round(statistics.median(ts), 3), round(max(ts) - min(ts), 3)

    def verify(encoded):
        pk, sg = (d_pkc, d_sigc) if encoded else (d_pk, d_sig)
        m.check(L.msm_sigs_verify(1, 0, status, ctypes.byref(nfail), pk.data_ptr(), None, sg.data_ptr(),
                                  d_msgs.data_ptr(), None, MSG_LEN, None, 0, n, TAG, len(TAG),
                                  m.SIG_ENCODED if encoded else 0, 1, s))

    def batch(seg, count=None):
        k = (count if count is not None else n) // seg
        o = (ctypes.c_size_t * (k + 1))(*range(0, k * seg + 1, seg))

        def run():
            m.check(L.msm_sigs_batch_verify(1, 0, status, ctypes.byref(nfail), d_pk.data_ptr(), d_sig.data_ptr(),
                                            d_w.data_ptr(), WBITS, WBITS // 8, d_msgs.data_ptr(), None, MSG_LEN, None, 0,
                                            o, k, TAG, len(TAG), 0, 1, s))
        return run, k

    o2 = (ctypes.c_size_t * (n + 1))(*range(0, 2 * n + 1, 2))
    st_k, st_s = (ctypes.c_uint8 * n)(), (ctypes.c_uint8 * n)()
    verdict = (ctypes.c_uint8 * n)()

    def stitched():
        m.check(L.msm_points_decode(1, 0, d_pk2.data_ptr(), st_k, None, d_pkc.data_ptr(), n, 0, 1, 1, 1, s))
        m.check(L.msm_points_decode(2, 0, d_sig2.data_ptr(), st_s, None, d_sigc.data_ptr(), n, 0, 1, 1, 1, s))
        m.check(L.msm_points_hash(2, 0, d_hm.data_ptr(), d_msgs.data_ptr(), None, MSG_LEN, None, 0, n, TAG, len(TAG), 0, 1,
                                  1, s))
        d_p[:, 0] = d_pk2.view(n, 96)
        d_p[:, 1] = d_neg
        d_q[:, 0] = d_hm.view(n, 192)
        d_q[:, 1] = d_sig2.view(n, 192)
        m.check(L.msm_pairing_segments(0, None, verdict, None, d_p.data_ptr(), d_q.data_ptr(), o2, n, 0, 1, 0, s))

    piece = L.msm_pairing_piece(2 * n)
    sum_piece = L.msm_segments_piece(2, n)
    out = {"n": n, "scheme": "min-pk", "fp_mul_per_s": rate, "warmup": WARMUP, "samples": SAMPLES, "msg_len": MSG_LEN,
           "weight_bits": WBITS, "pairing_piece": piece, "sum_piece": sum_piece,
           "products_per_signature_as_built": products_as_built(n, piece, sum_piece)}
    all_ok = True

    def entry(ms, spread, key, ok):
        pred = n * out["products_per_signature_as_built"][key] / rate * 1e3
        return {"device_resident_ms": ms, "spread_ms": spread, "us_per_signature": round(ms * 1e3 / n, 3),
                "predicted_valu_ms": round(pred, 3), "measured_over_predicted": round(ms / pred, 2),
                "all_verified": bool(ok)}

    ms, sp = timed(lambda: verify(False))
    ok = bytes(status) == bytes(n) and nfail.value == 0
    out["individual"] = entry(ms, sp, "individual", ok)
    all_ok &= ok
    ms, sp = timed(lambda: verify(True))
    ok = bytes(status) == bytes(n)
    out["individual_encoded"] = entry(ms, sp, "individual_encoded", ok)
    all_ok &= ok
    for name, seg in (("one_batch", n), (f"batches_of_{BATCH}", BATCH)):
        run, k = batch(seg)
        ms, sp = timed(run)
        ok = bytes(status[:k]) == bytes(k)
        out[name] = entry(ms, sp, name, ok)
        out[name]["batches"] = k
        all_ok &= ok
    # the same batches at pairing pieces of 3: n + k pairs in pieces of 2 are one piece more than the lane
    # pairs the chip holds at once (pairing.hpp), pieces of 3 fit in one round
    os.environ["MSM_PAIRING_PIECE"] = "3"
    pr3 = products_as_built(n, 3, sum_piece)
    for name, seg in (("one_batch", n), (f"batches_of_{BATCH}", BATCH)):
        run, k = batch(seg)
        ms, sp = timed(run)
        ok = bytes(status[:k]) == bytes(k)
        pred = n * pr3[name] / rate * 1e3
        out[name + "_piece3"] = {"device_resident_ms": ms, "spread_ms": sp, "us_per_signature": round(ms * 1e3 / n, 3),
                                 "products_per_signature_as_built": pr3[name], "predicted_valu_ms": round(pred, 3),
                                 "measured_over_predicted": round(ms / pred, 2), "all_verified": bool(ok)}
        all_ok &= ok
    del os.environ["MSM_PAIRING_PIECE"]
    # batches of 63: 1024 of them are 64512 tuples and exactly 2^16 pairs, one chunk of the pairing call;
    # the 2^16 + k pairs of the batches above leave a small second chunk that pays a whole pass
    run, k = batch(BATCH - 1, 1024 * (BATCH - 1))
    ms, sp = timed(run)
    ok = bytes(status[:k]) == bytes(k)
    out[f"batches_of_{BATCH - 1}_one_pairing_chunk"] = {"tuples": k * (BATCH - 1), "batches": k, "device_resident_ms": ms,
                                                        "spread_ms": sp,
                                                        "us_per_signature": round(ms * 1e3 / (k * (BATCH - 1)), 3),
                                                        "all_verified": bool(ok)}
    all_ok &= ok
    ms, sp = timed(stitched)
    ok = bytes(verdict) == b"\x01" * n and not any(st_k) and not any(st_s)
    out["stitched_chain_encoded"] = {"device_resident_ms": ms, "spread_ms": sp, "us_per_signature": round(ms * 1e3 / n, 3),
                                     "all_verified": bool(ok),
                                     "calls": "decode G1 + decode G2 (group check) + hash + torch interleave + pairing check"}
    all_ok &= ok
    out["single_call_over_stitched"] = round(out["individual_encoded"]["device_resident_ms"] / ms, 3)
    out["one_batch_over_individual"] = round(out["one_batch"]["device_resident_ms"] /
                                             out["individual"]["device_resident_ms"], 3)
    # one forged signature is found by both forms
    d_sig.view(n, 192)[n // 3] = d_sig.view(n, 192)[n // 3 + 1]
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        verify(False)
        ind = bytes(status)
        batch(n)[0]()
        bat = status[0]
    st.synchronize()
    ok = ind == bytes(5 if j == n // 3 else 0 for j in range(n)) and bat == 5
    out["forgery_found"] = bool(ok)
    all_ok &= ok
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")
    if not all_ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
