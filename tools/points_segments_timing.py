"""Segmented sums and MSMs (msm_points_msm_segments) of n = 2^lg device-resident
points, G1 and G2, cut into equal segments of 1, 16, 256, 4096 and n points: MSMs
at nbits = 255 and 64 and plain sums.  Per case the device time (device events
around the call on its stream) and the VALU prediction -- the field products per
point as built (products_as_built below) over the Fp-mul rate that msm_valu_probe
measures in this run.  In the same run msm_points_mult on the same points and
scalars: the way to do this job without the segmented call (and it still lacks the
sums).  A sweep of the piece length at segments of 4096 points shows what the
rule of segments_plan.hpp leaves on the table.  The points are a tile of 2^14
distinct fixed points, repeated; the scalars are SplitMix64 values below r.
Checked in the run: segments of one point against msm_points_mult (and the plain
sums against the points themselves), the one segment of n points against an
MSMContext and against blst_p{1,2}s_add.
Prints one JSON line.

usage: python tools/points_segments_timing.py [lg=20] [--out file.json]   (default profiles/points_segments_timing.json)"""
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import enc_inputs as ei  # noqa: E402

WARMUP, SAMPLES = 2, 7
TILE_LG = 14
SEG_LENGTHS = [1, 16, 256, 4096, None]  # None: one segment of n points
SWEEP_SEG, SWEEP_PIECES = 4096, [1, 2, 4, 8, 16, 32, 64]
MULT_CHUNK = 1 << 18
SEG_CHUNK_BUDGET, SEG_POINT_BYTES = 3 << 30, 8 * 112 + 7 * 224 + 224 + 72  # csrc/segments_plan.hpp


def _prices(group):
    mul, sqr, mulsub, lanes = (1, 1, 1.5, 1) if group == 1 else (3, 2, 5, 2)
    return mul, sqr, mulsub, lanes, 4 * mul + 3 * sqr + mulsub, 6 * mul + 2 * sqr + mulsub, 10 * mul + 2 * sqr + mulsub


def _tree(group, elems):
    """per element: up, prefix, back-substitution (2), the levels above, the leaf inversions (~575 each)"""
    mul, _, _, lanes = _prices(group)[:4]
    lv, e = [], elems
    while e:
        e = (e + 7) // 8
        lv.append(e)
        if e <= 256:
            break
    return mul * (4 + sum(4 * v for v in lv[:-1]) / elems) + lanes * 575 * lv[-1] / elems


def products_as_built(group, n, seg, piece, nbits):
    """Fp products per point of csrc/point_segments.hip (+ the table kernel of
    pm_common.hpp and the shared tree of to_affine.hip), priced as
    tools/points_mult_timing.py prices them: an fp_mul2 1.5 and an fp_mul4 2.5 Fp
    products; G2 counts both lanes of a pair.  seg: points per segment; piece: L;
    nbits None: plain sums."""
    mul, sqr, mulsub, lanes, dbl, madd, add = _prices(group)
    nseg = n // seg
    pieces = nseg * -(-seg // piece)
    c = min(n, SEG_CHUNK_BUDGET // (SEG_POINT_BYTES * group))
    merge = (pieces - nseg) / n * add
    out = nseg / n * (_tree(group, min(nseg, c)) + 2 * mul + sqr + lanes * 2)
    if nbits is None:
        return lanes * 2 + madd + merge + out
    nw = nbits // 4 + 1
    table = lanes * 2 + (2 * mul + 2 * sqr + dbl) + 6 * madd + 7 * (_tree(group, 7 * c) + 3 * mul + sqr)
    return table + nw * (15 / 16) * madd + (nw - 1) * 4 * dbl * pieces / n + merge + out


def mult_products(group, n, nbits):
    """msm_points_mult, per-point bases (tools/points_mult_timing.py products_as_built)"""
    mul, sqr, mulsub, lanes, dbl, madd, _ = _prices(group)
    nw = nbits // 4 + 1
    c = min(n, MULT_CHUNK)
    table = lanes * 2 + (2 * mul + 2 * sqr + dbl) + 6 * madd + 7 * (_tree(group, 7 * c) + 3 * mul + sqr)
    return (nw - 1) * 4 * dbl + nw * (15 / 16) * madd + _tree(group, c) + (2 * mul + sqr) + lanes * 2 + table


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    lg = int(args[0]) if args else 20
    out_path = (sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv
                else os.path.join(REPO, "profiles", "points_segments_timing.json"))
    n = 1 << lg
    tile = min(n, 1 << TILE_LG)
    for v in ("MSM_POINTS_SEGMENTS_PIECE", "MSM_POINTS_SEGMENTS_CHUNK"):
        os.environ.pop(v, None)
    import torch
    torch.cuda.init()  # before the engine's library initialises HIP (tests/conftest.py: torch found no device after it)
    import msm_blst_amd as m
    L = m.lib()
    probe = (ctypes.c_double * 4)()
    m.check(L.msm_valu_probe(0, probe))
    rate = probe[1]
    out = {"n": n, "fp_mul_per_s": rate, "warmup": WARMUP, "samples": SAMPLES, "input_tile": tile}
    dev = torch.device("cuda:0")
    sc = bytes(m.gen_scalars(n, 1))
    d_sc = torch.frombuffer(bytearray(sc), dtype=torch.uint8).to(dev)
    st = torch.cuda.Stream(device=dev)
    all_ok = True

    def timed(call):
        ts = []
        for s in range(WARMUP + SAMPLES):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(st):
                e0.record(st)
                m.check(call())
                e1.record(st)
            st.synchronize()
            if s >= WARMUP:
                ts.append(e0.elapsed_time(e1))
        return statistics.median(ts)

    def entry(ms, products):
        pred = n * products / rate * 1e3
        return {"products_per_point_as_built": round(products, 1), "device_resident_ms": round(ms, 3),
                "predicted_valu_ms": round(pred, 3), "device_resident_over_predicted": round(ms / pred, 2)}

    def split(e255, e64):
        """the two scalar widths run the same table, merge and output and differ by 47
        windows: the time of a window (the ladder) and what is left (the rest), each
        over the same split of the products as built"""
        w255, w64 = 255 // 4 + 1, 64 // 4 + 1
        per_w = (e255["device_resident_ms"] - e64["device_resident_ms"]) / (w255 - w64)
        pred_w = (e255["predicted_valu_ms"] - e64["predicted_valu_ms"]) / (w255 - w64)
        rest, pred_rest = e64["device_resident_ms"] - w64 * per_w, e64["predicted_valu_ms"] - w64 * pred_w
        return {"ladder_ms_per_window": round(per_w, 4), "ladder_over_predicted": round(per_w / pred_w, 2),
                "rest_ms": round(rest, 3), "rest_predicted_ms": round(pred_rest, 3)}

    for group in (1, 2):
        A = ei.AFF[group]
        aff = bytes(m.fixed_points(group, tile)) * (n // tile)
        d_pts = torch.frombuffer(bytearray(aff), dtype=torch.uint8).to(dev)
        d_dst = torch.zeros(n * A, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        g = {"piece_default": int(L.msm_segments_piece(group, n))}
        mult_out = {}
        for nbits in (255, 64):
            ms = timed(lambda: L.msm_points_mult(group, 0, d_dst.data_ptr(), d_pts.data_ptr(), d_sc.data_ptr(), n, nbits, 32,
                                                 0, 1, 1, st.cuda_stream))
            g[f"ps_mult_nbits{nbits}"] = entry(ms, mult_products(group, n, nbits))
            mult_out[nbits] = bytes(d_dst.cpu().numpy())

        def segments(seg, nbits, piece=None):
            k = n // seg
            offs = (ctypes.c_size_t * (k + 1))(*range(0, n + 1, seg))
            if piece is None:
                os.environ.pop("MSM_POINTS_SEGMENTS_PIECE", None)
            else:
                os.environ["MSM_POINTS_SEGMENTS_PIECE"] = str(piece)
            pl = int(L.msm_segments_piece(group, n))
            ms = timed(lambda: L.msm_points_msm_segments(group, 0, d_dst.data_ptr(), d_pts.data_ptr(),
                                                         d_sc.data_ptr() if nbits else None, offs, k, nbits or 0,
                                                         32 if nbits else 0, 0, 1, 1, st.cuda_stream))
            os.environ.pop("MSM_POINTS_SEGMENTS_PIECE", None)
            e = entry(ms, products_as_built(group, n, seg, pl, nbits))
            e["piece"] = pl
            return e, bytes(d_dst[:k * A].cpu().numpy())

        for seg in SEG_LENGTHS:
            name = "n" if seg is None else str(seg)
            seg = n if seg is None else seg
            if seg > n:
                continue
            for nbits in (255, 64, None):
                e, got = segments(seg, nbits)
                mode = "sums" if nbits is None else f"msm_nbits{nbits}"
                if nbits is not None:
                    ref = g[f"ps_mult_nbits{nbits}"]
                    e["ps_mult_ms_over_this"] = round(ref["device_resident_ms"] / e["device_resident_ms"], 2)
                    e["ps_mult_products_over_this"] = round(ref["products_per_point_as_built"] /
                                                            e["products_per_point_as_built"], 2)
                ok = None
                if seg == 1:
                    ok = got == (aff if nbits is None else mult_out[nbits])
                elif seg == n and nbits is None:
                    ok = got == m.to_affine(group, m.ps_add(group, aff, n))
                elif seg == n and nbits == 255:
                    ctx = m.MSMContext(group, 0, 0)
                    ctx.set_points(aff, n)
                    ok = ei.encode(group, got, 1) == m.compress(group, ctx.mult(sc, 255))
                    ctx.close()
                if ok is not None:
                    e["outputs_equal_expected"] = bool(ok)
                    all_ok = all_ok and ok
                g[f"seg{name}_{mode}"] = e
            g[f"seg{name}_split"] = split(g[f"seg{name}_msm_nbits255"], g[f"seg{name}_msm_nbits64"])
        g["ps_mult_split"] = split(g["ps_mult_nbits255"], g["ps_mult_nbits64"])
        if SWEEP_SEG <= n:
            want = None
            for piece in SWEEP_PIECES:
                e, got = segments(SWEEP_SEG, 255, piece)
                want = got if want is None else want
                e["outputs_equal_expected"] = bool(got == want)
                all_ok = all_ok and got == want
                g[f"sweep_seg{SWEEP_SEG}_msm_nbits255_piece{piece}"] = e
        out[f"g{group}"] = g
        del d_pts, d_dst
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")
    if not all_ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
