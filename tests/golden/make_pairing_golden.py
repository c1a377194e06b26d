#!/usr/bin/env python3
"""Golden fixture for the bulk pairings (ref src/pairing.c:181-262 and 371-404),
written from the REFERENCE itself: oracle/_ref/libblst_ref.so (built by
oracle/Makefile) is called through ctypes -- blst_miller_loop, blst_fp12_mul,
blst_final_exp, blst_fp12_is_one and, for the input points, blst_p{1,2}_mult /
blst_p{1,2}_to_affine -- on the inputs of tests/pairing_inputs.py.  Runs only in
the build container, on the CPU.

Writes tests/golden/pairing.json:
  pairs     per pair of pairing_inputs.pairs(): the reference's raw Miller value
            ("ml") and its pairing ("e"): hex in full for the first 8, an FNV-1a 64
            of the 576 bytes for the rest; the pairs with infinity give one
  segments  per layout of pairing_inputs.SEGMENTS and segment: fe(prod ml), hex
  tower     per special value of pairing_inputs.special_fp12(): the reference's
            blst_fp12_mul, _sqr, _inverse, _conjugate, _frobenius_map (1 .. 3),
            _mul_by_xy00z0 (the binary ones with "rand" as the second operand, the
            sparse one with its coefficients 0, 1, 4), _cyclotomic_sqr of the value's
            final exponentiation (FNV-1a 64 each) and blst_final_exp (hex); and that
            the reference's final exponentiation of zero is zero
While writing, the script asserts that the Python model agrees with the reference
on every input point, every pairing, every segment and every tower entry.
Test infrastructure only; data, no reference source text.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))

import pairing_inputs as pi  # noqa: E402

FULL = 8


def _buf(b):
    return (ctypes.c_uint8 * len(b)).from_buffer_copy(bytes(b))


def ref_point(L, g, k):
    """[k] generator through the reference, affine bytes"""
    gen = _buf(pi.ei.affine_bytes(g, pi.ei.GEN[g]))
    jac = (ctypes.c_uint8 * (144 * g))()
    getattr(L, f"blst_p{g}_from_affine")(jac, gen)
    out = (ctypes.c_uint8 * (144 * g))()
    sc = _buf(k.to_bytes(32, "little"))
    getattr(L, f"blst_p{g}_mult")(out, jac, sc, ctypes.c_size_t(255))
    aff = (ctypes.c_uint8 * (96 * g))()
    getattr(L, f"blst_p{g}_to_affine")(aff, out)
    return bytes(aff)


def ref_miller(L, pb, qb):
    out = (ctypes.c_uint8 * 576)()
    L.blst_miller_loop(out, _buf(qb), _buf(pb))
    return bytes(out)


def ref_mul(L, a, b):
    out = (ctypes.c_uint8 * 576)()
    L.blst_fp12_mul(out, _buf(a), _buf(b))
    return bytes(out)


def ref_fe(L, f):
    out = (ctypes.c_uint8 * 576)()
    L.blst_final_exp(out, _buf(f))
    return bytes(out)


def ref_tower(L, a, b):
    """the ten reference results on the Fp12 bytes a (second operand b), in the order of TOWER_OPS"""
    def call(name, *args):
        out = (ctypes.c_uint8 * 576)()
        getattr(L, name)(out, *args)
        return bytes(out)

    conj = _buf(a)
    L.blst_fp12_conjugate(conj)  # (in place)
    xyz = b[0:192] + b[4 * 96:5 * 96]  # a blst_fp6 (x, y, z): coefficients 0, 1 and 4 of b
    fe = call("blst_final_exp", _buf(a))
    return [call("blst_fp12_mul", _buf(a), _buf(b)), call("blst_fp12_sqr", _buf(a)),
            call("blst_fp12_inverse", _buf(a)), bytes(conj)] + [
            call("blst_fp12_frobenius_map", _buf(a), ctypes.c_size_t(k)) for k in (1, 2, 3)] + [
            call("blst_fp12_mul_by_xy00z0", _buf(a), _buf(xyz)), call("blst_fp12_cyclotomic_sqr", _buf(fe)), fe]


def tower(L):
    sp = pi.special_fp12()
    b = sp["rand"]
    out = {}
    for name in pi.SPECIAL_NAMES:
        ref = ref_tower(L, pi.fp12_bytes(sp[name]), pi.fp12_bytes(b))
        model = pi.tower_model(sp[name], b)
        for op, r, m in zip(pi.TOWER_OPS, ref, model):
            assert r == pi.fp12_bytes(m), ("tower", name, op)
        assert (L.blst_fp12_is_one(_buf(ref[-1])) == 1) == (name in pi.SPECIAL_FE_ONE), ("fe is one", name)
        out[name] = {op: (r.hex() if op == "final_exp" else pi.fnv(r)) for op, r in zip(pi.TOWER_OPS, ref)}
        print("tower", name, flush=True)
    zero = ref_fe(L, bytes(576))
    return {"values": out, "final_exp_of_zero_is_zero": zero == bytes(576)}


def main():
    L = ctypes.CDLL(os.path.join(REPO, "oracle", "_ref", "libblst_ref.so"))
    L.blst_fp12_is_one.restype = ctypes.c_int
    ps = pi.pairs()
    ks = pi.mi.gen_scalars(2 * pi.N_RANDOM, 0x9a1712)
    for i in range(pi.N_RANDOM):  # the model's input points are the reference's
        assert ref_point(L, 1, ks[2 * i]) == pi.ei.affine_bytes(1, ps[i][0]), ("p1", i)
        assert ref_point(L, 2, ks[2 * i + 1]) == pi.ei.affine_bytes(2, ps[i][1]), ("p2", i)
    one = pi.fp12_one()
    assert L.blst_fp12_is_one(_buf(one)) == 1
    ml, e = [], []
    for i in range(pi.N_PAIRS):
        pb, qb = pi.pair_bytes([i])
        m = ref_miller(L, pb, qb)
        v = ref_fe(L, m)
        assert pi.fp12_bytes(pi.pairing(*ps[i])) == v, ("pairing", i)
        if i in pi.INF_PAIRS:
            assert m == one and v == one, ("infinity", i)
        else:
            assert L.blst_fp12_is_one(_buf(v)) == 0
        ml.append(m)
        e.append(v)
        print("pair", i, flush=True)
    segs = {}
    for name, layout in pi.SEGMENTS.items():
        res = []
        for seg in layout:
            acc = one
            for i in seg:
                acc = ref_mul(L, acc, ml[i])
            v = ref_fe(L, acc)
            assert pi.fp12_bytes(pi.pairing_product([ps[i] for i in seg])) == v, (name, seg)
            res.append(v.hex())
        segs[name] = res
        print(name, len(res), flush=True)

    tw = tower(L)

    def ent(b, i):
        return b.hex() if i < FULL else pi.fnv(b)

    with open(os.path.join(HERE, "pairing.json"), "w") as f:
        json.dump({"source": "reference libblst (oracle/_ref/libblst_ref.so) blst_miller_loop / blst_fp12_mul / "
                             "blst_final_exp on the inputs of tests/pairing_inputs.py (pairs(), SEGMENTS); ml = the "
                             "raw Miller value, e = the pairing, 576 bytes in blst's layout: hex for the first 8 "
                             "pairs and every segment, FNV-1a 64 for the rest; tower = blst_fp12_mul / _sqr / "
                             "_inverse / _conjugate / _frobenius_map / _mul_by_xy00z0 / _cyclotomic_sqr (FNV-1a 64) "
                             "and blst_final_exp (hex) on pairing_inputs.special_fp12(), second operand 'rand', "
                             "cyclotomic_sqr taken on the value's final exponentiation",
                   "pairs": [{"ml": ent(ml[i], i), "e": ent(e[i], i)} for i in range(pi.N_PAIRS)],
                   "segments": segs, "tower": tw}, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
