#!/usr/bin/env python3
"""Golden fixture for the bulk hash-to-curve (ref src/map_to_g1.c:285-453,
src/map_to_g2.c:173-401, src/hash_to_field.c:51-154), written from the
REFERENCE itself: oracle/_ref/libblst_ref.so (built by oracle/Makefile) is
called through ctypes -- blst_hash_to_g{1,2}, blst_encode_to_g{1,2},
blst_map_to_g{1,2} and blst_p{1,2}_to_affine, one message at a time, on the
inputs of tests/h2c_inputs.py.  Runs only in the build container, on the CPU.

Writes tests/golden/hash_to_curve.json: per group
  mixed    the 131-message batch under the standard DST, {"hash", "encode"}: per
           message the compressed point and an FNV-1a 64 of its affine bytes
  cases    the 8-message cases (DST lengths 0 / 255 / 256 / 300, aug of 48 / 96
           bytes, fixed 32-byte messages), hashed
  map1/2   blst_map_to_g{1,2} on the special u values, count 1 and 2
  fields   hash_to_field (count 2) of the first 16 messages, blst layout, hex
While writing, the script asserts that the Python model of h2c_inputs.py agrees
with the reference on every entry; the field elements are tied to the reference
by mapping them with its own blst_map_to_g{1,2}, which must give its own
blst_hash_to_g{1,2}, and by its blst_expand_message_xmd.
Test infrastructure only; data, no reference source text.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))

import h2c_inputs as h  # noqa: E402

JAC = {1: 144, 2: 288}


def _buf(b):
    return (ctypes.c_uint8 * max(len(b), 1)).from_buffer_copy(bytes(b) or b"\0")


def ref_affine(L, g, jac):
    out = (ctypes.c_uint8 * h.AFF[g])()
    getattr(L, f"blst_p{g}_to_affine")(out, jac)
    # the reference leaves garbage x, y for Z = 0: infinity is the all-zero point here
    z = bytes(jac)[2 * 48 * g:]
    return bytes(h.AFF[g]) if not any(z) else bytes(out)


def ref_hash(L, g, msg, dst, aug, encode):
    jac = (ctypes.c_uint8 * JAC[g])()
    f = getattr(L, f"blst_{'encode' if encode else 'hash'}_to_g{g}")
    f(jac, _buf(msg), ctypes.c_size_t(len(msg)), _buf(dst), ctypes.c_size_t(len(dst)), _buf(aug),
      ctypes.c_size_t(len(aug)))
    return ref_affine(L, g, jac)


def ref_map(L, g, us):
    jac = (ctypes.c_uint8 * JAC[g])()
    u = _buf(h.mont_bytes(g, us[0]))
    v = _buf(h.mont_bytes(g, us[1])) if len(us) == 2 else None
    getattr(L, f"blst_map_to_g{g}")(jac, u, v)
    return ref_affine(L, g, jac)


def checked(g, ref_bytes, model_pt, what):
    assert h.affine_bytes(g, model_pt) == ref_bytes, what
    return h.entry(g, model_pt)


def main():
    L = ctypes.CDLL(os.path.join(REPO, "oracle", "_ref", "libblst_ref.so"))
    out = {}
    msgs = h.messages()
    for g in (1, 2):
        dst = h.DST[g]
        G = {"mixed": {}, "cases": {}}
        for encode in (False, True):
            ents = []
            for i, m in enumerate(msgs):
                ents.append(checked(g, ref_hash(L, g, m, dst, b"", encode), h.hash_to_curve(g, m, dst, b"", encode),
                                    (g, encode, i)))
            G["mixed"]["encode" if encode else "hash"] = ents
        for name in h.CASES:
            cm, cdst, caug, _ = h.case(g, name)
            ents = []
            for i, m in enumerate(cm):
                a = caug[i] if caug else b""
                ents.append(checked(g, ref_hash(L, g, m, cdst, a, False), h.hash_to_curve(g, m, cdst, a, False),
                                    (g, name, i)))
            G["cases"][name] = ents
        us, pairs = h.map_cases(g)
        G["map1"] = [checked(g, ref_map(L, g, [u]), h.map_to_curve(g, [u]), (g, "map1", k)) for k, u in enumerate(us)]
        G["map2"] = [checked(g, ref_map(L, g, list(p)), h.map_to_curve(g, list(p)), (g, "map2", k))
                     for k, p in enumerate(pairs)]
        assert any(e["c"].startswith("c0") for e in G["map2"]), "the u == -v pair gives infinity"
        fields = []
        for i, m in enumerate(msgs[:16]):
            el = h.hash_to_field(g, m, dst, 2)
            assert ref_map(L, g, el) == ref_hash(L, g, m, dst, b"", False), (g, "fields", i)
            uni = (ctypes.c_uint8 * (128 * g))()
            L.blst_expand_message_xmd(uni, ctypes.c_size_t(128 * g), _buf(m), ctypes.c_size_t(len(m)), _buf(dst),
                                      ctypes.c_size_t(len(dst)))
            assert bytes(uni) == h.expand_message_xmd(m, dst, 128 * g), (g, "xmd", i)
            fields.append(h.field_bytes(g, el).hex())
        G["fields"] = fields
        out[str(g)] = G
        print(g, {k: (len(v) if isinstance(v, list) else {kk: len(vv) for kk, vv in v.items()}) for k, v in G.items()},
              flush=True)
    with open(os.path.join(HERE, "hash_to_curve.json"), "w") as f:
        json.dump({"source": "reference libblst (oracle/_ref/libblst_ref.so) blst_hash_to_g{1,2} / blst_encode_to_g{1,2} / "
                             "blst_map_to_g{1,2} / blst_p{1,2}_to_affine on the inputs of tests/h2c_inputs.py "
                             "(messages(), case(g, name), map_cases(g)); per point c = the compressed encoding, "
                             "fnv = FNV-1a 64 of the affine bytes (infinity all zero)",
                   "groups": out}, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
