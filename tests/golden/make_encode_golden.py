#!/usr/bin/env python3
"""Golden fixture for the bulk point encoding (ref src/e1.c:139-234 and the
src/e2.c twins), written from the REFERENCE itself: oracle/_ref/libblst_ref.so
(built by oracle/Makefile) is called through ctypes -- blst_p{1,2}_affine_compress,
blst_p{1,2}_affine_serialize, blst_p{1,2}_compress and blst_p{1,2}_serialize, one
entry at a time, on the batches of tests/enc_special.py.  Runs only in the build
container, on the CPU.

Writes tests/golden/encode.json: per group, batch ("affine", "jacobian",
"jacobian_zero") and encoding
  fnv    FNV-1a 64 of the reference's output
  first  the first byte of every entry (the flag bits), as one hex string
While writing, the script asserts entry by entry that enc_inputs.encode_point
(on Jacobians normalised in plain Python) agrees with the reference.
Test infrastructure only; data, no reference source text.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))

import enc_inputs as ei  # noqa: E402
import enc_special as es  # noqa: E402


def ref_encode(L, group, raw, n, compressed, jacobian):
    name = f"blst_p{group}_{'' if jacobian else 'affine_'}{'compress' if compressed else 'serialize'}"
    f = getattr(L, name)
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    f.restype = None
    sz = (es.ji.JAC if jacobian else ei.AFF)[group]
    E = ei.ENC[group] * (1 if compressed else 2)
    out = bytearray()
    for i in range(n):
        src = (ctypes.c_uint8 * sz).from_buffer_copy(raw[i * sz:(i + 1) * sz])
        dst = (ctypes.c_uint8 * E)()
        f(dst, src)
        out += bytes(dst)
    return bytes(out)


def main():
    L = ctypes.CDLL(os.path.join(REPO, "oracle", "_ref", "libblst_ref.so"))
    cases = []
    for group in (1, 2):
        names = {"affine": es.affine_batch(group)[1], "jacobian": es.jacobian_batch(group)[1]}
        for form in es.FORMS:
            raw, n, jac = es.batch(group, form)
            for compressed in (True, False):
                E = ei.ENC[group] * (1 if compressed else 2)
                ref = ref_encode(L, group, raw, n, compressed, jac)
                mine = es.expected(group, raw, n, compressed, jac)
                for i in range(n):
                    assert mine[i * E:(i + 1) * E] == ref[i * E:(i + 1) * E], \
                        (group, form, compressed, i, names.get(form, ["z_zero"] * n)[i])
                cases.append({"group": group, "form": form, "encoding": "compressed" if compressed else "serialized",
                              "n": n, "fnv": ei.fnv(ref), "first": bytes(ref[i * E] for i in range(n)).hex()})
                print({k: v for k, v in cases[-1].items() if k != "first"}, flush=True)
    with open(os.path.join(HERE, "encode.json"), "w") as f:
        json.dump({"source": "reference libblst (oracle/_ref/libblst_ref.so) blst_p{1,2}_affine_compress / "
                             "_affine_serialize / _compress / _serialize on the batches of tests/enc_special.py "
                             "(batch(group, form)); fnv = FNV-1a 64 of the output, first = the first byte of "
                             "every entry",
                   "cases": cases}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
