#!/usr/bin/env python3
"""Golden fixture of the Fr layer, written from the REFERENCE itself:
oracle/_ref/libblst_ref.so (built by oracle/Makefile) is called through ctypes.
Runs only where the reference is present, on the CPU.

Writes tests/golden/fr_ops.json:
  values     the special values (tests/fr_inputs.special_values, seed stated), hex
  pairs      per op, the FNV-1a 64 of the reference's outputs over all ordered pairs
             (a, b) of the values, a-major (one-operand ops: over the values), and the
             outputs themselves for the one-operand ops
  mul, add, sub  the outputs of the binary ops on the pairs, hex, a-major
  from_scalar_wide  blst_fr_from_scalar of r, r + 1 and 2^256 - 1
  inverse_of_zero   what blst_fr_inverse returns for 0
  ntt        the FNV of a 2^10-point forward NTT computed on the reference side as
             the plain O(n^2) sum over blst_fr_mul / blst_fr_add, the powers of
             omega_n built by blst_fr_mul
  cpu        single-thread ns per blst_fr_mul / add / sub on a 2^12 sample (recorded,
             not gated)
Data only; no reference source text.
"""
import ctypes
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import enc_inputs as ei  # noqa: E402
import fr_inputs as fi  # noqa: E402

B32 = ctypes.c_uint8 * 32


def main():
    L = ctypes.CDLL(os.path.join(REPO, "oracle", "_ref", "libblst_ref.so"))
    vp = ctypes.c_void_p
    for name in ("add", "sub", "mul"):
        getattr(L, f"blst_fr_{name}").argtypes = [vp, vp, vp]
    for name in ("blst_fr_sqr", "blst_fr_inverse", "blst_fr_from_scalar", "blst_scalar_from_fr"):
        getattr(L, name).argtypes = [vp, vp]
    L.blst_fr_cneg.argtypes = [vp, vp, ctypes.c_int]

    def call1(fn, a, *extra):
        out = B32()
        fn(out, B32.from_buffer_copy(a), *extra)
        return bytes(out)

    def call2(fn, a, b):
        out = B32()
        fn(out, B32.from_buffer_copy(a), B32.from_buffer_copy(b))
        return bytes(out)

    def ref(op, a, b=None):
        if op in fi.BINARY:
            return call2(getattr(L, f"blst_fr_{op}"), a, b)
        if op == "neg":
            return call1(L.blst_fr_cneg, a, 1)
        return call1({"sqr": L.blst_fr_sqr, "inv": L.blst_fr_inverse, "from_scalar": L.blst_fr_from_scalar,
                      "to_scalar": L.blst_scalar_from_fr}[op], a)

    vals = fi.special_values()
    frs = [fi.fr_bytes(v) for v in vals]
    doc = {"seed": fi.SEED, "values": [f"{v:064x}" for v in vals], "pairs": {}}
    for op in fi.OPS:
        if op in fi.BINARY:
            outs = [ref(op, a, b) for a in frs for b in frs]
            doc[op] = [o.hex() for o in outs]
        else:
            src = [fi.scalar_bytes(v) for v in vals] if op == "from_scalar" else frs
            outs = [ref(op, a) for a in src]
            doc[op] = [o.hex() for o in outs]
        doc["pairs"][op] = ei.fnv(b"".join(outs))
    wide = [fi.R, fi.R + 1, (1 << 256) - 1]
    doc["from_scalar_wide"] = [[f"{v:064x}", ref("from_scalar", fi.scalar_bytes(v)).hex()] for v in wide]
    doc["inverse_of_zero"] = ref("inv", fi.fr_bytes(0)).hex()

    # the 2^10 forward NTT as the plain sum, on the reference's own arithmetic
    log_n, n = 10, 1 << 10
    x = [fi.fr_bytes(v) for v in fi.rand_values(n, fi.NTT_HASH_SEED)]
    w = fi.fr_bytes(fi.root(log_n))
    pw = [fi.fr_bytes(1)]
    for _ in range(n - 1):
        pw.append(ref("mul", pw[-1], w))
    out = []
    for k in range(n):
        acc = fi.fr_bytes(0)
        for j in range(n):
            acc = ref("add", acc, ref("mul", x[j], pw[j * k % n]))
        out.append(acc)
    doc["ntt"] = {"log_n": log_n, "seed": fi.NTT_HASH_SEED, "fnv": ei.fnv(b"".join(out))}

    # single-thread cost of the reference's loops (2^12 sample, in place, one call per element)
    m = 1 << 12
    buf = (ctypes.c_uint8 * (32 * m)).from_buffer_copy(fi.pack(fi.rand_values(m, 5)))
    base = ctypes.addressof(buf)
    cpu = {}
    for name in ("mul", "add", "sub"):
        fn = getattr(L, f"blst_fr_{name}")
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            for i in range(m - 1):
                fn(base + 32 * i, base + 32 * i, base + 32 * (i + 1))
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        cpu[name + "_ns_ctypes"] = round(best / (m - 1) * 1e9, 1)
    doc["cpu"] = cpu

    path = os.path.join(REPO, "tests", "golden", "fr_ops.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
