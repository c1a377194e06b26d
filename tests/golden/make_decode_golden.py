#!/usr/bin/env python3
"""Golden fixture for the bulk point decoding (ref src/e1.c:236-351,
src/e2.c:279-410, src/map_to_g1.c:531-559, src/map_to_g2.c:403-443), written
from the REFERENCE itself: oracle/_ref/libblst_ref.so (built by oracle/Makefile)
is called through ctypes -- blst_p{1,2}_uncompress, blst_p{1,2}_deserialize and
blst_p{1,2}_affine_in_g{1,2}, one entry at a time, on the mixed batch of
tests/enc_inputs.py.  Runs only in the build container, on the CPU.

Writes tests/golden/decode.json: per group and encoding
  status     the reference's return code per entry
  in_group   per entry its affine_in_g{1,2} Boolean (null where status != 0)
  fnv        FNV-1a 64 of its outputs with the entries of non-zero status zeroed
  fnv_group  the same with the entries outside the subgroup zeroed too
While writing, the script asserts that enc_inputs.py's own fixed points,
decoder and subgroup test agree with the reference on every entry.
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
from make_to_affine_golden import ref_fixed_points  # noqa: E402


def ref_decode(L, group, data, n, serialized):
    f = getattr(L, f"blst_p{group}_{'deserialize' if serialized else 'uncompress'}")
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    f.restype = ctypes.c_int
    ing = getattr(L, f"blst_p{group}_affine_in_g{group}")
    ing.argtypes = [ctypes.c_void_p]
    ing.restype = ctypes.c_int
    sz, A = ei.ENC[group] * (2 if serialized else 1), ei.AFF[group]
    status, in_group, out = [], [], bytearray()
    for i in range(n):
        src = (ctypes.c_uint8 * sz).from_buffer_copy(data[i * sz:(i + 1) * sz])
        dst = (ctypes.c_uint8 * A)()
        st = f(dst, src)
        status.append(st)
        if st:
            in_group.append(None)
            out += bytes(A)
        else:
            in_group.append(bool(ing(dst)))
            out += bytes(dst)
    return status, in_group, bytes(out)


def main():
    L = ctypes.CDLL(os.path.join(REPO, "oracle", "_ref", "libblst_ref.so"))
    cases = []
    for group in (1, 2):
        assert ei.fixed_affine(group, 48) == ref_fixed_points(L, group, 48), "fixed points differ from the reference's"
        for serialized in (False, True):
            data, names = ei.mixed_batch(group, serialized)
            n, A = ei.MIXED_N, ei.AFF[group]
            status, in_group, out = ref_decode(L, group, data, n, serialized)
            mine_st, mine_out = ei.decode(group, data, n, serialized)
            for i in range(n):
                assert mine_st[i] == status[i], (group, serialized, i, names[i], mine_st[i], status[i])
                assert mine_out[i * A:(i + 1) * A] == out[i * A:(i + 1) * A], (group, serialized, i, names[i])
                if status[i] == 0:
                    assert ei.in_group(group, out[i * A:(i + 1) * A]) == in_group[i], (group, serialized, i, names[i])
            checked = bytearray(out)
            for i in range(n):
                if in_group[i] is False:
                    checked[i * A:(i + 1) * A] = bytes(A)
            st_g, out_g = ei.expected(group, serialized, True)
            assert out_g == bytes(checked) and st_g == [3 if g is False else s for s, g in zip(status, in_group)]
            cases.append({"group": group, "encoding": "serialized" if serialized else "compressed", "n": n,
                          "status": status, "in_group": in_group, "fnv": ei.fnv(out), "fnv_group": ei.fnv(checked)})
            print({k: v for k, v in cases[-1].items() if k not in ("status", "in_group")},
                  "".join(map(str, status)), flush=True)
    with open(os.path.join(HERE, "decode.json"), "w") as f:
        json.dump({"source": "reference libblst (oracle/_ref/libblst_ref.so) blst_p{1,2}_uncompress / _deserialize / "
                             "_affine_in_g{1,2} on the mixed batch of tests/enc_inputs.py (mixed_batch(group, "
                             "serialized)); fnv = FNV-1a 64 of the outputs with failed entries zeroed, fnv_group = "
                             "with the entries outside the subgroup zeroed too",
                   "cases": cases}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
