#!/usr/bin/env python3
"""Golden fixture for the bulk signature verification (ref src/aggregate.c), written
from the REFERENCE itself: oracle/_ref/libblst_ref.so (built by oracle/Makefile) is
called through ctypes -- blst_core_verify_pk_in_g{1,2}, blst_pairing_init,
blst_pairing_chk_n_aggr_pk_in_g{1,2}, blst_pairing_chk_n_mul_n_aggr_pk_in_g{1,2},
blst_pairing_commit, blst_pairing_finalverify, blst_p{1,2}_uncompress,
blst_p{1,2}_affine_in_g{1,2}, blst_p{1,2}s_add -- on the tables of
tests/sig_inputs.py, in exactly the sequences include/msm_mi355x.h documents.  Runs
only in the build container, on the CPU.

Writes tests/golden/sigs.json:
  tables[name][scheme][form]  form "affine" or "encoded": "status", the reference's
                              code per check, and "inputs", an FNV-1a 64 of the input
                              bytes (drift of the generator is caught)
  model                       the checks on which the Python model was evaluated
While writing, the script asserts that the Python model agrees with the reference on
the checks of MODEL_CHECKS (the pure-Python pairing affords no more).
Test infrastructure only; data, no reference source text.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))

import sig_inputs as si  # noqa: E402

sz = ctypes.c_size_t


def _buf(b):
    return (ctypes.c_uint8 * max(len(b), 1)).from_buffer_copy(bytes(b) or b"\0")


class Ref:
    def __init__(self, path):
        self.L = L = ctypes.CDLL(path)
        L.blst_pairing_sizeof.restype = sz
        for g in (1, 2):
            getattr(L, f"blst_p{g}_affine_in_g{g}").restype = ctypes.c_int

    def point(self, g, item, encoded):
        """(uncompress code, affine bytes) of one entry as the library receives it"""
        raw = si.item_bytes(g, item, encoded)
        if not encoded:
            return 0, raw
        out = (ctypes.c_uint8 * (96 * g))()
        rc = getattr(self.L, f"blst_p{g}_uncompress")(out, _buf(raw))
        return rc, bytes(out)

    def in_group(self, g, aff):
        return bool(getattr(self.L, f"blst_p{g}_affine_in_g{g}")(_buf(aff)))

    def sum(self, g, affs):
        ptrs = (ctypes.c_void_p * len(affs))()
        keep = [_buf(a) for a in affs]
        for i, k in enumerate(keep):
            ptrs[i] = ctypes.addressof(k)
        jac = (ctypes.c_uint8 * (144 * g))()
        getattr(self.L, f"blst_p{g}s_add")(jac, ptrs, sz(len(affs)))
        out = (ctypes.c_uint8 * (96 * g))()
        getattr(self.L, f"blst_p{g}_to_affine")(out, jac)
        return bytes(out)

    def core_verify(self, scheme, pk, sig, hash_mode, msg, dst, aug):
        f = getattr(self.L, f"blst_core_verify_pk_in_g{scheme}")
        return f(_buf(pk), _buf(sig), ctypes.c_int(hash_mode), _buf(msg), sz(len(msg)), _buf(dst), sz(len(dst)),
                 _buf(aug), sz(len(aug)))


def ref_check(R, call, j, encoded):
    """the status of check j by the reference's own sequence"""
    scheme, mode = call["scheme"], call["mode"]
    kg, sg = scheme, 3 - scheme
    dst = si.tag(scheme)
    hash_mode = 0 if call["variant"] == "encode" else 1

    def sig_steps(item):
        rc, aff = R.point(sg, item, encoded)
        if rc:
            return rc, None
        if any(aff) and not R.in_group(sg, aff):
            return 3, None
        return 0, aff

    def key_steps(item):
        rc, aff = R.point(kg, item, encoded)
        if rc:
            return rc, None
        if not any(aff):
            return 6, None
        if not R.in_group(kg, aff):
            return 3, None
        return 0, aff

    if mode == si.VERIFY and not encoded and not call["pk_off"]:  # one affine key: the reference's call, nothing else
        return R.core_verify(scheme, si.item_bytes(kg, call["keys"][j], False), si.item_bytes(sg, call["sigs"][j], False),
                             hash_mode, call["msgs"][j], dst, call["augs"][j])
    if mode == si.VERIFY:
        rc, sig = sig_steps(call["sigs"][j])
        if rc:
            return rc
        k0, k1 = (call["pk_off"][j], call["pk_off"][j + 1]) if call["pk_off"] else (j, j + 1)
        affs = []
        for t in range(k0, k1):
            rc, aff = key_steps(call["keys"][t])
            if rc:
                return rc
            affs.append(aff)
        if not affs:
            return 6
        pk = R.sum(kg, affs) if len(affs) != 1 else affs[0]
        if not any(pk):
            return 6
        return R.core_verify(scheme, pk, sig, hash_mode, call["msgs"][j], dst, call["augs"][j])
    # the pairing context: chk_n_aggr / chk_n_mul_n_aggr per tuple, commit, finalverify
    L = R.L
    ctx = (ctypes.c_uint8 * L.blst_pairing_sizeof())()
    dbuf = _buf(dst)
    L.blst_pairing_init(ctx, ctypes.c_int(hash_mode), dbuf, sz(len(dst)))
    nbits = call["nbits"]
    for t in range(call["o"][j], call["o"][j + 1]):
        sig = None
        if mode == si.BATCH or t == call["o"][j]:
            rc, sig = sig_steps(call["sigs"][t if mode == si.BATCH else j])
            if rc:
                return rc
        rc, key = key_steps(call["keys"][t])
        if rc:
            return rc
        msg, aug = call["msgs"][t], call["augs"][t]
        sp = _buf(sig) if sig is not None else None
        if mode == si.AGGREGATE:
            rc = getattr(L, f"blst_pairing_chk_n_aggr_pk_in_g{scheme}")(
                ctx, _buf(key), sz(1), sp, sz(1), _buf(msg), sz(len(msg)), _buf(aug), sz(len(aug)))
        else:
            w = _buf(call["weights"][t].to_bytes((nbits + 7) // 8, "little")) if call["weights"] else None
            rc = getattr(L, f"blst_pairing_chk_n_mul_n_aggr_pk_in_g{scheme}")(
                ctx, _buf(key), sz(1), sp, sz(1), w, sz(nbits), _buf(msg), sz(len(msg)), _buf(aug), sz(len(aug)))
        if rc:
            return rc
    L.blst_pairing_commit(ctx)
    return 0 if L.blst_pairing_finalverify(ctx, None) else 5


# the checks the model is evaluated on: (table, form, indices); every status value and every mode
MODEL_CHECKS = [
    ("individual", "affine", [0, 28, 30, 31, 32, 33, 34, 35, 36]),
    ("individual_encoded", "encoded", [1, 40, 41, 42, 43, 44]),
    ("individual_encode", "affine", [0, 12]),
    ("individual_aug", "affine", [1, 13]),
    ("key_sets", "affine", [0, 2, 4, 5, 6, 7]),
    ("aggregate", "affine", [0, 2, 5, 6, 8, 10]),
    ("batch_w64", "affine", [1, 5, 6, 7, 8]),
    ("batch_w255", "affine", [0]),
    ("batch_w0", "affine", [1, 3]),
]


def main():
    R = Ref(os.path.join(REPO, "oracle", "_ref", "libblst_ref.so"))
    out = {"tables": {}, "model": [[n, f, idx] for n, f, idx in MODEL_CHECKS]}
    for name in si.TABLES:
        out["tables"][name] = {}
        for scheme in (1, 2):
            call = si.table(name, scheme)
            forms = {}
            for form in ("affine", "encoded"):
                enc = form == "encoded"
                if enc and name not in si.ENCODED_TOO:
                    continue
                if not enc and name == "individual_encoded":
                    continue
                status = [ref_check(R, call, j, enc) for j in range(si.nchecks(call))]
                forms[form] = {"status": status, "inputs": si.input_hash(call, enc)}
                print(name, scheme, form, status, flush=True)
            out["tables"][name][str(scheme)] = forms
    for name, form, idx in MODEL_CHECKS:
        for scheme in (1, 2):
            call = si.table(name, scheme)
            want = out["tables"][name][str(scheme)][form]["status"]
            for j in idx:
                got = si.model_status(call, j)
                assert got == want[j], (name, scheme, form, j, got, want[j])
        print("model agrees on", name, form, idx, flush=True)
    seen = {v for t in out["tables"].values() for s in t.values() for f in s.values() for v in f["status"]}
    assert seen == {0, 1, 2, 3, 5, 6}, seen
    with open(os.path.join(HERE, "sigs.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
