"""CPU-side checks of msm_test_fp_ops (include/msm_mi355x.h), the per-operation device entry
of tests/test_gpu_fp_ops.py: exported, declared, bound in _ffi.py, and every argument error
returned before any device work (there is no GPU here), n == 0 accepted."""
import ctypes
import os
import subprocess

import pytest

MSM_OK, MSM_E_ARG = 0, -1
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP, FP2, FP2L = 0, 1, 2
N_OPS = 29
FP_ONLY = range(18, 24)
CHAIN_OPS = {0, 1, 2, 3, 4, 18, 19, 24, 25, 26, 27}
READS_FLAGS = {21, 24}
COOP_ADD, F_MUL_SUB_BS, F_ONE = 28, 4, 15


@pytest.fixture(scope="module")
def L():
    import msm_blst_amd as m
    return m.lib()


def test_entry_is_exported_declared_and_bound(L):
    lib = os.path.join(REPO, "msm_blst_amd", "libmsm_mi355x.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert "msm_test_fp_ops" in {line.split()[-1] for line in out.splitlines() if line.strip()}
    with open(os.path.join(REPO, "include", "msm_mi355x.h")) as f:
        hdr = " ".join(f.read().split())
    assert ("int msm_test_fp_ops(int field, int form, int op, const uint32_t *in, const uint32_t *flags, "
            "uint32_t *out, size_t n, size_t cap);") in hdr
    assert len(L.msm_test_fp_ops.argtypes) == 8


def test_argument_errors_come_before_any_device_work(L):
    buf = (ctypes.c_uint32 * (8 * 4 * 28))()
    fl = (ctypes.c_uint32 * 4)()
    call = L.msm_test_fp_ops
    # nothing to do: accepted for every op that exists on the field, NULL arrays and all
    for field in (FP, FP2, FP2L):
        for op in range(N_OPS):
            ok = not (field != FP and op in FP_ONLY) and not (field == FP2 and op in (COOP_ADD, F_MUL_SUB_BS))
            assert call(field, 0, op, None, None, None, 0, 0) == (MSM_OK if ok else MSM_E_ARG), (field, op)
    for op in (-1, N_OPS, 1000):
        assert call(FP, 0, op, buf, fl, buf, 1, 1) == MSM_E_ARG, op            # unknown op
    for field in (-1, 3):
        assert call(field, 0, 0, buf, fl, buf, 1, 1) == MSM_E_ARG, field        # unknown field
    for form in (-1, 2):
        assert call(FP, form, 0, buf, fl, buf, 1, 1) == MSM_E_ARG, form         # unknown form
    for op in range(N_OPS):                                                     # the single chain: Fp, and only its ops
        want_fp = MSM_OK if op in CHAIN_OPS else MSM_E_ARG
        assert call(FP, 1, op, buf, fl, buf, 0, 0) == want_fp, op
        assert call(FP2, 1, op, buf, fl, buf, 0, 0) == MSM_E_ARG, op
        assert call(FP2L, 1, op, buf, fl, buf, 0, 0) == MSM_E_ARG, op
    for op in FP_ONLY:                                                          # an Fp-only op elsewhere
        assert call(FP2, 0, op, buf, fl, buf, 1, 1) == MSM_E_ARG and call(FP2L, 0, op, buf, fl, buf, 1, 1) == MSM_E_ARG
    assert call(FP2, 0, COOP_ADD, buf, fl, buf, 1, 1) == MSM_E_ARG              # no cooperative kernel on one-lane Fp2
    assert call(FP2, 0, F_MUL_SUB_BS, buf, fl, buf, 1, 1) == MSM_E_ARG          # fp.hpp has none there
    assert call(FP, 0, 0, buf, fl, buf, 2, 1) == MSM_E_ARG                      # cap < n
    for op in range(N_OPS):                                                     # a NULL array that is used
        assert call(FP, 0, op, buf, fl, None, 1, 1) == MSM_E_ARG, op
        if op != F_ONE:
            assert call(FP, 0, op, None, fl, buf, 1, 1) == MSM_E_ARG, op
        if op in READS_FLAGS:
            assert call(FP, 0, op, buf, None, buf, 1, 1) == MSM_E_ARG, op
