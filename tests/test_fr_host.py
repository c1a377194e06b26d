"""CPU-side checks of the Fr layer (include/msm_mi355x.h: msm_fr_ntt, msm_fr_op,
msm_fr_root_of_unity, msm_ntt_plan; msm_blst_amd.fr_ntt / fr_op): the plain-Python
oracle of tests/fr_inputs.py against the reference's recorded answers
(tests/golden/fr_ops.json), the host-only calls, the pass plan, and the argument
errors that are decided before any device work.  No GPU is used; the GPU parity
lives in test_gpu_fr_ntt.py, the range argument in test_fr_bounds.py."""
import ctypes
import json
import os

import pytest

import enc_inputs as ei
import fr_inputs as fi

MSM_OK, MSM_E_ARG, MSM_E_NODEV = 0, -1, -3
vp = ctypes.c_void_p
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fr_ops.json")


@pytest.fixture(scope="module")
def m():
    import msm_blst_amd as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_exported(m):
    for name in ("msm_fr_ntt", "msm_fr_op", "msm_fr_root_of_unity", "msm_ntt_plan", "msm_fr_probe"):
        assert hasattr(m.lib(), name)
    for name in ("fr_ntt", "fr_op", "fr_root_of_unity", "ntt_plan"):
        assert name in m.__all__ and callable(getattr(m, name))
    assert (m.NTT_INVERSE, m.FR_SRC_SCALAR, m.FR_DST_SCALAR, m.FR_B_ONE) == (1, 2, 4, 1)
    assert [m.FR_OPS[o] for o in fi.OPS] == list(range(8))
    assert "fr_ntt" in m.__doc__


# ---- the oracle against the reference's recorded answers ----
def test_oracle_reproduces_the_golden_ops(golden):
    vals = [int(v, 16) for v in golden["values"]]
    assert vals == fi.special_values() and golden["seed"] == fi.SEED
    frs = [fi.fr_bytes(v) for v in vals]
    for op in fi.OPS:
        if op in fi.BINARY:
            outs = [fi.op_bytes(op, a, b) for a in frs for b in frs]
        elif op == "from_scalar":
            outs = [fi.op_bytes(op, fi.scalar_bytes(v)) for v in vals]
        else:
            outs = [fi.op_bytes(op, a) for a in frs]
        assert [o.hex() for o in outs] == golden[op], op
        assert ei.fnv(b"".join(outs)) == golden["pairs"][op], op
    for v, want in golden["from_scalar_wide"]:
        assert fi.op_bytes("from_scalar", fi.scalar_bytes(int(v, 16))).hex() == want
    # the contract's inverse of zero is the reference's
    assert golden["inverse_of_zero"] == fi.op_bytes("inv", fi.fr_bytes(0)).hex() == bytes(32).hex()


def test_oracle_reproduces_the_golden_ntt_hash(golden):
    g = golden["ntt"]
    x = fi.rand_values(1 << g["log_n"], g["seed"])
    assert (g["log_n"], g["seed"]) == (10, fi.NTT_HASH_SEED)
    assert ei.fnv(fi.pack(fi.ntt(x))) == g["fnv"]


def test_oracle_ntt_is_the_plain_sum_and_inverts():
    x = fi.rand_values(32, 3)
    assert fi.ntt(x) == fi.ntt_slow(x)
    assert fi.ntt(fi.ntt(x), inverse=True) == x
    for s in (7, fi.rand_values(1, 9)[0]):
        ev = fi.ntt(x, shift=s)
        w = fi.root(5)
        assert ev[3] == sum(x[j] * pow(s * pow(w, 3, fi.R), j, fi.R) for j in range(32)) % fi.R
        assert fi.ntt(ev, inverse=True, shift=s) == x


# ---- host-only calls ----
def test_root_of_unity(m):
    L = m.lib()
    for k in range(33):
        w = fi.fr_int(m.fr_root_of_unity(k))
        assert w == fi.root(k), k
        assert m.fr_root_of_unity(k) == fi.fr_bytes(w)
        if k:
            assert pow(w, 1 << (k - 1), fi.R) == fi.R - 1, k
    out = (ctypes.c_uint8 * 32)()
    assert L.msm_fr_root_of_unity(33, out) == MSM_E_ARG
    assert L.msm_fr_root_of_unity(3, None) == MSM_E_ARG


@pytest.mark.parametrize("tile", [None, 2, 4, 10, 11])
def test_ntt_plan(m, tile, monkeypatch):
    if tile is None:
        monkeypatch.delenv("MSM_NTT_TILE", raising=False)
    else:
        monkeypatch.setenv("MSM_NTT_TILE", str(tile))
    t = tile or 10
    for log_n in range(27):
        plan = m.ntt_plan(log_n)
        assert sum(plan) == log_n and all(1 <= k <= t for k in plan), (log_n, plan)
        assert (len(plan) == 1) == (1 <= log_n <= t)
        if len(plan) > 1:  # a tile of several passes keeps columns beside its rows
            assert all(k <= t - (2 if t >= 4 else 1) for k in plan), (log_n, plan)
            assert max(plan) - min(plan) <= 1
    n = ctypes.c_int(-1)
    radix = (ctypes.c_int * 32)()
    assert m.lib().msm_ntt_plan(27, ctypes.byref(n), radix, 32) == MSM_E_ARG
    assert m.lib().msm_ntt_plan(5, None, radix, 32) == MSM_E_ARG
    assert m.lib().msm_ntt_plan(26, ctypes.byref(n), None, 0) == MSM_OK and n.value >= 3


def test_ntt_tile_out_of_range_is_the_default(m, monkeypatch):
    monkeypatch.delenv("MSM_NTT_TILE", raising=False)
    want = m.ntt_plan(20)
    for bad in ("1", "12", "abc", "0"):
        monkeypatch.setenv("MSM_NTT_TILE", bad)
        assert m.ntt_plan(20) == want


# ---- argument errors, before any device work ----
def test_ntt_empty_call_touches_nothing(m):
    L = m.lib()
    assert L.msm_fr_ntt(0, None, None, 10, 0, None, 0, 0, 0, None) == MSM_OK
    assert L.msm_fr_ntt(0, None, None, 0, 0, None, 7, 1, 1, None) == MSM_OK
    assert m.fr_ntt(b"", 5, 0) == b""
    assert L.msm_fr_op(0, 2, None, None, None, 0, 0, 0, 0, None) == MSM_OK
    assert m.fr_op("mul", b"", b"") == b""


def test_ntt_argument_errors(m):
    L = m.lib()
    n = 8
    src = (ctypes.c_uint8 * (32 * n + 64))()
    dst = (ctypes.c_uint8 * (32 * n))()

    def call(*a):
        rc = L.msm_fr_ntt(*a)
        if rc == MSM_E_ARG:
            assert L.msm_last_error()
        return rc

    assert call(0, None, src, 3, 1, None, 0, 0, 0, None) == MSM_E_ARG  # NULL dst
    assert b"null" in L.msm_last_error()
    assert call(0, dst, None, 3, 1, None, 0, 0, 0, None) == MSM_E_ARG  # NULL src
    assert call(0, dst, src, 27, 1, None, 0, 0, 0, None) == MSM_E_ARG  # log_n above 26
    assert b"log_n" in L.msm_last_error()
    assert call(0, dst, src, 3, 1, None, 8, 0, 0, None) == MSM_E_ARG  # unknown flag bits
    assert b"flag" in L.msm_last_error()
    for bad in (0, fi.R, fi.R + 5, (1 << 256) - 1):  # a shift of 0 or >= r
        s = (ctypes.c_uint8 * 32).from_buffer_copy(bad.to_bytes(32, "little"))
        assert call(0, dst, src, 3, 1, s, 0, 0, 0, None) == MSM_E_ARG
        assert b"shift" in L.msm_last_error()
    # an overlap other than dst == src; misaligned device pointers
    base = ctypes.addressof(src)
    assert call(0, vp(base + 32), src, 3, 1, None, 0, 0, 0, None) == MSM_E_ARG
    assert b"overlap" in L.msm_last_error()
    assert call(0, vp(base + 4), vp(base), 3, 1, None, 0, 1, 1, None) == MSM_E_ARG
    assert call(0, dst, vp(base + 4), 3, 1, None, 0, 1, 0, None) == MSM_E_ARG
    assert b"aligned" in L.msm_last_error()
    assert call(0, vp(base + 2), src, 3, 1, None, 0, 0, 1, None) == MSM_E_ARG
    assert bytes(dst) == bytes(len(dst))
    # a good call (in place included) gets as far as the device check
    good = (ctypes.c_uint8 * 32).from_buffer_copy((7).to_bytes(32, "little"))
    for d in (dst, src):
        rc = call(0, d, src, 3, 1, good, 7, 0, 0, None)
        assert rc in (MSM_OK, MSM_E_NODEV)
    assert call(1 << 20, dst, src, 3, 1, None, 0, 0, 0, None) == MSM_E_NODEV
    assert call(-1, dst, src, 3, 1, None, 0, 0, 0, None) == MSM_E_NODEV


def test_op_argument_errors(m):
    L = m.lib()
    n = 4
    a = (ctypes.c_uint8 * (32 * n + 64))()
    b = (ctypes.c_uint8 * (32 * n))()
    dst = (ctypes.c_uint8 * (32 * n))()

    def call(*args):
        rc = L.msm_fr_op(*args)
        if rc == MSM_E_ARG:
            assert L.msm_last_error()
        return rc

    for op in (-1, 8, 100):
        assert call(0, op, dst, a, b, n, 0, 0, 0, None) == MSM_E_ARG
        assert b"op" in L.msm_last_error()
    assert call(0, 0, dst, a, b, n, 2, 0, 0, None) == MSM_E_ARG  # unknown flag bits
    assert b"flag" in L.msm_last_error()
    assert call(0, 0, None, a, b, n, 0, 0, 0, None) == MSM_E_ARG
    assert call(0, 0, dst, None, b, n, 0, 0, 0, None) == MSM_E_ARG
    assert call(0, 2, dst, a, None, n, 0, 0, 0, None) == MSM_E_ARG  # a two-operand op reads b
    assert b"null" in L.msm_last_error()
    base = ctypes.addressof(a)
    assert call(0, 0, vp(base + 32), a, b, n, 0, 0, 0, None) == MSM_E_ARG
    assert b"overlap" in L.msm_last_error()
    assert call(0, 0, vp(ctypes.addressof(b) + 32), a, b, 2, 0, 0, 0, None) == MSM_E_ARG
    assert call(0, 0, dst, vp(base + 4), b, n, 0, 1, 0, None) == MSM_E_ARG
    assert b"aligned" in L.msm_last_error()
    assert call(0, 0, dst, a, vp(ctypes.addressof(b) + 4), n, 0, 1, 0, None) == MSM_E_ARG
    assert call(0, 4, vp(base + 2), a, None, n, 0, 0, 1, None) == MSM_E_ARG
    # the one-operand ops ignore b; dst may be a or b
    for args in ((4, dst, a, None), (5, a, a, None), (0, a, a, b), (0, b, a, b)):
        assert call(0, args[0], args[1], args[2], args[3], n, 0, 0, 0, None) in (MSM_OK, MSM_E_NODEV)
    assert call(1 << 20, 0, dst, a, b, n, 0, 0, 0, None) == MSM_E_NODEV


def test_python_wrapper_checks(m):
    with pytest.raises(ValueError):
        m.fr_ntt(bytes(32), 27)
    with pytest.raises(ValueError):
        m.fr_ntt(bytes(31 * 8), 3)  # too few bytes
    with pytest.raises(ValueError):
        m.fr_ntt(bytes(32 * 8), 3, shift=0)
    with pytest.raises(ValueError):
        m.fr_op("mul", bytes(64))  # needs b
    with pytest.raises(ValueError):
        m.fr_op("add", bytes(64), bytes(32))  # b too short without b_one
    with pytest.raises(KeyError):
        m.fr_op("div", bytes(64), bytes(64))
