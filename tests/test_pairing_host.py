"""CPU-side checks of the bulk pairings (include/msm_mi355x.h: msm_pairing_segments,
msm_fp12_final_exp; msm_blst_amd.ps_pairing / ps_pairing_segments / ps_pairing_check
/ ps_final_exp): the plain-integer model of tests/pairing_inputs.py against the
reference's recorded answers (tests/golden/pairing.json), its bilinearity, the
Frobenius coefficients on their own evidence, the generated constants header, the
piece length and the plan, argument errors (returned before any device work) and
the wrappers' checks.  No GPU is used; the GPU parity lives in test_gpu_pairing.py."""
import ctypes
import os
import sys

import pytest

import pairing_inputs as pi

MSM_OK, MSM_E_ARG, MSM_E_NODEV = 0, -1, -3
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import gen_pairing_consts  # noqa: E402
import pairing_constants as pc  # noqa: E402

G = pi.FP12_BYTES


@pytest.fixture(scope="module")
def m():
    import msm_blst_amd as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def fx(golden):
    return golden("pairing.json")


def entry(b, i):
    return b.hex() if i < 8 else pi.fnv(b)


# ------------------------------------------------------- the model and the fixture ----
def test_model_equals_fixture_pairs(fx):
    ps = pi.pairs()
    assert len(fx["pairs"]) == len(ps) == pi.N_PAIRS
    for i, (p, q) in enumerate(ps):
        assert entry(pi.fp12_bytes(pi.pairing(p, q)), i) == fx["pairs"][i]["e"], i
    for i in pi.INF_PAIRS:
        assert fx["pairs"][i]["e"] == fx["pairs"][i]["ml"] == pi.fnv(pi.fp12_one())
    # the model's raw Miller value differs from the reference's only by what the final exponentiation removes
    for i in range(3):
        ref_ml = pi.fp12_from_bytes(bytes.fromhex(fx["pairs"][i]["ml"]))
        assert pi.fp12_bytes(pi.final_exp(ref_ml)).hex() == fx["pairs"][i]["e"]


def test_model_equals_fixture_segments(fx):
    ps = pi.pairs()
    assert set(fx["segments"]) == set(pi.SEGMENTS)
    for name, layout in pi.SEGMENTS.items():
        assert len(fx["segments"][name]) == len(layout)
        for j, seg in enumerate(layout):
            if len(seg) <= 9:
                assert pi.fp12_bytes(pi.pairing_product([ps[i] for i in seg])).hex() == fx["segments"][name][j], (name, j)
    assert [len(s) for s in pi.SEGMENTS["L3"]] == [0, 1, 2, 3, 4, 7, 0]
    assert fx["segments"]["inf_only"] == [pi.fp12_one().hex()] and fx["segments"]["L1"][0] == pi.fp12_one().hex()
    # the infinity pairs of inf_ends contribute one: the product of the four others
    assert fx["segments"]["inf_ends"][0] == pi.fp12_bytes(pi.pairing_product([ps[i] for i in (3, 4, 5, 6)])).hex()


def test_model_equals_fixture_tower(fx):
    """The ten reference calls per special value (blst_fp12_mul, _sqr, _inverse, _conjugate,
    _frobenius_map 1 .. 3, _mul_by_xy00z0, _cyclotomic_sqr, blst_final_exp), recomputed with the
    model: the oracle of the per-operation tower tests is pinned to the reference op by op."""
    tw = fx["tower"]
    sp = pi.special_fp12()
    assert tuple(tw["values"]) == pi.SPECIAL_NAMES == tuple(sp) and len(sp) == 13
    b = sp["rand"]
    for name in pi.SPECIAL_NAMES:
        want = tw["values"][name]
        assert tuple(want) == pi.TOWER_OPS and len(pi.TOWER_OPS) == 10
        for op, v in zip(pi.TOWER_OPS, pi.tower_model(sp[name], b)):
            raw = pi.fp12_bytes(v)
            assert (raw.hex() if op == "final_exp" else pi.fnv(raw)) == want[op], (name, op)
        assert (want["final_exp"] == pi.fp12_one().hex()) == (name in pi.SPECIAL_FE_ONE), name
    assert tw["final_exp_of_zero_is_zero"] is True
    # the shapes the names promise
    z = pi.F2_ZERO
    assert sp["minus_one"] == [(pi.P - 1, 0)] + [z] * 5 and sp["w"][3] == pi.F2_ONE and sp["v"][1] == pi.F2_ONE
    assert [j for j, c in enumerate(sp["line"]) if c != z] == [0, 1, 4]
    assert pi.fp12_bytes(sp["mont_max"]) == (pi.P - 1).to_bytes(48, "little") * 12


def test_model_is_bilinear():
    p, q = pi.pairs()[0]
    e = pi.pairing(p, q)
    e2 = pi.f12_sqr(e)
    assert not pi.f12_is_one(e) and not pi.f12_is_one(e2)
    assert pi.pairing(pi.mi.smul(1, p, 2), q) == e2 == pi.pairing(p, pi.mi.smul(2, q, 2))
    assert pi.f12_is_one(pi.f12_pow(e, pi.R))
    neg = (p[0], -p[1] % pi.P)
    assert pi.f12_is_one(pi.pairing_product([(p, q), (neg, q)]))
    assert pi.fp12_from_bytes(pi.fp12_bytes(e)) == e and pi.f12_is_one(pi.fp12_from_bytes(pi.fp12_one()))
    assert pi.ei.affine_point(1, pi.neg_g1()) == pi.NEG_G1


def test_tower_identities():
    a = pi.miller_loop([pi.pairs()[1]])
    assert pi.f12_is_one(pi.f12_mul(a, pi.f12_inv(a)))
    for k in (1, 2, 3):
        assert pi.f12_frob(a, k) == pi.f12_pow(a, pi.P ** k), k
    # after the easy part the value is unitary: the conjugate is the inverse
    u = pi.f12_mul(pi.f12_conj(a), pi.f12_inv(a))
    u = pi.f12_mul(u, pi.f12_frob(u, 2))
    assert pi.f12_is_one(pi.f12_mul(u, pi.f12_conj(u)))


# ------------------------------------------------------------------ the constants ----
def test_frobenius_coefficients_from_p():
    assert pc.P == pi.P and pc.XI == (1, 1)
    for k in (1, 2, 3):
        g = pc.gamma(k)
        assert pc.f2_pow(g, 6) == pc.f2_pow(pc.XI, pc.P ** k - 1)
        assert pc.FROB[k] == [pc.f2_pow(g, e) for e in (0, 2, 4, 1, 3, 5)]
    assert pc.f2_pow(pc.gamma(1), 12) != (1, 0)  # w^(p-1) has order above 12: no coefficient is trivial by accident


def test_constants_header_is_generated():
    with open(gen_pairing_consts.OUT) as f:
        assert f.read() == gen_pairing_consts.text(), "run python tools/gen_pairing_consts.py"
    assert gen_pairing_consts.internal(1) == gen_pairing_consts.limbs(pow(2, 392, pi.P))


# ------------------------------------------------------------------------ the ABI ----
def test_exported(m):
    L = m.lib()
    with open(os.path.join(REPO, "include", "msm_mi355x.h")) as f:
        header = f.read()
    for name in ("msm_pairing_segments", "msm_fp12_final_exp"):
        assert hasattr(L, name) and f"int {name}(" in header
    assert "MSM_PAIRING_MILLER_ONLY = 1" in header and m.PAIRING_MILLER_ONLY == 1
    for name in ("ps_pairing", "ps_pairing_segments", "ps_pairing_check", "ps_final_exp"):
        assert name in m.__all__ and callable(getattr(m, name)) and name in m.__doc__
    assert "fp12_one" in m.__all__ and "FP12_BYTES" in m.__all__
    assert m.FP12_BYTES == 576 and m.fp12_one() == pi.fp12_one()
    assert len(L.msm_pairing_segments.argtypes) == 12 and len(L.msm_fp12_final_exp.argtypes) == 9


def test_piece_length(m, monkeypatch):
    L = m.lib()
    monkeypatch.delenv("MSM_PAIRING_PIECE", raising=False)
    monkeypatch.delenv("MSM_PAIRING_CHUNK", raising=False)
    # one piece per resident lane pair (32768), at most a chunk (2^16 pairs) in flight
    assert [L.msm_pairing_piece(n) for n in (0, 1, 100, 1 << 15, 1 << 16, 1 << 20)] == [1, 1, 1, 1, 2, 2]
    monkeypatch.setenv("MSM_PAIRING_CHUNK", str(1 << 22))
    assert L.msm_pairing_piece(1 << 20) == 32 and L.msm_pairing_piece(1 << 22) == 64
    monkeypatch.setenv("MSM_PAIRING_PIECE", "3")
    assert L.msm_pairing_piece(5) == 3
    monkeypatch.setenv("MSM_PAIRING_PIECE", "1000")
    assert L.msm_pairing_piece(5) == 64
    # the pieces of a layout are those of the shared plan
    o = [0]
    for seg in pi.SEGMENTS["L3"]:
        o.append(o[-1] + len(seg))
    assert [c for _, c, _ in m.segments_plan(o, 3)] == [1, 2, 3, 3, 1, 3, 3, 1]


def test_argument_errors_before_any_device_work(m):
    L = m.lib()
    p = (ctypes.c_uint8 * (96 * 4))()
    q = (ctypes.c_uint8 * (192 * 4))()
    dst = (ctypes.c_uint8 * (G * 4))()
    one = (ctypes.c_uint8 * 4)()
    nf = ctypes.c_size_t(0)
    offs = (ctypes.c_size_t * 3)(0, 1, 4)
    bad = (ctypes.c_size_t * 3)(0, 3, 2)
    empty = (ctypes.c_size_t * 3)(2, 2, 2)
    # nothing to do
    assert L.msm_pairing_segments(0, None, None, None, None, None, None, 0, 0, 0, 0, None) == MSM_OK
    assert L.msm_fp12_final_exp(0, None, None, None, None, 0, 0, 0, None) == MSM_OK
    # bad arguments
    assert L.msm_pairing_segments(0, dst, None, None, None, q, offs, 2, 0, 0, 0, None) == MSM_E_ARG  # NULL p
    assert L.msm_pairing_segments(0, dst, None, None, p, None, offs, 2, 0, 0, 0, None) == MSM_E_ARG  # NULL q
    assert L.msm_pairing_segments(0, dst, None, None, p, None, None, 2, 0, 0, 0, None) == MSM_E_ARG  # NULL q, no offsets
    assert L.msm_pairing_segments(0, None, None, None, p, q, offs, 2, 0, 0, 0, None) == MSM_E_ARG  # nothing wanted
    assert L.msm_pairing_segments(0, dst, None, None, p, q, bad, 2, 0, 0, 0, None) == MSM_E_ARG
    assert b"decrease" in L.msm_last_error()
    assert L.msm_pairing_segments(0, dst, None, None, p, q, offs, 2, 2, 0, 0, None) == MSM_E_ARG  # flag bits
    assert L.msm_pairing_segments(0, dst, one, None, p, q, offs, 2, 1, 0, 0, None) == MSM_E_ARG  # is_one, Miller only
    assert L.msm_pairing_segments(0, dst, None, ctypes.byref(nf), p, q, offs, 2, 1, 0, 0, None) == MSM_E_ARG
    assert L.msm_pairing_segments(0, p, None, None, p, q, offs, 2, 0, 0, 0, None) == MSM_E_ARG  # overlap
    assert L.msm_pairing_segments(0, q, None, None, p, q, None, 2, 0, 0, 0, None) == MSM_E_ARG  # overlap
    assert L.msm_fp12_final_exp(0, dst, None, None, None, 2, 0, 0, None) == MSM_E_ARG  # NULL src
    assert L.msm_fp12_final_exp(0, None, None, None, dst, 2, 0, 0, None) == MSM_E_ARG  # nothing wanted
    assert L.msm_fp12_final_exp(0, dst, None, None, dst, 2, 0, 0, None) == MSM_E_ARG  # overlap
    assert L.msm_pairing_segments(0, 12, None, None, 8, 16, offs, 2, 0, 1, 1, None) == MSM_E_ARG  # unaligned device dst
    assert L.msm_pairing_segments(0, 16, None, None, 4, 16, offs, 2, 0, 1, 1, None) == MSM_E_ARG  # unaligned device p
    # a device that does not exist, after the argument checks (no pairs are read from NULL: every segment is empty)
    assert L.msm_pairing_segments(1 << 20, dst, None, None, p, q, offs, 2, 0, 0, 0, None) == MSM_E_NODEV
    assert L.msm_pairing_segments(-1, dst, None, None, None, None, empty, 2, 0, 0, 0, None) == MSM_E_NODEV
    assert L.msm_fp12_final_exp(-1, None, one, None, dst, 2, 0, 0, None) == MSM_E_NODEV
    assert bytes(dst) == bytes(len(dst)) and nf.value == 0  # nothing was touched


def test_tower_test_entry_argument_errors(m):
    """msm_test_fp12 (the per-operation entry of tests/test_gpu_fp12_tower.py): exported, declared,
    and its argument checks come before any device work"""
    L = m.lib()
    with open(os.path.join(REPO, "include", "msm_mi355x.h")) as f:
        assert "int msm_test_fp12(int op, int k, int alias, int raw, const void *a, const void *b, void *out, size_t n);" \
            in f.read()
    assert len(L.msm_test_fp12.argtypes) == 8
    a = (ctypes.c_uint8 * 672)()
    out = (ctypes.c_uint8 * 672)()
    assert L.msm_test_fp12(0, 0, 0, 0, None, None, None, 0) == MSM_OK  # nothing to do
    for op in (-1, 9, 100):
        assert L.msm_test_fp12(op, 1, 0, 0, a, a, out, 1) == MSM_E_ARG, op  # unknown op
    for k in (0, 4, -1):
        assert L.msm_test_fp12(4, k, 0, 0, a, None, out, 1) == MSM_E_ARG, k  # Frobenius power outside 1..3
    for k in (0, 65):
        assert L.msm_test_fp12(6, k, 0, 0, a, None, out, 1) == MSM_E_ARG, k  # squaring count
    assert L.msm_test_fp12(5, 0, 1, 0, a, None, out, 1) == MSM_E_ARG  # the inverse forbids d == a
    assert L.msm_test_fp12(1, 0, 2, 0, a, a, out, 1) == MSM_E_ARG  # d == b for the product only
    assert L.msm_test_fp12(0, 0, 3, 0, a, a, out, 1) == MSM_E_ARG and L.msm_test_fp12(0, 0, 0, 2, a, a, out, 1) == MSM_E_ARG
    assert L.msm_test_fp12(0, 0, 0, 0, a, None, out, 1) == MSM_E_ARG  # the product reads b
    assert L.msm_test_fp12(1, 0, 0, 0, None, None, out, 1) == MSM_E_ARG and L.msm_test_fp12(1, 0, 0, 0, a, None, None, 1) == MSM_E_ARG
    assert bytes(out) == bytes(672)


def test_wrapper_value_errors(m):
    p, q = pi.pair_bytes([0, 1])
    with pytest.raises(ValueError):
        m.ps_pairing(p, q, 3)  # short p and q
    with pytest.raises(ValueError):
        m.ps_pairing(p, q[:-1], 2)  # short q
    with pytest.raises(ValueError):
        m.ps_pairing(p[:-1], q, 2)  # short p
    with pytest.raises(ValueError):
        m.ps_pairing(p, q, -1)
    with pytest.raises(ValueError):
        m.ps_pairing_segments(p, q, [0, 3])  # more pairs than given
    with pytest.raises(ValueError):
        m.ps_pairing_segments(p, q, [0, 2, 1])  # decreasing
    with pytest.raises(ValueError):
        m.ps_pairing_segments(p, q, [-1, 2])
    with pytest.raises(ValueError):
        m.ps_pairing_segments(p, q, [])
    with pytest.raises(ValueError):
        m.ps_pairing_check(p, q, [0, 1, 3])
    with pytest.raises(ValueError):
        m.ps_final_exp(bytes(G), 2)
    with pytest.raises(ValueError):
        m.ps_final_exp(bytes(G), -1)
    # nothing to do: no device is touched
    assert m.ps_pairing(b"", b"", 0) == b"" and m.ps_final_exp(b"", 0) == b""
    assert m.ps_pairing_segments(b"", b"", [0]) == b"" and m.ps_pairing_check(b"", b"", [5]) == b""
