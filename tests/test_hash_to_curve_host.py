"""CPU-side checks of the bulk hash-to-curve (include/msm_mi355x.h: msm_points_map,
msm_hash_to_field, msm_points_hash, msm_h2c_dst_prime; msm_blst_amd.ps_map_to_curve /
ps_hash_to_field / ps_hash_to_curve): the plain-Python model of tests/h2c_inputs.py
against the reference's recorded answers (tests/golden/hash_to_curve.json), the
isogeny tables on their own evidence, the generated constants header, DST_prime
through the ABI, argument errors (returned before any device work), the wrappers'
checks, and the host SHA-256 / template code of csrc/hash_to_curve.hpp against
hashlib in a stand-alone program under AddressSanitizer and UBSan.  No GPU is used;
the GPU parity lives in test_gpu_hash_to_curve.py."""
import ctypes
import hashlib
import os
import subprocess
import sys

import pytest

import h2c_inputs as h
from jac_inputs import SplitMix64

MSM_OK, MSM_E_ARG, MSM_E_NODEV = 0, -1, -3
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import gen_h2c_consts  # noqa: E402
import h2c_constants as hc  # noqa: E402


@pytest.fixture(scope="module")
def m():
    import msm_blst_amd as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def fx(golden):
    return golden("hash_to_curve.json")["groups"]


# ------------------------------------------------------- the model and the fixture ----
@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("encode", [False, True])
def test_model_equals_fixture_mixed(fx, group, encode):
    want = fx[str(group)]["mixed"]["encode" if encode else "hash"]
    msgs = h.messages()
    assert len(want) == len(msgs) == h.MIXED_N and [len(x) for x in msgs[:130]] == list(range(130))
    for i, msg in enumerate(msgs):
        assert h.entry(group, h.hash_to_curve(group, msg, h.DST[group], b"", encode)) == want[i], i


@pytest.mark.parametrize("group", [1, 2])
def test_model_equals_fixture_cases(fx, group):
    G = fx[str(group)]
    for name in h.CASES:
        msgs, dst, aug, _ = h.case(group, name)
        for i, msg in enumerate(msgs):
            assert h.entry(group, h.hash_to_curve(group, msg, dst, aug[i] if aug else b"")) == G["cases"][name][i], (name, i)
    us, pairs = h.map_cases(group)
    assert [h.entry(group, h.map_to_curve(group, [u])) for u in us] == G["map1"]
    assert [h.entry(group, h.map_to_curve(group, list(p))) for p in pairs] == G["map2"]
    assert sum(e["c"].startswith("c0") for e in G["map2"]) >= 2  # the u == -v pairs
    for i in range(16):
        assert h.field_bytes(group, h.hash_to_field(group, h.messages()[i], h.DST[group], 2)).hex() == G["fields"][i]


def test_special_u_hit_the_exceptional_cases():
    A, Z = hc.A[1], hc.Z[1]
    hits = 0
    for u in h.special_u(1):
        zuu = Z * u * u % h.P
        hits += (-A * (zuu * zuu + zuu)) % h.P == 0
    assert hits == 3  # u = 0 and +-sqrt(-1/Z)
    assert h.f_sqrt(2, h.f_neg(2, h.f_inv(2, hc.Z[2]))) is None  # none but u = 0 over Fp2


# ------------------------------------------------------------- the isogeny tables ----
def _random_point(group, rng, a, b):
    while True:
        x = rng.fp() if group == 1 else (rng.fp(), rng.fp())
        y = h.f_sqrt(group, h._rhs(group, x, a, b))
        if y is not None:
            return (x, y)


@pytest.mark.parametrize("group", [1, 2])
def test_isogeny_maps_onto_the_curve_and_is_a_homomorphism(group):
    rng = SplitMix64(0x150 + group)
    a, b = hc.A[group], hc.B[group]
    zero, b_e = h.f_zero(group), (4 if group == 1 else (4, 4))
    pts = [_random_point(group, rng, a, b) for _ in range(6)]
    for p in pts:
        assert h.on_curve(group, p, a, b) and not h.on_curve(group, p, zero, b_e)
        assert h.on_curve(group, h.iso(group, p), zero, b_e)
    for p, q in zip(pts[::2], pts[1::2]):
        lhs = h.iso(group, h.add_affine(group, p, q, a))
        assert lhs == h.add_pt(group, h.iso(group, p), h.iso(group, q))
        assert h.iso(group, h.add_affine(group, p, p, a)) == h.add_pt(group, h.iso(group, p), h.iso(group, p))
    assert h.add_affine(group, pts[0], h.neg_pt(group, pts[0]), a) is None


def test_constants_header_is_generated_from_the_table():
    with open(gen_h2c_consts.OUT) as f:
        assert f.read() == gen_h2c_consts.text(), "run python tools/gen_h2c_consts.py"
    # the round constants against a digest computed with them
    st = gen_h2c_consts.sha_compress(gen_h2c_consts.SHA_H0, b"abc" + b"\x80" + bytes(59) + b"\x18")
    assert b"".join(v.to_bytes(4, "big") for v in st) == hashlib.sha256(b"abc").digest()


# ------------------------------------------------------------------------ the ABI ----
def test_exported(m):
    L = m.lib()
    with open(os.path.join(REPO, "include", "msm_mi355x.h")) as f:
        header = f.read()
    for name in ("msm_points_map", "msm_hash_to_field", "msm_points_hash", "msm_h2c_dst_prime"):
        assert hasattr(L, name) and f"int {name}(" in header
    assert "MSM_H2C_ENCODE = 1" in header and m.H2C_ENCODE == 1
    for name in ("ps_map_to_curve", "ps_hash_to_field", "ps_hash_to_curve"):
        assert name in m.__all__ and callable(getattr(m, name)) and name in m.__doc__
    assert len(L.msm_points_hash.argtypes) == 15 and len(L.msm_points_map.argtypes) == 9


@pytest.mark.parametrize("n", [0, 43, 255, 256, 300])
def test_dst_prime(m, n):
    dst = h._bytes(n, 250) if n != 43 else h.DST[1]
    assert len(dst) == n
    assert m.h2c_dst_prime(dst) == h.dst_prime(dst)
    assert len(m.h2c_dst_prime(dst)) == (n + 1 if n <= 255 else 33)


def test_dst_prime_argument_errors(m):
    L = m.lib()
    out, n = (ctypes.c_uint8 * 256)(), ctypes.c_size_t(0)
    assert L.msm_h2c_dst_prime(None, ctypes.byref(n), b"x", 1) == MSM_E_ARG
    assert L.msm_h2c_dst_prime(out, None, b"x", 1) == MSM_E_ARG
    assert L.msm_h2c_dst_prime(out, ctypes.byref(n), None, 1) == MSM_E_ARG
    assert L.msm_h2c_dst_prime(out, ctypes.byref(n), None, 0) == MSM_OK and n.value == 1 and out[0] == 0


@pytest.mark.parametrize("group", [1, 2])
def test_argument_errors_before_any_device_work(m, group):
    L = m.lib()
    buf = (ctypes.c_uint8 * 4096)()
    dst = (ctypes.c_uint8 * 4096)()
    offs = (ctypes.c_size_t * 3)(0, 5, 9)
    bad = (ctypes.c_size_t * 3)(0, 5, 4)
    tag = b"tag"
    # nothing to do
    assert L.msm_points_map(group, 0, None, None, 0, 2, 0, 0, None) == MSM_OK
    assert L.msm_points_hash(group, 0, None, None, None, 0, None, 0, 0, tag, 3, 0, 0, 0, None) == MSM_OK
    assert L.msm_hash_to_field(group, 0, None, None, None, 0, None, 0, 0, tag, 3, 2, 0, 0, None) == MSM_OK
    # bad arguments
    assert L.msm_points_map(3, 0, dst, buf, 2, 2, 0, 0, None) == MSM_E_ARG
    assert L.msm_points_map(group, 0, dst, buf, 2, 3, 0, 0, None) == MSM_E_ARG
    assert L.msm_points_map(group, 0, None, buf, 2, 2, 0, 0, None) == MSM_E_ARG
    assert L.msm_points_map(group, 0, dst, None, 2, 2, 0, 0, None) == MSM_E_ARG
    assert L.msm_points_map(group, 0, buf, buf, 2, 2, 0, 0, None) == MSM_E_ARG  # overlap
    assert L.msm_points_hash(0, 0, dst, buf, offs, 0, None, 0, 2, tag, 3, 0, 0, 0, None) == MSM_E_ARG
    assert L.msm_points_hash(group, 0, dst, buf, offs, 0, None, 0, 2, tag, 3, 2, 0, 0, None) == MSM_E_ARG  # flag bits
    assert L.msm_points_hash(group, 0, dst, buf, bad, 0, None, 0, 2, tag, 3, 0, 0, 0, None) == MSM_E_ARG
    assert b"decrease" in L.msm_last_error()
    assert L.msm_points_hash(group, 0, dst, None, offs, 0, None, 0, 2, tag, 3, 0, 0, 0, None) == MSM_E_ARG
    assert L.msm_points_hash(group, 0, dst, buf, offs, 0, None, 0, 2, None, 3, 0, 0, 0, None) == MSM_E_ARG
    assert L.msm_points_hash(group, 0, None, buf, offs, 0, None, 0, 2, tag, 3, 0, 0, 0, None) == MSM_E_ARG
    assert L.msm_hash_to_field(group, 0, dst, buf, offs, 0, None, 0, 2, tag, 3, 0, 0, 0, None) == MSM_E_ARG  # count
    assert L.msm_hash_to_field(group, 0, buf, buf, offs, 0, None, 0, 2, tag, 3, 2, 0, 0, None) == MSM_E_ARG  # overlap
    # a device that does not exist, after the argument checks
    assert L.msm_points_map(group, 1 << 20, dst, buf, 2, 2, 0, 0, None) == MSM_E_NODEV
    assert L.msm_points_hash(group, -1, dst, buf, offs, 0, None, 0, 2, tag, 3, 0, 0, 0, None) == MSM_E_NODEV


@pytest.mark.parametrize("group", [1, 2])
def test_wrapper_value_errors(m, group):
    tag = h.DST[group]
    with pytest.raises(ValueError):
        m.ps_hash_to_curve(3, [b"a"], dst_tag=tag)
    with pytest.raises(ValueError):
        m.ps_hash_to_curve(group, b"abcd", dst_tag=tag)  # neither offsets nor msg_len
    with pytest.raises(ValueError):
        m.ps_hash_to_curve(group, b"abcd", offsets=[0, 4], msg_len=4, dst_tag=tag)  # both
    with pytest.raises(ValueError):
        m.ps_hash_to_curve(group, b"abcd", offsets=[0, 3, 2], dst_tag=tag)  # decreasing
    with pytest.raises(ValueError):
        m.ps_hash_to_curve(group, b"abcd", offsets=[-1, 2], dst_tag=tag)  # negative
    with pytest.raises(ValueError):
        m.ps_hash_to_curve(group, b"abcd", offsets=[0, 5], dst_tag=tag)  # short messages
    with pytest.raises(ValueError):
        m.ps_hash_to_curve(group, b"abcde", msg_len=2, dst_tag=tag)  # no multiple
    with pytest.raises(ValueError):
        m.ps_hash_to_curve(group, b"abcd", msg_len=2, aug=b"xyz", aug_len=2, dst_tag=tag)  # short aug
    with pytest.raises(ValueError):
        m.ps_hash_to_curve(group, [b"a"], offsets=[0, 1], dst_tag=tag)  # a list brings its own offsets
    with pytest.raises(ValueError):
        m.ps_hash_to_curve(group, 0x1000, msg_len=32, src_on_device=True, dst_tag=tag)  # n unknown
    with pytest.raises(ValueError):
        m.ps_hash_to_field(group, [b"a"], dst_tag=tag, count=3)
    with pytest.raises(ValueError):
        m.ps_map_to_curve(group, bytes(48 * group), 1, count=2)  # short buffer
    with pytest.raises(ValueError):
        m.ps_map_to_curve(group, bytes(96 * group), 1, count=0)
    with pytest.raises(ValueError):
        m.ps_map_to_curve(0, bytes(96), 1)
    assert m.ps_hash_to_curve(group, [], dst_tag=tag) == b""
    assert m.ps_map_to_curve(group, b"", 0) == b""


# --------------------------------------------------- the host SHA path, sanitized ----
SRC = os.path.join(REPO, "tests", "host", "h2c_host.cpp")
OUT = os.path.join(REPO, "tests", "host", "_build")
HDRS = [os.path.join(REPO, "msm_blst_amd", "csrc", f) for f in ("hash_to_curve.hpp", "hash_to_curve_consts.hpp")]


@pytest.fixture(scope="module")
def h2c_host():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "h2c_host_asan")
    if not (os.path.exists(exe) and all(os.path.getmtime(d) <= os.path.getmtime(exe) for d in [SRC] + HDRS)):
        r = subprocess.run(["g++", "-std=c++17", SRC, "-o", exe, "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror",
                            "-Wno-unused-function", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]

    def run(*args):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
                   UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
        env.pop("LD_PRELOAD", None)  # the sanitizer runtimes are linked statically
        r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
        return r.stdout.split()

    return run


def _hex(b):
    return b.hex() if b else "-"


def test_host_sha_against_hashlib_under_asan_ubsan(h2c_host):
    msgs = [h._bytes(n, n) for n in (0, 1, 55, 56, 63, 64, 65, 119, 120, 128, 1000)]
    assert h2c_host("sha", *[_hex(x) for x in msgs]) == [hashlib.sha256(x).hexdigest() for x in msgs]
    dsts = [h._bytes(n, 250) for n in (0, 43, 255, 256, 300)]
    assert h2c_host("dstprime", *[_hex(d) for d in dsts]) == [h.dst_prime(d).hex() for d in dsts]


@pytest.mark.parametrize("dst_len", [0, 21, 22, 43, 85, 86, 255, 256, 300])
def test_host_template_under_asan_ubsan(h2c_host, dst_len):
    """the b_i blocks the kernel hashes and the tail of the b_0 hash, for DST lengths on
    both sides of every block boundary (33 + len + 1 + 9 bytes: 64 at 21, 128 at 85)"""
    dst = h._bytes(dst_len, 251)
    dp = h.dst_prime(dst)
    b0 = hashlib.sha256(b"b0").digest()
    for i in (1, 2, 255):
        assert h2c_host("bi", _hex(dst), "256", b0.hex(), str(i)) == [hashlib.sha256(b0 + bytes([i]) + dp).hexdigest()]
    assert h2c_host("tail", _hex(dst), "256") == [(b"\x01\x00\x00" + dp).hex()]
