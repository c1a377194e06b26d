"""CPU-side checks of the NTT over group elements (include/msm_mi355x.h: msm_points_ntt,
msm_points_ntt_model, msm_kzg_ctx_create_monomial; msm_blst_amd.ps_ntt, ntt_model,
KZGContext.from_monomial): exported symbols, flag values, argument errors (returned
before any device work), the empty call, the missing-device code, the Python wrapper's
checks -- and the whole schedule of csrc/points_ntt_plan.hpp run on the host with Fr
elements in place of points (ntt_model) against the plain-Python NTT of
tests/fr_inputs.py, under every slice and chunk override, once more as a stand-alone
program under the sanitizers.  No GPU is used; the GPU parity lives in
test_gpu_points_ntt.py."""
import ctypes
import json
import os
import shutil
import subprocess

import pytest

import enc_inputs as ei
import fr_inputs as fi
import mult_inputs as mi
import pntt_inputs as pi

MSM_OK, MSM_E_ARG, MSM_E_NODEV = 0, -1, -3
INVERSE, BITREV = 1, 8
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "points_ntt.json")
vp = ctypes.c_void_p
FLAGS = [(False, False), (True, False), (False, True), (True, True)]


@pytest.fixture(scope="module")
def m():
    import msm_blst_amd as m
    m.lib()
    return m


@pytest.fixture(autouse=True)
def _no_overrides(monkeypatch):
    monkeypatch.delenv("MSM_POINTS_NTT_SLICE", raising=False)
    monkeypatch.delenv("MSM_POINTS_NTT_CHUNK", raising=False)


def _bufs(group, n):
    return (ctypes.c_uint8 * (ei.AFF[group] * n))(), (ctypes.c_uint8 * (ei.AFF[group] * n))()


def test_exported(m):
    L = m.lib()
    for name in ("msm_points_ntt", "msm_points_ntt_model", "msm_kzg_ctx_create_monomial"):
        assert hasattr(L, name), name
    for name in ("ps_ntt", "ntt_model"):
        assert name in m.__all__ and callable(getattr(m, name)) and name in m.__doc__
    assert callable(m.KZGContext.from_monomial) and "from_monomial" in m.__doc__
    assert (m.NTT_INVERSE, m.POLY_BITREV) == (INVERSE, BITREV)
    with open(os.path.join(REPO, "include", "msm_mi355x.h")) as f:
        hdr = f.read()
    assert "MSM_NTT_INVERSE = 1" in hdr and "MSM_POLY_BITREV = 8" in hdr
    assert "prime-order subgroup" in hdr[hdr.index("msm_points_ntt:"):]


@pytest.mark.parametrize("group", [1, 2])
def test_empty_call_touches_nothing(m, group):
    L = m.lib()
    for flags in (0, INVERSE, BITREV, INVERSE | BITREV):
        assert L.msm_points_ntt(group, 0, None, None, 5, 0, flags, 0, 0, None) == MSM_OK
        assert L.msm_points_ntt(group, 0, None, None, 0, 0, flags, 1, 1, None) == MSM_OK
    assert m.ps_ntt(group, b"", 4, 0) == b""


@pytest.mark.parametrize("group", [1, 2])
def test_argument_errors(m, group):
    L = m.lib()
    src, dst = _bufs(group, 8)

    def call(*a):
        rc = L.msm_points_ntt(*a)
        if rc == MSM_E_ARG:
            assert L.msm_last_error()
        return rc

    assert call(group, 0, None, src, 2, 2, 0, 0, 0, None) == MSM_E_ARG  # NULL dst
    assert b"null" in L.msm_last_error()
    assert call(group, 0, dst, None, 2, 2, 0, 0, 0, None) == MSM_E_ARG  # NULL src
    assert b"null" in L.msm_last_error()
    assert call(group, 0, dst, src, 25, 1, 0, 0, 0, None) == MSM_E_ARG  # log_n > 24
    assert b"log_n" in L.msm_last_error()
    assert call(group, 0, None, None, 25, 0, 0, 0, 0, None) == MSM_E_ARG
    assert call(group, 0, dst, src, 3, (1 << 37) + 1, 0, 0, 0, None) == MSM_E_ARG  # batch n > 2^40
    assert b"batch" in L.msm_last_error()
    assert call(group, 0, dst, src, 24, (1 << 16) + 1, 0, 0, 0, None) == MSM_E_ARG
    for flags in (2, 4, 16, INVERSE | 0x100):  # unknown flag bits
        assert call(group, 0, dst, src, 2, 2, flags, 0, 0, None) == MSM_E_ARG
        assert b"flag" in L.msm_last_error()
    assert bytes(dst) == bytes(len(dst))
    # a dst that overlaps src without equalling it; misaligned device pointers
    base = ctypes.addressof(src)
    assert call(group, 0, vp(base + ei.AFF[group]), src, 2, 1, 0, 0, 0, None) == MSM_E_ARG
    assert b"overlap" in L.msm_last_error()
    assert call(group, 0, vp(0x7f0000001000 + 96), vp(0x7f0000001000), 2, 1, 0, 1, 1, None) == MSM_E_ARG
    assert b"overlap" in L.msm_last_error()
    assert call(group, 0, vp(base + 1), src, 2, 2, 0, 0, 1, None) == MSM_E_ARG
    assert b"aligned" in L.msm_last_error()
    assert call(group, 0, dst, vp(base + 2), 2, 2, 0, 1, 0, None) == MSM_E_ARG
    assert b"aligned" in L.msm_last_error()


def test_bad_group(m):
    L = m.lib()
    src, dst = _bufs(2, 4)
    for group in (0, 3, -1):
        assert L.msm_points_ntt(group, 0, dst, src, 2, 1, 0, 0, 0, None) == MSM_E_ARG
        assert b"group" in L.msm_last_error()
        assert L.msm_points_ntt(group, 0, None, None, 2, 0, 0, 0, 0, None) == MSM_E_ARG


@pytest.mark.parametrize("group", [1, 2])
def test_no_such_device(m, group):
    L = m.lib()
    src, dst = _bufs(group, 4)
    nd = m.device_count()
    for dev in (nd, -1):
        assert L.msm_points_ntt(group, dev, dst, src, 2, 1, 0, 0, 0, None) == MSM_E_NODEV
        assert L.msm_points_ntt(group, dev, src, src, 0, 4, INVERSE, 0, 0, None) == MSM_E_NODEV
    assert bytes(dst) == bytes(len(dst))
    with pytest.raises(m.MsmError):
        m.ps_ntt(group, bytes(src), 2, device=nd)


def test_monomial_context_argument_errors(m):
    L = m.lib()
    h = vp()
    srs, tau = (ctypes.c_uint8 * (96 * 4))(), (ctypes.c_uint8 * 192)()
    create = L.msm_kzg_ctx_create_monomial
    assert create(None, 0, 2, srs, 0, tau, 0, None) == MSM_E_ARG
    assert create(ctypes.byref(h), 0, 2, None, 0, tau, 0, None) == MSM_E_ARG
    assert create(ctypes.byref(h), 0, 2, srs, 0, None, 0, None) == MSM_E_ARG
    assert b"null" in L.msm_last_error()
    assert create(ctypes.byref(h), 0, 21, srs, 0, tau, 0, None) == MSM_E_ARG
    assert b"log_n" in L.msm_last_error()
    assert create(ctypes.byref(h), 0, 2, srs, 0, tau, 1, None) == MSM_E_ARG
    assert b"flag" in L.msm_last_error()
    assert create(ctypes.byref(h), 0, 2, vp(ctypes.addressof(srs) + 1), 1, tau, BITREV, None) == MSM_E_ARG
    assert b"aligned" in L.msm_last_error()
    assert create(ctypes.byref(h), m.device_count(), 2, srs, 0, tau, BITREV, None) == MSM_E_NODEV
    assert not h.value
    with pytest.raises(ValueError):
        m.KZGContext.from_monomial(21, bytes(96), bytes(192))
    with pytest.raises(ValueError):
        m.KZGContext.from_monomial(2, bytes(96 * 3), bytes(192))  # 4 points needed
    with pytest.raises(ValueError):
        m.KZGContext.from_monomial(2, bytes(96 * 4), bytes(191))


class _FakeLib:
    def __init__(self):
        self.calls = []

    def msm_points_ntt(self, *a):
        self.calls.append(a)
        return 0

    def msm_kzg_ctx_create_monomial(self, *a):
        self.calls.append(a)
        return 0

    def msm_kzg_ctx_destroy(self, h):
        pass


def test_wrapper_marshalling_and_checks(m, monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(m, "lib", lambda: fake)
    pts = bytes(range(96)) * 8
    out = m.ps_ntt(1, pts, 2, 2)
    assert len(out) == 8 * 96
    group, device, dst, src, log_n, batch, flags, s_dev, d_dev, stream = fake.calls[-1]
    assert (group, device, log_n, batch, flags, s_dev, d_dev, stream) == (1, 0, 2, 2, 0, 0, 0, None)
    assert bytes(src) == pts and ctypes.sizeof(dst) == 8 * 96
    m.ps_ntt(2, bytes(192 * 8), 3, inverse=True)
    assert fake.calls[-1][4:7] == (3, 1, INVERSE)
    m.ps_ntt(2, bytes(192 * 8), 3, bitrev=True)
    assert fake.calls[-1][4:7] == (3, 1, BITREV)
    m.ps_ntt(1, pts, 3, inverse=True, bitrev=True)
    assert fake.calls[-1][4:7] == (3, 1, INVERSE | BITREV)
    assert m.ps_ntt(2, pts, 0, 4) == bytes(4 * 192)  # log_n = 0: batch points
    # device source and destination (which may be the source)
    assert m.ps_ntt(2, 0x7f0000001000, 10, 3, inverse=True, src_on_device=True, dst=0x7f0000001000, device=1,
                    stream=0x55) is None
    assert fake.calls[-1] == (2, 1, 0x7f0000001000, 0x7f0000001000, 10, 3, INVERSE, 1, 1, 0x55)
    ncalls = len(fake.calls)
    with pytest.raises(ValueError):
        m.ps_ntt(1, pts, 4)  # 8 points given
    with pytest.raises(ValueError):
        m.ps_ntt(1, pts, 2, 3)
    with pytest.raises(ValueError):
        m.ps_ntt(3, pts, 1)
    with pytest.raises(ValueError):
        m.ps_ntt(1, pts, 25)
    with pytest.raises(ValueError):
        m.ps_ntt(1, pts, -1)
    with pytest.raises(ValueError):
        m.ps_ntt(1, pts, 2, -1)
    assert len(fake.calls) == ncalls
    ctx = m.KZGContext.from_monomial(3, pts, bytes(192), bitrev=True, device=2, stream=0x77)
    h, device, log_n, src, on_dev, tau, flags, stream = fake.calls[-1]
    assert (device, log_n, on_dev, flags, stream) == (2, 3, 0, BITREV, 0x77) and bytes(src) == pts
    assert (ctx.log_n, ctx.n, ctx.bitrev, ctx.device) == (3, 8, True, 2)
    m.KZGContext.from_monomial(3, 0x7f0000001000, bytes(192), srs_on_device=True)
    assert fake.calls[-1][3:5] == (0x7f0000001000, 1) and fake.calls[-1][6] == 0


# ------------------------------------------------------------ the host model ----
def _vals(log_n):
    v = fi.rand_values(1 << log_n, 4100 + log_n)
    if log_n >= 2:
        v[1], v[-1] = 0, fi.R - 1
    return v


@pytest.mark.parametrize("slice_,chunk", [(None, None), ("1", None), ("3", None), (None, "4"), ("3", "1"), ("5", "24")])
@pytest.mark.parametrize("log_n", range(8))
def test_model_against_the_oracle(m, monkeypatch, log_n, slice_, chunk):
    """the plan's maps, levels, pairs, exponents, n^-1 pass and slices with Fr elements:
    all four flag combinations against fr_inputs.ntt"""
    if slice_:
        monkeypatch.setenv("MSM_POINTS_NTT_SLICE", slice_)
    if chunk:
        monkeypatch.setenv("MSM_POINTS_NTT_CHUNK", chunk)
    v = _vals(log_n)
    for inverse, bitrev in FLAGS:
        got = m.ntt_model(fi.pack(v), log_n, inverse=inverse, bitrev=bitrev)
        assert fi.unpack(got) == pi.ntt_scalars(v, log_n, inverse=inverse, bitrev=bitrev), (inverse, bitrev)


@pytest.mark.parametrize("log_n", [0, 1, 4, 9])
def test_model_identities(m, log_n):
    x = fi.pack(_vals(log_n))
    assert m.ntt_model(m.ntt_model(x, log_n), log_n, inverse=True) == x
    assert m.ntt_model(m.ntt_model(x, log_n, inverse=True), log_n) == x
    assert m.ntt_model(m.ntt_model(x, log_n, inverse=True, bitrev=True), log_n, bitrev=True) == x
    n = 1 << log_n
    nat = m.ntt_model(x, log_n, inverse=True)
    rev = m.ntt_model(x, log_n, inverse=True, bitrev=True)
    assert all(rev[32 * pi.brev(j, log_n):][:32] == nat[32 * j:32 * j + 32] for j in range(n))


def test_model_argument_errors(m):
    L = m.lib()
    buf = (ctypes.c_uint8 * 64)()
    assert L.msm_points_ntt_model(17, 0, buf, buf) == MSM_E_ARG
    assert b"log_n" in L.msm_last_error()
    assert L.msm_points_ntt_model(1, 2, buf, buf) == MSM_E_ARG
    assert b"flag" in L.msm_last_error()
    assert L.msm_points_ntt_model(1, 0, None, buf) == MSM_E_ARG
    assert L.msm_points_ntt_model(1, 0, buf, None) == MSM_E_ARG
    with pytest.raises(ValueError):
        m.ntt_model(bytes(32), 1)
    with pytest.raises(ValueError):
        m.ntt_model(bytes(32), 17)
    # in place
    v = _vals(1)
    b = (ctypes.c_uint8 * 64).from_buffer_copy(fi.pack(v))
    assert L.msm_points_ntt_model(1, 0, b, b) == MSM_OK
    assert fi.unpack(bytes(b)) == fi.ntt(v)


# ---------------------------------------------------------------- the golden ----
def test_golden_scalars_reproduce():
    """the recorded points are the Python oracle's: inputs [a_j]G, outputs [ntt(a)_k]G"""
    with open(GOLDEN) as f:
        g = json.load(f)
    log_n = g["log_n"]
    a = pi.golden_scalars()
    assert g["scalars"] == [hex(v) for v in a] and log_n == pi.GOLDEN_LOG_N and 0 in a
    for group in (1, 2):
        e = g["groups"][str(group)]

        def comp(k):
            return ei.encode_point(group, mi.smul(group, ei.GEN[group], k % fi.R), True).hex()

        assert e["inputs"] == [comp(k) for k in a]
        assert e["forward"] == [comp(k) for k in pi.ntt_scalars(a, log_n)]
        assert e["inverse"] == [comp(k) for k in pi.ntt_scalars(a, log_n, inverse=True)]
    assert fi.ntt(a) == fi.ntt_slow(a)


# ------------------------------------------------- under the sanitizers ----
MAIN = r"""
// the model of points_ntt_model.hpp on the plan of points_ntt_plan.hpp, log_n = 0 .. 6, all
// flag combinations, odd slice and chunk sizes and batches, against the O(n^2) sums
#include <cstdio>
#include <vector>

#include "host_fr.hpp"
#include "points_ntt_model.hpp"
#include "points_ntt_plan.hpp"

using namespace msm;

int main() {
  int runs = 0;
  for (int log_n = 0; log_n <= 6; ++log_n) {
    const size_t n = (size_t)1 << log_n;
    const hfr::Fr w = hfr::root_of_unity((unsigned)log_n), wi = hfr::inverse(w);
    const hfr::Fr ninv = hfr::inverse(hfr::from_u64(n));
    for (size_t batch : {(size_t)1, (size_t)3})
      for (int flags : {0, PN_INVERSE, PN_BITREV, PN_INVERSE | PN_BITREV})
        for (size_t slice : {(size_t)1, (size_t)3, (size_t)7, (size_t)1 << 18})
          for (size_t chunk : {(size_t)1, (size_t)5, (size_t)96, (size_t)1 << 20}) {
            std::vector<hfr::Fr> src(batch * n), dst(batch * n), want(batch * n);
            for (size_t i = 0; i < src.size(); ++i) src[i] = hfr::from_u64(0x9e3779b97f4a7c15ull * (i + 1) + log_n);
            if (n > 2) src[2] = hfr::from_u64(0);
            const bool inv = flags & PN_INVERSE, rev = flags & PN_BITREV;
            for (size_t b = 0; b < batch; ++b)
              for (size_t k = 0; k < n; ++k) {
                hfr::Fr acc = hfr::from_u64(0);
                const uint64_t e1[4] = {k, 0, 0, 0};
                const hfr::Fr wk = hfr::pow(inv ? wi : w, e1);
                hfr::Fr p = hfr::ONE;
                for (size_t j = 0; j < n; ++j) {
                  const size_t at = rev && !inv ? pn_bitrev(j, log_n) : j;
                  acc = hfr::add(acc, hfr::mul(src[b * n + at], p));
                  p = hfr::mul(p, wk);
                }
                if (inv) acc = hfr::mul(acc, ninv);
                want[b * n + (rev && inv ? pn_bitrev(k, log_n) : k)] = acc;
              }
            pn_model(log_n, flags, batch, dst.data(), src.data(), chunk, slice);
            for (size_t i = 0; i < dst.size(); ++i)
              if (!hfr::eq(dst[i], want[i])) {
                printf("MISMATCH log_n %d flags %d batch %zu slice %zu chunk %zu at %zu\n", log_n, flags, batch, slice,
                       chunk, i);
                return 1;
              }
            pn_model(log_n, flags, batch, src.data(), src.data(), chunk, slice);  // in place
            for (size_t i = 0; i < dst.size(); ++i)
              if (!hfr::eq(src[i], want[i])) {
                printf("MISMATCH in place log_n %d flags %d\n", log_n, flags);
                return 1;
              }
            ++runs;
          }
  }
  printf("OK %d\n", runs);
  return 0;
}
"""


def test_model_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.fail("g++ missing")
    src = tmp_path / "points_ntt_main.cpp"
    src.write_text(MAIN)
    exe = tmp_path / "points_ntt_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "msm_blst_amd", "csrc"), str(src),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == f"OK {7 * 2 * 4 * 4 * 4}" and "runtime error" not in r.stderr
