"""CPU-side checks of the segmented sums and MSMs (include/msm_mi355x.h:
msm_points_msm_segments, msm_segments_plan; msm_blst_amd.ps_msm_segments /
ps_sum_segments): exported symbols, argument errors (returned before any device
work), the empty call, the missing-device code, the Python wrappers' checks, the
host plan (pieces) -- through the ABI and, under AddressSanitizer and UBSan, in a
stand-alone program -- and the plain-Python oracle of tests/seg_inputs.py against
the reference's recorded answers (tests/golden/points_segments.json).  No GPU is
used; the GPU parity lives in test_gpu_points_segments.py."""
import ctypes
import os
import shutil
import subprocess

import pytest

import enc_inputs as ei
import seg_inputs as si

MSM_OK, MSM_E_ARG, MSM_E_NODEV = 0, -1, -3
vp = ctypes.c_void_p
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def m():
    import msm_blst_amd as m
    m.lib()
    return m


def _bufs(group, n, k, stride=32):
    pts = (ctypes.c_uint8 * (ei.AFF[group] * n))()
    sc = (ctypes.c_uint8 * (stride * n))()
    dst = (ctypes.c_uint8 * (ei.AFF[group] * k))()
    return pts, sc, dst


def _offs(values):
    return (ctypes.c_size_t * len(values))(*values)


def edge_offsets(L):
    """segments of length 0, 1, L-1, L, L+1, 2L+1 with leading, trailing and consecutive empty ones"""
    return si.offsets_of([0, 0, 1, L - 1, L, 0, 0, L + 1, 2 * L + 1, 0], first=3)


def test_exported(m):
    L = m.lib()
    for name in ("msm_points_msm_segments", "msm_segments_plan", "msm_segments_piece"):
        assert hasattr(L, name)
    for name in ("ps_msm_segments", "ps_sum_segments"):
        assert name in m.__all__ and callable(getattr(m, name)) and name in m.__doc__
    assert len(L.msm_points_msm_segments.argtypes) == 13


@pytest.mark.parametrize("group", [1, 2])
def test_empty_call_touches_nothing(m, group):
    L = m.lib()
    assert L.msm_points_msm_segments(group, 0, None, None, None, None, 0, 255, 32, 0, 0, 0, None) == MSM_OK
    assert L.msm_points_msm_segments(group, 0, None, None, None, None, 0, 0, 0, 0, 1, 1, None) == MSM_OK
    assert m.ps_msm_segments(group, b"", b"", [0]) == b""
    assert m.ps_sum_segments(group, b"", [5]) == b""


@pytest.mark.parametrize("group", [1, 2])
def test_argument_errors(m, group):
    L = m.lib()
    pts, sc, dst = _bufs(group, 4, 2)
    o = _offs([0, 1, 4])

    def call(*a):
        rc = L.msm_points_msm_segments(*a)
        if rc == MSM_E_ARG:
            assert L.msm_last_error()
        return rc

    assert call(group, 0, None, pts, sc, o, 2, 255, 32, 0, 0, 0, None) == MSM_E_ARG  # NULL dst
    assert b"null" in L.msm_last_error()
    assert call(group, 0, dst, None, sc, o, 2, 255, 32, 0, 0, 0, None) == MSM_E_ARG  # NULL points
    assert call(group, 0, dst, pts, sc, None, 2, 255, 32, 0, 0, 0, None) == MSM_E_ARG  # NULL offsets
    assert call(group, 0, dst, pts, None, None, 2, 0, 0, 0, 0, 0, None) == MSM_E_ARG
    assert call(group, 0, dst, pts, sc, _offs([0, 3, 2]), 2, 255, 32, 0, 0, 0, None) == MSM_E_ARG  # decreasing
    assert b"offsets" in L.msm_last_error()
    assert call(group, 0, dst, pts, None, _offs([2, 1, 4]), 2, 0, 0, 0, 0, 0, None) == MSM_E_ARG
    assert call(group, 0, dst, pts, sc, o, 2, 257, 33, 0, 0, 0, None) == MSM_E_ARG  # nbits > 256
    assert b"nbits" in L.msm_last_error()
    assert call(group, 0, dst, pts, sc, o, 2, 255, 31, 0, 0, 0, None) == MSM_E_ARG  # stride too short
    assert b"stride" in L.msm_last_error()
    assert call(group, 0, dst, pts, sc, o, 2, 9, 1, 0, 0, 0, None) == MSM_E_ARG
    assert call(group, 0, dst, pts, sc, o, 2, 255, 32, 1, 0, 0, None) == MSM_E_ARG  # non-zero flags
    assert b"flag" in L.msm_last_error()
    assert call(group, 0, dst, pts, None, o, 2, 0, 0, 0x100, 0, 0, None) == MSM_E_ARG
    assert bytes(dst) == bytes(len(dst))
    # host ranges: dst on the points, dst on the scalars; misaligned device pointers
    base = ctypes.addressof(pts)
    assert call(group, 0, vp(base), pts, sc, o, 2, 255, 32, 0, 0, 0, None) == MSM_E_ARG
    assert b"overlap" in L.msm_last_error()
    assert call(group, 0, vp(base + 3 * ei.AFF[group]), pts, None, o, 2, 0, 0, 0, 0, 0, None) == MSM_E_ARG
    assert b"overlap" in L.msm_last_error()
    big = (ctypes.c_uint8 * (ei.AFF[group] * 8))()  # scalars of stride 96 G, dst on the last of them
    assert call(group, 0, vp(ctypes.addressof(big) + 3 * ei.AFF[group]), pts, big, o, 2, 255, ei.AFF[group], 0, 0, 0,
                None) == MSM_E_ARG
    assert b"overlap" in L.msm_last_error()
    assert call(group, 0, vp(base + 1), pts, sc, o, 2, 255, 32, 0, 0, 1, None) == MSM_E_ARG
    assert call(group, 0, dst, vp(base + 2), sc, o, 2, 255, 32, 0, 1, 0, None) == MSM_E_ARG
    assert bytes(dst) == bytes(len(dst))


def test_bad_group(m):
    L = m.lib()
    pts, sc, dst = _bufs(2, 4, 2)
    o = _offs([0, 1, 4])
    for group in (0, 3, -1):
        assert L.msm_points_msm_segments(group, 0, dst, pts, sc, o, 2, 255, 32, 0, 0, 0, None) == MSM_E_ARG
        assert b"group" in L.msm_last_error()
        assert L.msm_points_msm_segments(group, 0, None, None, None, None, 0, 255, 32, 0, 0, 0, None) == MSM_E_ARG


@pytest.mark.parametrize("group", [1, 2])
def test_no_such_device(m, group):
    L = m.lib()
    pts, sc, dst = _bufs(group, 4, 2)
    o = _offs([0, 1, 4])
    nd = m.device_count()
    for dev in (nd, -1):
        assert L.msm_points_msm_segments(group, dev, dst, pts, sc, o, 2, 255, 32, 0, 0, 0, None) == MSM_E_NODEV
        assert L.msm_points_msm_segments(group, dev, dst, pts, None, o, 2, 0, 0, 0, 0, 0, None) == MSM_E_NODEV
    assert bytes(dst) == bytes(len(dst))
    with pytest.raises(m.MsmError):
        m.ps_msm_segments(group, bytes(pts), bytes(sc), [0, 1, 4], device=nd)
    with pytest.raises(m.MsmError):
        m.ps_sum_segments(group, bytes(pts), [0, 1, 4], device=nd)


class _FakeLib:
    def __init__(self):
        self.calls = []

    def msm_points_msm_segments(self, *a):
        self.calls.append(a)
        return 0


def test_wrapper_marshalling_and_checks(m, monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(m, "lib", lambda: fake)
    pts, sc = bytes(range(96)) * 3, bytes(range(32)) * 3
    out = m.ps_msm_segments(1, pts, sc, [0, 1, 1, 3])
    assert len(out) == 3 * 96
    group, device, dst, p, s, o, k, nbits, stride, flags, s_dev, d_dev, stream = fake.calls[-1]
    assert (group, device, k, nbits, stride, flags, s_dev, d_dev, stream) == (1, 0, 3, 255, 32, 0, 0, 0, None)
    assert bytes(p) == pts and bytes(s) == sc and ctypes.sizeof(dst) == 3 * 96 and list(o) == [0, 1, 1, 3]
    # any sequence of ints; narrow scalars packed tight: the last scalar may end the buffer
    out = m.ps_msm_segments(2, bytes(3 * 192), bytes(2 * 9 + 8), range(1, 4), nbits=64, stride=9)
    assert len(out) == 2 * 192 and fake.calls[-1][6:10] == (2, 64, 9, 0) and list(fake.calls[-1][5]) == [1, 2, 3]
    # plain sums: no scalars, nbits and stride zero
    out = m.ps_sum_segments(1, pts, (0, 3))
    assert len(out) == 96 and fake.calls[-1][4] is None and fake.calls[-1][6:10] == (1, 0, 0, 0)
    # device sources and destination
    assert m.ps_msm_segments(2, 0x7f0000001000, 0x7f0000003000, [0, 5], src_on_device=True, dst=0x7f0000002000,
                             device=1, stream=0x55) is None
    c = fake.calls[-1]
    assert c[:5] == (2, 1, 0x7f0000002000, 0x7f0000001000, 0x7f0000003000) and c[6:] == (1, 255, 32, 0, 1, 1, 0x55)
    assert m.ps_sum_segments(1, 0x7f0000001000, [0, 5], src_on_device=True, dst=0x7f0000002000) is None
    ncalls = len(fake.calls)
    with pytest.raises(ValueError):
        m.ps_msm_segments(1, pts, sc, [0, 4])  # 3 points given
    with pytest.raises(ValueError):
        m.ps_sum_segments(1, pts, [0, 4])
    with pytest.raises(ValueError):
        m.ps_msm_segments(1, pts + pts, sc, [0, 4])  # 3 scalars given
    with pytest.raises(ValueError):
        m.ps_msm_segments(1, pts, sc, [0, 2, 1])  # decreasing
    with pytest.raises(ValueError):
        m.ps_sum_segments(1, pts, [-1, 2])
    with pytest.raises(ValueError):
        m.ps_sum_segments(1, pts, [])
    with pytest.raises(ValueError):
        m.ps_msm_segments(1, pts, sc, [0, 3], nbits=64, stride=7)
    with pytest.raises(ValueError):
        m.ps_msm_segments(1, pts, sc, [0, 3], nbits=257, stride=40)
    with pytest.raises(ValueError):
        m.ps_msm_segments(3, pts, sc, [0, 1])
    with pytest.raises(ValueError):
        m.ps_msm_segments(1, pts, None, [0, 1])
    assert len(fake.calls) == ncalls


@pytest.mark.parametrize("L", [1, 3, 64])
def test_pieces(m, L):
    o = edge_offsets(L)
    got = m.segments_plan(o, L)
    assert got == si.pieces(o, L)
    # each point once and in order, never across a segment, never longer than L
    at = o[0]
    for start, count, seg in got:
        assert start == at and 1 <= count <= L and o[seg] <= start and start + count <= o[seg + 1]
        at += count
        if at < o[-1] and at == o[seg + 1]:  # the next piece opens the next non-empty segment
            nxt = next(j for j in range(seg + 1, len(o) - 1) if o[j + 1] > o[j])
            assert o[nxt] == at
    assert at == o[-1]
    assert len(got) == sum(-(-(b - a) // L) for a, b in zip(o, o[1:]))
    # the count alone (no arrays), a short capacity, and the errors
    lib = m.lib()
    n = ctypes.c_size_t(99)
    assert lib.msm_segments_plan(_offs(o), len(o) - 1, L, ctypes.byref(n), None, None, None, 0) == MSM_OK
    assert n.value == len(got)
    st = (ctypes.c_size_t * 3)(7, 7, 7)
    assert lib.msm_segments_plan(_offs(o), len(o) - 1, L, ctypes.byref(n), st, None, None, 2) == MSM_OK
    assert list(st) == [got[0][0], got[1][0], 7]
    assert lib.msm_segments_plan(_offs(o), len(o) - 1, 0, ctypes.byref(n), None, None, None, 0) == MSM_E_ARG
    assert lib.msm_segments_plan(_offs([0, 2, 1]), 2, L, ctypes.byref(n), None, None, None, 0) == MSM_E_ARG
    assert lib.msm_segments_plan(_offs([4]), 0, L, ctypes.byref(n), None, None, None, 0) == MSM_OK and n.value == 0
    assert m.segments_plan([0, 0, 0], L) == []


def test_piece_rule(m, monkeypatch):
    """a piece for every resident lane (pair), L in [1, 64]; the variable overrides"""
    lib = m.lib()
    monkeypatch.delenv("MSM_POINTS_SEGMENTS_PIECE", raising=False)
    monkeypatch.delenv("MSM_POINTS_SEGMENTS_CHUNK", raising=False)
    lanes = 256 * 4 * 2 * 64
    for g in (1, 2):
        assert lib.msm_segments_piece(g, 0) == 1 and lib.msm_segments_piece(g, 1000) == 1
        assert lib.msm_segments_piece(g, 2 * lanes // g - 1) == 1
        assert lib.msm_segments_piece(g, 2 * lanes // g) == 2
        assert 1 <= lib.msm_segments_piece(g, 1 << 40) <= 64
    assert lib.msm_segments_piece(1, 1 << 20) == 8
    monkeypatch.setenv("MSM_POINTS_SEGMENTS_PIECE", "8")
    assert lib.msm_segments_piece(1, 10) == 8
    monkeypatch.setenv("MSM_POINTS_SEGMENTS_PIECE", "1000")
    assert lib.msm_segments_piece(2, 10) == 64


PLAN_MAIN = r"""
#include <stdio.h>
int main() {
  const size_t Ls[] = {1, 3, 64};
  size_t total = 0;
  for (size_t L : Ls) {
    const size_t len[] = {0, 0, 1, L - 1, L, 0, 0, L + 1, 2 * L + 1, 0};
    std::vector<size_t> o{3};
    for (size_t n : len) o.push_back(o.back() + n);
    const size_t k = o.size() - 1;
    if (!seg_offsets_ok(o.data(), k)) return 2;
    // the whole range, then every chunk size that puts a boundary inside a segment
    for (size_t C = 1; C <= o[k] - o[0] + 1; ++C) {
      std::vector<size_t> seen;
      size_t want = 0;
      for (size_t lo = o[0]; lo < o[k]; lo += C) {
        const size_t hi = std::min(lo + C, o[k]);
        size_t j = 0;
        while (j < k && o[j + 1] <= lo) ++j;
        std::vector<size_t> st(hi - lo), ct(hi - lo), sg(hi - lo);
        size_t w = 0;
        const size_t np = seg_cut(o.data(), k, L, lo, hi, j, [&](size_t s, size_t c, size_t seg) {
          st[w] = s, ct[w] = c, sg[w] = seg;
          ++w;
        });
        if (np != w) return 3;
        for (size_t p = 0; p < np; ++p) {
          if (ct[p] < 1 || ct[p] > L || st[p] < o[sg[p]] || st[p] + ct[p] > o[sg[p] + 1]) return 4;
          for (size_t i = 0; i < ct[p]; ++i) seen.push_back(st[p] + i);
        }
        want += np;
      }
      if (seen.size() != o[k] - o[0]) return 5;
      for (size_t i = 0; i < seen.size(); ++i)
        if (seen[i] != o[0] + i) return 6;
      total += want;
    }
    std::vector<size_t> bad{0, 2, 1};
    if (seg_offsets_ok(bad.data(), 2)) return 7;
    // the chunk planner at every C from 1 to total + 1
    for (size_t C = 1; C <= o[k] - o[0] + 1; ++C)
      if (int rc = plan_chunks(o, L, C)) return rc;
  }
  const std::vector<size_t> empty(8, 5);  // 7 segments, all empty
  for (size_t C : {1, 3, 7, 8})
    if (int rc = plan_chunks(empty, 3, C)) return rc;
  printf("ok %zu\n", total);
  return 0;
}
"""

# SegPlanner over one offsets array at chunk knob C: the covering, the bounds, the runs, and a
# simulation in plain integers of what the engines do with a plan (exit codes 10 ..)
PLAN_CHUNKS = r"""
#include <stdint.h>
#include <vector>
#include "segments_plan.hpp"
using namespace msm;
static uint64_t worth(size_t i) { return (uint64_t)i * i + 1; }
static int plan_chunks(const std::vector<size_t> &o, size_t L, size_t chunk) {
  const size_t k = o.size() - 1, total = o[k] - o[0];
  const SegSizes z = seg_sizes(total, k, chunk);
  if (z.C != std::min(std::max(total, k), chunk) || z.CP != std::min(z.C, std::max<size_t>(total, 1))) return 10;
  if (z.pmax != z.CP + 1 || z.META != z.pmax * sizeof(SegMeta) + z.C * sizeof(uint32_t)) return 11;
  SegPlanner pl;
  std::vector<uint64_t> got;  // the value of every segment, in the order written
  uint64_t carry = 0;
  bool carried = false;
  size_t at = o[0], seg = 0;
  pl.begin(o.data(), k, z, L, "test");
  while (pl.next()) {
    // the chunks cover the points and the segments in order, without gap or overlap
    if (pl.i != at || pl.j != seg || pl.e < pl.i || pl.je < pl.j || pl.e > o[k] || pl.je > k) return 12;
    if (pl.cnt() == 0 && pl.nseg() == 0) return 13;  // (no progress)
    at = pl.e, seg = pl.je;
    const size_t np = pl.np(), nseg = pl.nseg();
    if (nseg > z.C || pl.cnt() > z.CP || np > z.pmax) return 14;
    if (pl.meta.size() != np || pl.src.size() != nseg || pl.npieces() + pl.pc != np) return 15;
    if ((pl.pc != 0) != carried) return 16;  // the carried partial is there when a carry came in, and first
    for (size_t j = pl.j; j < pl.je; ++j)
      if (o[j + 1] > pl.e) return 17;  // a segment that is written ends in the chunk
    if (pl.je < k && o[pl.je + 1] <= pl.e && nseg < z.C) return 18;  // and one that ends in it is written
    // the partials: the carried one holds the value carried in, a piece sums its points
    std::vector<uint64_t> part(np, 0);
    size_t pt = pl.i;
    for (size_t p = 0; p < np; ++p) {
      const SegMeta &m = pl.meta[p];
      if (p < pl.pc) {
        if (m.start || m.count) return 19;
        part[p] = carry;
        continue;
      }
      if (m.count < 1 || m.count > L || pl.i + m.start != pt) return 20;  // the pieces tile [i, e)
      for (size_t q = 0; q < m.count; ++q) part[p] += worth(pt + q);
      pt += m.count;
    }
    if (pt != pl.e) return 21;
    // the runs are contiguous: rel counts 0 .. len - 1 within each
    size_t maxrun = 0;
    for (size_t p = 0; p < np;) {
      const size_t len = pl.meta[p].len;
      if (len < 1 || p + len > np) return 22;
      for (size_t r = 0; r < len; ++r)
        if (pl.meta[p + r].rel != r || pl.meta[p + r].len != len) return 23;
      maxrun = std::max(maxrun, len);
      p += len;
    }
    if (maxrun != pl.maxrun) return 24;
    // the merge of the engines: at step s the partial at rel r (a multiple of 2 s) takes in the one at r + s
    for (size_t step = 1; step < pl.maxrun; step *= 2)
      for (size_t p = 0; p < np; ++p) {
        const SegMeta &m = pl.meta[p];
        if ((m.rel & (2 * step - 1)) == 0 && m.rel + step < m.len) part[p] += part[p + step];
      }
    // the gather, and the next carry
    for (size_t t = 0; t < nseg; ++t) {
      const size_t j = pl.j + t;
      const bool is_empty = o[j + 1] == o[j];
      if (is_empty != (pl.src[t] == ~0u)) return 25;
      if (!is_empty && (pl.src[t] >= np || pl.meta[pl.src[t]].rel != 0)) return 26;
      got.push_back(is_empty ? 0 : part[pl.src[t]]);
    }
    carried = pl.carry();
    if (carried != (pl.je < k && o[pl.je] < pl.e)) return 27;  // a segment is left open where points of it were summed
    if (carried) {
      if (pl.open_src >= np || pl.meta[pl.open_src].rel != 0) return 28;
      carry = part[pl.open_src];
    }
  }
  if (at != o[k] || seg != k || got.size() != k || carried) return 29;
  for (size_t j = 0; j < k; ++j) {  // the direct sums
    uint64_t want = 0;
    for (size_t i = o[j]; i < o[j + 1]; ++i) want += worth(i);
    if (got[j] != want) return 30;
  }
  // a plan that cannot fit its buffers is refused (at the first chunk that has a point)
  SegSizes small = z;
  small.pmax = 0, small.CP = 0;
  pl.begin(o.data(), k, small, L, "test");
  if (total) {
    try {
      while (pl.next()) {
      }
      return 31;
    } catch (const std::runtime_error &err) {
      if (std::string(err.what()) != "test: plan larger than its buffers") return 32;
    }
  }
  return 0;
}
"""


def test_planner_under_sanitizers(tmp_path):
    """csrc/segments_plan.hpp in a stand-alone host program built with ASan + UBSan:
    the edge offsets, whole and cut at every chunk size, by seg_cut and by the chunk
    planner of point_segments.hip and pairing.hip (SegPlanner), whose plans are also
    carried out in plain integers against the direct per-segment sums"""
    if not shutil.which("g++"):
        pytest.fail("g++ missing")
    src = tmp_path / "plan_main.cpp"
    src.write_text(PLAN_CHUNKS + PLAN_MAIN)
    exe = tmp_path / "plan_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "msm_blst_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and not r.stderr


@pytest.mark.parametrize("group", [1, 2])
def test_oracle_reproduces_the_reference(golden, group):
    """seg_inputs.expected (smul and the Jacobian addition in plain integers) against
    the reference's recorded per-segment sums of the golden batch"""
    c = [c for c in golden("points_segments.json")["segments"] if c["group"] == group][0]
    pts, ks, o, ing = si.golden_batch(group)
    assert c["lengths"] == si.GOLDEN_LENGTHS and c["nbits"] == si.GOLDEN_NBITS
    assert c["in_group"] == [j for j in range(len(o) - 1) if ing[j]]
    A = ei.AFF[group]
    want = si.expected(group, pts, ks, o)
    for j, hexs in zip(c["in_group"], c["compressed"]):
        assert ei.encode(group, want[j * A:(j + 1) * A], 1).hex() == hexs, j
    assert ei.fnv(b"".join(want[j * A:(j + 1) * A] for j in c["in_group"])) == c["fnv"]
    # empty segments are infinity, and the batch holds a sum that cancels inside a segment
    for j, n in enumerate(si.GOLDEN_LENGTHS):
        if n == 0:
            assert want[j * A:(j + 1) * A] == bytes(A)
    assert all(k < (1 << si.GOLDEN_NBITS) for k in ks)
    assert si.segment_sum(group, pts[13:15], ks[13:15]) is None
    # a plain sum is the MSM with every scalar 1
    assert si.expected(group, pts[:6], None, [0, 2, 6]) == si.expected(group, pts[:6], [1] * 6, [0, 2, 6])
