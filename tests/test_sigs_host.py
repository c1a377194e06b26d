"""CPU tests of the bulk signature verification (msm_sigs_verify,
msm_sigs_aggregate_verify, msm_sigs_batch_verify, msm_points_in_group): the
plain-integer model against the fixture the reference wrote
(tests/golden/sigs.json), the input hashes, every MSM_E_ARG case (all of them
return before any device work), the Python wrappers' own checks, and the host
plan csrc/sig_plan.hpp against a Python restatement and under the sanitizers.
"""
import ctypes
import os
import random
import shutil
import subprocess

import pytest

import sig_inputs as si

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MSM_E_ARG = -1
ROW_SIG = 0x80000000


@pytest.fixture(scope="module")
def m():
    import msm_blst_amd as m
    return m


@pytest.fixture(scope="module")
def fx(golden):
    return golden("sigs.json")


def forms(name):
    out = []
    if name != "individual_encoded":
        out.append("affine")
    if name in si.ENCODED_TOO:
        out.append("encoded")
    return out


# ------------------------------------------------------------------ fixture ----
def test_fixture_covers_every_table_and_code(fx):
    seen = set()
    for name in si.TABLES:
        for scheme in (1, 2):
            for form in forms(name):
                rec = fx["tables"][name][str(scheme)][form]
                assert len(rec["status"]) == si.nchecks(si.table(name, scheme)), (name, scheme, form)
                seen.update(rec["status"])
    assert seen == {0, 1, 2, 3, 5, 6}


@pytest.mark.parametrize("scheme", [1, 2])
def test_input_hashes(fx, scheme):
    """the inputs the tests build are the inputs the reference judged"""
    for name in si.TABLES:
        for form in forms(name):
            assert si.input_hash(si.table(name, scheme), form == "encoded") == \
                fx["tables"][name][str(scheme)][form]["inputs"], (name, form)


@pytest.mark.parametrize("scheme", [1, 2])
def test_model_against_the_fixture(fx, scheme):
    """The pure-Python pairing affords a subset: the cap is the list the generator
    recorded (at most 9 checks per table, 39 per scheme, products of at most four
    pairs).  It holds every status value and every mode."""
    codes, modes, count = set(), set(), 0
    for name, form, idx in fx["model"]:
        assert len(idx) <= 9
        call = si.table(name, scheme)
        want = fx["tables"][name][str(scheme)][form]["status"]
        for j in idx:
            assert si.model_status(call, j) == want[j], (name, form, j)
            codes.add(want[j]), modes.add(call["mode"])
            count += 1
    assert codes == {0, 1, 2, 3, 5, 6} and modes == {0, 1, 2} and count <= 39


# ------------------------------------------------------------------ MSM_E_ARG ----
def _arrs(n=2):
    st = (ctypes.c_uint8 * n)(*([9] * n))
    nf = ctypes.c_size_t(77)
    pk, sg = (ctypes.c_uint8 * (96 * n))(), (ctypes.c_uint8 * (192 * n))()
    msgs = (ctypes.c_uint8 * (4 * n))()
    return st, nf, pk, sg, msgs


def test_verify_argument_errors(m):
    L = m.lib()
    st, nf, pk, sg, msgs = _arrs()
    tag = b"T"
    good = dict(scheme=1, status=st, nfail=ctypes.byref(nf), pks=pk, pk_off=None, sigs=sg, msgs=msgs, mo=None, ml=4,
                aug=None, al=0, n=2, dst=tag, dl=1, flags=0)

    def call(**kw):
        a = dict(good, **kw)
        return L.msm_sigs_verify(a["scheme"], 0, a["status"], a["nfail"], a["pks"], a["pk_off"], a["sigs"], a["msgs"],
                                 a["mo"], a["ml"], a["aug"], a["al"], a["n"], a["dst"], a["dl"], a["flags"], 0, None)

    dec = (ctypes.c_size_t * 3)(0, 2, 1)
    for bad in (dict(scheme=0), dict(scheme=3), dict(flags=4), dict(flags=8), dict(status=None, nfail=None),
                dict(pks=None), dict(sigs=None), dict(msgs=None), dict(dst=None), dict(pk_off=dec), dict(mo=dec)):
        assert call(**bad) == MSM_E_ARG, bad
        assert bytes(st) == b"\x09\x09" and nf.value == 77, bad  # nothing touched
        assert m.lib().msm_last_error()
    assert call(n=0, pks=None, sigs=None, msgs=None, status=None, nfail=None) == 0  # a count of zero touches nothing
    assert bytes(st) == b"\x09\x09" and nf.value == 77


def test_aggregate_and_batch_argument_errors(m):
    L = m.lib()
    st, nf, pk, sg, msgs = _arrs()
    o = (ctypes.c_size_t * 3)(0, 1, 2)
    dec = (ctypes.c_size_t * 3)(0, 2, 1)
    w = (ctypes.c_uint8 * 64)()

    def agg(scheme=1, offs=o, flags=0, pks=pk, sigs=sg, status=st, n=2):
        return L.msm_sigs_aggregate_verify(scheme, 0, status, ctypes.byref(nf), pks, sigs, msgs, None, 4, None, 0, offs,
                                           n, b"T", 1, flags, 0, None)

    def bat(scheme=1, offs=o, flags=0, scalars=w, nbits=64, stride=8, pks=pk, n=2):
        return L.msm_sigs_batch_verify(scheme, 0, st, ctypes.byref(nf), pks, sg, scalars, nbits, stride, msgs, None, 4,
                                       None, 0, offs, n, b"T", 1, flags, 0, None)

    for r in (agg(scheme=5), agg(offs=None), agg(offs=dec), agg(flags=16), agg(pks=None), agg(sigs=None),
              bat(scheme=0), bat(offs=None), bat(offs=dec), bat(flags=4), bat(nbits=257, stride=64), bat(stride=7),
              bat(stride=(1 << 20) + 1), bat(pks=None)):
        assert r == MSM_E_ARG
    assert bytes(st) == b"\x09\x09" and nf.value == 77
    assert agg(n=0) == 0 and bat(n=0) == 0
    # a bad nbits or stride is an error even when no check is given; NULL scalars make them irrelevant
    assert bat(n=0, nbits=300) == MSM_E_ARG and bat(n=0, stride=1) == MSM_E_ARG
    assert bat(n=0, scalars=None, nbits=300) == 0


def test_in_group_argument_errors(m):
    L = m.lib()
    out = (ctypes.c_uint8 * 2)(7, 7)
    pts = (ctypes.c_uint8 * 192)()
    assert L.msm_points_in_group(3, 0, out, pts, 2, 0, None) == MSM_E_ARG
    assert L.msm_points_in_group(1, 0, None, pts, 2, 0, None) == MSM_E_ARG
    assert L.msm_points_in_group(1, 0, out, None, 2, 0, None) == MSM_E_ARG
    assert L.msm_points_in_group(1, 0, out, ctypes.c_void_p(0x1004), 2, 1, None) == MSM_E_ARG  # misaligned device pointer
    assert L.msm_points_in_group(2, 0, None, None, 0, 0, None) == 0
    assert bytes(out) == b"\x07\x07"


def test_wrapper_checks(m):
    pk, sg = bytes(96 * 2), bytes(192 * 2)
    kw = dict(dst_tag=b"T")
    with pytest.raises(ValueError):
        m.ps_verify(3, pk, sg, [b"a", b"b"], **kw)
    with pytest.raises(ValueError):
        m.ps_verify(1, pk[:100], sg, [b"a", b"b"], **kw)  # short keys
    with pytest.raises(ValueError):
        m.ps_verify(1, pk, sg[:200], [b"a", b"b"], **kw)  # short signatures
    with pytest.raises(ValueError):
        m.ps_verify(1, pk, sg, [b"a", b"b"], pk_offsets=[0, 1], **kw)  # one offset short
    with pytest.raises(ValueError):
        m.ps_verify(1, pk, sg, [b"a", b"b"], pk_offsets=[0, 2, 1], **kw)
    with pytest.raises(ValueError):
        m.ps_verify(2, pk, sg, [b"a", b"b"], **kw)  # min-sig keys are 192 bytes
    with pytest.raises(ValueError):
        m.ps_aggregate_verify(1, pk, sg, [b"a", b"b"], [0, 3], **kw)  # more tuples than messages
    with pytest.raises(ValueError):
        m.ps_aggregate_verify(1, pk, sg, [b"a", b"b"], [], **kw)
    with pytest.raises(ValueError):
        m.ps_batch_verify(1, pk, sg, [b"a", b"b"], [0, 2], scalars=bytes(16), nbits=300, **kw)
    with pytest.raises(ValueError):
        m.ps_batch_verify(1, pk, sg, [b"a", b"b"], [0, 2], scalars=bytes(16), nbits=64, stride=4, **kw)
    with pytest.raises(ValueError):
        m.ps_batch_verify(1, pk, sg, [b"a", b"b"], [0, 2], scalars=bytes(15), nbits=64, **kw)  # short scalars
    with pytest.raises(ValueError):
        m.ps_in_group(3, pk, 2)
    with pytest.raises(ValueError):
        m.ps_in_group(1, pk, 3)
    assert m.ps_in_group(1, b"", 0) == b"" and m.SIG_MIN_PK == 1 and m.SIG_MIN_SIG == 2


# ------------------------------------------------------------------- the plan ----
def py_chunk_end(mode, o, pk, k, c0, C):
    rb = (lambda j: j) if mode == 0 else (lambda j: o[j])
    kb = (lambda j: pk[j] if pk else j) if mode == 0 else rb
    c1 = c0
    while c1 < k:
        if c1 > c0 and (rb(c1 + 1) - rb(c0) > C or kb(c1 + 1) - kb(c0) > C or c1 - c0 >= C):
            break
        c1 += 1
    return c1


def py_plan(mode, o, pk, c0, c1):
    rb = (lambda j: j) if mode == 0 else (lambda j: o[j])
    ent, po = [], []
    for j in range(c0, c1):
        po.append(len(ent))
        ent += [(j - c0, r - rb(c0)) for r in range(rb(j), rb(j + 1))] + [(j - c0, ROW_SIG)]
    po.append(len(ent))
    kb = (lambda j: pk[j] if pk else j) if mode == 0 else rb
    sb = rb if mode == 2 else (lambda j: j)
    return dict(rows=rb(c1) - rb(c0), keys=kb(c1) - kb(c0), sigs=sb(c1) - sb(c0), ent=ent, pair_off=po,
                key_off=[pk[j] - pk[c0] for j in range(c0, c1 + 1)] if mode == 0 and pk else [],
                sig_off=[o[j] - o[c0] for j in range(c0, c1 + 1)] if mode == 2 else [])


def py_status(mode, o, pk, j, scode, kcode, late, one):
    """scode / kcode indexed from signature 0 / key 0 of the call"""
    step = lambda c, key: (6 if key else 0) if c == 0x80 else c  # noqa: E731
    if mode == 0:
        ks = range(pk[j], pk[j + 1]) if pk else [j]
        seq = [(scode[j], False)] + [(kcode[t], True) for t in ks]
        rows = 1
    elif mode == 1:
        ts = range(o[j], o[j + 1])
        seq = ([(scode[j], False)] if len(ts) else []) + [(kcode[t], True) for t in ts]
        rows = len(ts)
    else:
        ts = range(o[j], o[j + 1])
        seq = [x for t in ts for x in ((scode[t], False), (kcode[t], True))]
        rows = len(ts)
    if rows == 0:
        return 5
    for c, key in seq:
        if step(c, key):
            return step(c, key)
    if late[j]:
        return 6
    return 0 if one[j] else 5


def layouts():
    rnd = random.Random(0x516)
    out = []
    for scheme in (1,):
        out.append((1, si.aggregate(scheme)["o"], None))
        out.append((2, si.batch(scheme, "w64")["o"], None))
        out.append((0, None, si.key_sets(scheme)["pk_off"]))
    out.append((0, None, None))
    for _ in range(12):
        k = rnd.randrange(1, 24)
        o = [rnd.randrange(0, 3)]
        for _ in range(k):
            o.append(o[-1] + rnd.choice([0, 0, 1, 1, 2, 3, 5, 17, 33]))
        out.append((rnd.choice([1, 2]), o, None))
        out.append((0, None, o))
    return out


@pytest.mark.parametrize("chunk", [1, 16, 1 << 20])
def test_plan_against_restatement(m, chunk):
    rnd = random.Random(chunk)
    for mode, o, pk in layouts():
        k = len(o) - 1 if o else (len(pk) - 1 if pk else 9)
        nsig = k if mode != 2 else o[-1]
        nkey = (pk[-1] if pk else k) if mode == 0 else o[-1]
        scode = [rnd.choice([0, 0, 0, 0, 0, 3, 0x80, 1, 2]) for _ in range(nsig)]
        kcode = [rnd.choice([0, 0, 0, 0, 0, 0, 3, 0x80, 1, 2]) for _ in range(nkey)]
        late = [rnd.choice([0, 0, 0, 1]) if mode == 0 else 0 for _ in range(k)]
        one = [rnd.choice([0, 1]) for _ in range(k)]
        c0, seen = 0, 0
        while c0 < k:
            got = m.sigs_plan(mode, o, pk, k, c0, chunk)
            c1 = py_chunk_end(mode, o, pk, k, c0, chunk)
            assert got.pop("c1") == c1 and c1 > c0, (mode, o, pk, c0)
            want = py_plan(mode, o, pk, c0, c1)
            assert got == want, (mode, o, pk, c0)
            # the chunk rule: whole checks, at most `chunk` tuples unless the chunk is one check
            assert want["rows"] <= chunk or c1 == c0 + 1
            rb = (lambda j: j) if mode == 0 else (lambda j: o[j])
            kb = (lambda j: pk[j] if pk else j) if mode == 0 else rb
            sb = rb if mode == 2 else (lambda j: j)
            st = m.sigs_reduce(mode, o, pk, c0, c1, scode[sb(c0):sb(c1)], kcode[kb(c0):kb(c1)],
                               late[c0:c1] if mode == 0 else None, one[c0:c1])
            assert list(st) == [py_status(mode, o, pk, j, scode, kcode, late, one) for j in range(c0, c1)], (mode, o, pk, c0)
            seen += c1 - c0
            c0 = c1
        assert seen == k


def test_reduction_order(m):
    """the signature's code before the key's, tuple by tuple; infinity a skip for a signature
    and 6 for a key; no tuples 5; the late 6 only where nothing failed before"""
    R = m.sigs_reduce
    assert R(0, None, None, 0, 4, [3, 0x80, 0, 0], [0x80, 0x80, 3, 0], [0, 0, 0, 1], [1, 1, 1, 1]) == bytes([3, 6, 3, 6])
    assert R(0, None, [0, 0, 2], 0, 2, [0, 0], [0, 0], [1, 0], [0, 1]) == bytes([6, 0])
    assert R(1, [0, 0, 3], None, 0, 2, [3, 0], [0, 2, 0x80], None, [1, 1]) == bytes([5, 2])
    assert R(1, [0, 2], None, 0, 1, [0x80], [0, 0], None, [0]) == bytes([5])
    assert R(2, [0, 3], None, 0, 1, [0, 0, 3], [0, 0x80, 0], None, [1]) == bytes([6])
    assert R(2, [0, 3], None, 0, 1, [0, 3, 0], [0x80, 0, 0], None, [1]) == bytes([6])
    assert R(2, [0, 2], None, 0, 1, [0, 1], [0, 0x80], None, [1]) == bytes([1])
    assert R(2, [0, 2, 2], None, 0, 2, [0, 0x80], [0, 0], None, [1, 1]) == bytes([0, 5])


PLAN_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "sig_plan.hpp"
using namespace msm;
int main() {
  unsigned long long s = 0x9e3779b97f4a7c15ull, total = 0;
  auto rnd = [&](unsigned m) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)((s >> 33) % m); };
  const size_t lens[] = {0, 0, 1, 1, 2, 5, 17, 33};
  for (int it = 0; it < 300; ++it) {
    const int mode = (int)rnd(3);
    const size_t k = 1 + rnd(20), C = it % 3 == 0 ? 1 : it % 3 == 1 ? 16 : (size_t)1 << 20;
    std::vector<size_t> o(1, rnd(3));
    for (size_t j = 0; j < k; ++j) o.push_back(o.back() + lens[rnd(8)]);
    const bool sets = mode == SIG_VERIFY && rnd(2);
    const size_t *po = mode == SIG_VERIFY ? nullptr : o.data(), *pk = sets ? o.data() : nullptr;
    std::vector<uint8_t> sc(o.back() + k + 1), kc(o.back() + k + 1);
    for (auto &c : sc) c = (uint8_t)(rnd(6) == 0 ? (rnd(2) ? SIG_INF : 3) : 0);
    for (auto &c : kc) c = (uint8_t)(rnd(6) == 0 ? (rnd(2) ? SIG_INF : 1 + rnd(3)) : 0);
    SigChunkPlan pl;
    size_t seen = 0;
    for (size_t c0 = 0; c0 < k;) {
      const size_t c1 = sig_chunk_end(mode, po, pk, k, c0, C);
      if (c1 <= c0 || c1 > k) return 1;
      sig_plan_chunk(pl, mode, po, pk, c0, c1);
      if (pl.pair_off.size() != c1 - c0 + 1 || pl.pair_off.back() != pl.ent.size()) return 2;
      if (pl.ent.size() != pl.nrows + (c1 - c0)) return 3;
      if (pl.nrows > C && c1 != c0 + 1) return 4;
      for (const SigEntry &e : pl.ent)
        if (e.check >= c1 - c0 || (e.src != SIG_ROW_SIG && e.src >= pl.nrows)) return 5;
      // the codes of the chunk, exactly as many as the plan says (the sanitizer sees any read past them)
      std::vector<uint8_t> s2(sc.begin() + pl.s0, sc.begin() + pl.s0 + pl.nsigs), k2(kc.begin() + pl.k0, kc.begin() + pl.k0 + pl.nkeys);
      std::vector<uint8_t> cc(c1 - c0);
      sig_reduce(pl, mode, po, pk, s2.data(), k2.data(), cc.data());
      for (size_t j = 0; j < c1 - c0; ++j) total += sig_status(cc[j], false, true, pl.pair_off[j + 1] - pl.pair_off[j] - 1);
      seen += c1 - c0;
      c0 = c1;
    }
    if (seen != k) return 6;
  }
  printf("ok %llu\n", total);
  return 0;
}
"""


def test_plan_under_sanitizers(tmp_path):
    """csrc/sig_plan.hpp in a stand-alone host program built with ASan + UBSan: seeded layouts
    with empty, short and long checks, cut at chunk sizes 1, 16 and larger than the input"""
    if not shutil.which("g++"):
        pytest.fail("g++ missing")
    src = tmp_path / "sig_plan_main.cpp"
    src.write_text(PLAN_MAIN)
    exe = tmp_path / "sig_plan_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "msm_blst_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and not r.stderr
