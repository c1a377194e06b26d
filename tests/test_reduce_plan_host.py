"""csrc/reduce_plan.hpp without a GPU: the plan of the weighted bucket reduction
(WeightedReducer) and the steps of a reduction, walked over integers mod 2^61 - 1
in a stand-alone host program built with ASan + UBSan.  Every buffer is a vector of
exactly the planned size, so a stride or sizing slip is an overrun the sanitizer
sees; every MSM's window sums must equal the direct sum of w_i S_i; the index
tables are checked for structure and pinned by hash (tests/golden/reduce_plan.json)
to the tables the reducer built before the plan became a header of its own.  The
weights include the real CHES bucket sets (csrc/ches_setup.hpp) and the plain
engine's windows."""
import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <string>
#include "ches_setup.hpp"
#include "reduce_plan.hpp"
using namespace msm;

typedef std::vector<uint32_t> U32s;
static const uint64_t P = ((uint64_t)1 << 61) - 1;
static uint64_t addm(uint64_t a, uint64_t b) { return a + b >= P ? a + b - P : a + b; }  // a, b < P
static uint64_t mulm(uint64_t a, uint64_t b) {  // 2^61 = 1 mod P: fold the product's high bits down twice
  const unsigned __int128 x = (unsigned __int128)a * b;
  const uint64_t r = (uint64_t)(x & P) + (uint64_t)(x >> 61);  // < 2^62 + 2^61 for a, b < P
  return addm(r & P, r >> 61);
}
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

static std::string name;
#define CHECK(c)                                                             \
  do {                                                                       \
    if (!(c)) {                                                              \
      printf("%s: line %d: %s\n", name.c_str(), __LINE__, #c);               \
      exit(1);                                                               \
    }                                                                        \
  } while (0)

struct Fnv {
  uint64_t h = 1469598103934665603ull;
  void u64(uint64_t v) {
    for (int k = 0; k < 8; ++k) h = (h ^ ((v >> (8 * k)) & 255)) * 1099511628211ull;
  }
  void vec(const U32s &v) {
    u64(v.size());
    for (uint32_t x : v)
      for (int k = 0; k < 4; ++k) h = (h ^ ((x >> (8 * k)) & 255)) * 1099511628211ull;
  }
};

// every table and number of the plan
static uint64_t plan_hash(const ReducePlan &p) {
  Fnv f;
  f.u64(p.sbits), f.u64(p.nwin), f.u64(p.c0), f.u64(p.nbuckets);
  f.vec(p.items);
  f.u64(p.l0_off), f.u64(p.perm_off), f.u64(p.bit_off), f.u64(p.bperm_off);
  for (const std::vector<ReduceLevel> *ph : {&p.seg, &p.bit}) {
    f.u64(ph->size());
    for (const ReduceLevel &lv : *ph) f.u64(lv.nout), f.vec(lv.starts);
  }
  f.u64(p.dense_slots()), f.u64(p.bit_slots()), f.u64(p.maxp), f.u64(p.maxp1);
  return f.h;
}

// one phase: level 0 over items [i0, i1) that index `nsrc` sources, pairwise
// levels, the scatter over permutation items [p0, p1)
static void check_phase(const ReducePlan &p, const std::vector<ReduceLevel> &ph, size_t i0, size_t i1, size_t nsrc,
                        size_t p0, size_t p1, size_t nslots) {
  size_t prev = i1 - i0;
  for (size_t l = 0; l < ph.size(); ++l) {
    const ReduceLevel &lv = ph[l];
    const bool last = l + 1 == ph.size();
    CHECK(lv.starts.size() == lv.nout + 1 && lv.starts[0] == 0);
    for (size_t t = 0; t < lv.nout; ++t) CHECK(lv.starts[t] <= lv.starts[t + 1]);
    CHECK(lv.starts.back() == (last ? p1 - p0 : prev));
    if (last) {
      CHECK(lv.nout == nslots);
      for (size_t t = 0; t < lv.nout; ++t) CHECK(lv.starts[t + 1] - lv.starts[t] <= 1);  // a slot: one partial or none
      for (size_t k = p0; k < p1; ++k) CHECK(p.items[k] < prev);
      CHECK(p1 - p0 == prev);  // every final partial lands in a slot
    } else {
      for (size_t t = 0; t < lv.nout; ++t) CHECK(lv.starts[t] < lv.starts[t + 1]);  // no empty partial
    }
    prev = lv.nout;
  }
  for (size_t k = i0; k < i1; ++k) CHECK(p.items[k] < nsrc);
}

static void check_plan(const ReducePlan &p, const U32s &w, const U32s &win) {
  const size_t L = p.seg.size(), S = (size_t)1 << p.sbits;
  CHECK(L >= 2);  // level 0 and the scatter
  CHECK(p.nbuckets == w.size() && p.l0_off == 0 && p.l0_off <= p.perm_off && p.perm_off <= p.bit_off);
  CHECK(p.bit_off <= p.bperm_off && p.bperm_off <= p.items.size());
  CHECK(p.maxp1 <= p.maxp && p.maxp1 >= 1);
  check_phase(p, p.seg, p.l0_off, p.perm_off, w.size(), p.perm_off, p.bit_off, p.dense_slots());
  CHECK(p.has_bit_tail() == (p.nwin == 1));
  if (p.has_bit_tail())
    check_phase(p, p.bit, p.bit_off, p.bperm_off, p.seg[L - 2].nout, p.bperm_off, p.items.size(), p.bit_slots());
  else
    CHECK(p.bit_off == p.items.size());
  // the dense slot of every level-0 item: down the levels, then through the scatter
  const ReduceLevel &sc = p.seg[L - 1];
  U32s slot_of(p.seg[L - 2].nout, ~0u);
  for (size_t sl = 0; sl < sc.nout; ++sl)
    for (size_t k = sc.starts[sl]; k < sc.starts[sl + 1]; ++k) slot_of[p.items[p.perm_off + k]] = (uint32_t)sl;
  U32s at(p.perm_off - p.l0_off);
  for (size_t k = 0; k < at.size(); ++k) at[k] = (uint32_t)k;
  for (size_t l = 0; l + 1 < L; ++l) {  // item -> its partial of level l
    U32s out_of(p.seg[l].starts.back());
    for (size_t t = 0; t < p.seg[l].nout; ++t)
      for (size_t k = p.seg[l].starts[t]; k < p.seg[l].starts[t + 1]; ++k) out_of[k] = (uint32_t)t;
    for (uint32_t &a : at) a = out_of[a];
  }
  // weight 0 never read; once in the low list iff the low half is non-zero, once in the high list iff the high is
  std::vector<uint8_t> lo(w.size(), 0), hi(w.size(), 0);
  for (size_t k = 0; k < at.size(); ++k) {
    const uint32_t i = p.items[p.l0_off + k], sl = slot_of[at[k]];
    CHECK(sl != ~0u);
    const size_t blk = sl / S, val = sl % S + 1;
    CHECK(blk / 2 == (win.empty() ? 0 : win[i]));
    CHECK(val == (blk & 1 ? w[i] >> p.sbits : w[i] & (S - 1)));
    ++(blk & 1 ? hi : lo)[i];
  }
  for (size_t i = 0; i < w.size(); ++i) {
    CHECK(lo[i] == ((w[i] & (S - 1)) != 0));
    CHECK(hi[i] == ((w[i] >> p.sbits) != 0));
  }
}

// the plan's own steps over integers, every buffer exactly the planned size
static void simulate(const ReducePlan &p, const U32s &w, const U32s &win, ReduceEnding end, size_t nmsm) {
  std::vector<uint64_t> bufs[4];
  for (int b = 0; b < 4; ++b) bufs[b] = std::vector<uint64_t>(p.elems((ReduceBuf)b, nmsm), P);  // P: not a residue
  for (uint64_t &x : bufs[kRedBuckets]) x = rnd() % P;
  const std::vector<ReduceStep> steps = p.steps(end);
  CHECK(!steps.empty() && steps[0].src == kRedBuckets && steps[0].sstride == w.size() && steps[0].items == p.l0_off);
  CHECK(steps.back().dst == kRedDense);
  for (size_t k = 0; k < steps.size(); ++k) {
    const ReduceStep &st = steps[k];
    const ReduceLevel &lv = p.level(st.level);
    CHECK(st.src != st.dst);
    if (k) CHECK(st.src == steps[k - 1].dst && st.sstride == steps[k - 1].dstride);
    CHECK((st.dst == kRedDense) == (k + 1 == steps.size()) && st.dst != kRedBuckets);
    CHECK(st.dstride >= lv.nout && nmsm * st.dstride <= bufs[st.dst].size());
    CHECK(nmsm * st.sstride <= bufs[st.src].size());
    const uint64_t *src = bufs[st.src].data();
    uint64_t *dst = bufs[st.dst].data();
    const uint32_t *ix = st.items == kNoItems ? nullptr : p.items.data() + st.items;
    for (size_t m = 0; m < nmsm; ++m)
      for (size_t t = 0; t < lv.nout; ++t) {
        uint64_t a = 0;
        for (size_t q = lv.starts[t]; q < lv.starts[t + 1]; ++q) {
          const uint64_t x = src[m * st.sstride + (ix ? ix[q] : q)];
          CHECK(x < P);  // written by an earlier step
          a = addm(a, x);
        }
        dst[m * st.dstride + t] = a;
      }
  }
  const size_t S = (size_t)1 << p.sbits, s = p.sbits;
  const std::vector<uint64_t> &D = bufs[kRedDense];
  for (size_t m = 0; m < nmsm; ++m) {
    std::vector<uint64_t> got(p.nwin, 0), want(p.nwin, 0);
    if (end == kEndDense) {  // per block sum_b (b + 1) A_b, then low + 2^s high
      for (size_t blk = 0; blk < (size_t)2 * p.nwin; ++blk) {
        uint64_t T = 0;
        for (size_t b = 0; b < S; ++b) T = addm(T, mulm(b + 1, D[m * p.dense_slots() + blk * S + b]));
        got[blk / 2] = addm(got[blk / 2], blk & 1 ? mulm((uint64_t)1 << s, T) : T);
      }
    } else {  // sum_j 2^j B_j: the low half's s bit sums, then the high half's
      for (size_t j = 0; j < 2 * s; ++j) got[0] = addm(got[0], mulm((uint64_t)1 << j, D[m * p.bit_slots() + j]));
    }
    for (size_t i = 0; i < w.size(); ++i) {
      uint64_t &t = want[win.empty() ? 0 : win[i]];
      t = addm(t, mulm(w[i], bufs[kRedBuckets][m * w.size() + i]));
    }
    CHECK(got == want);
  }
}

static size_t ncases = 0;
static void run(const std::string &nm, const U32s &w, const U32s &win, int nwin, int c0, int lane_factor = 1,
                int want_c0 = 0) {
  name = nm;
  const ReducePlan p = ReducePlan::build(w, win, nwin, c0, lane_factor);
  CHECK(p.c0 == (want_c0 ? want_c0 : c0 ? c0 : p.c0));
  check_plan(p, w, win);
  for (size_t nmsm : {1, 2, 3, 20}) {
    simulate(p, w, win, kEndDense, nmsm);
    if (p.has_bit_tail()) simulate(p, w, win, kEndBits, nmsm);
  }
  printf("H %s %016llx\n", nm.c_str(), (unsigned long long)plan_hash(p));
  ++ncases;
}

int main(int argc, char **argv) {
  const std::string S = " ";
  auto num = [](long v) { return std::to_string(v); };
  // dense 1..N
  for (int N : {0, 1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000})
    for (int c0 : {0, 2, 3, 8, 64}) {
      U32s w(N);
      for (int i = 0; i < N; ++i) w[i] = i + 1;
      run("dense" + S + num(N) + S + num(c0), w, {}, 1, c0);
    }
  // small lists
  const std::vector<U32s> lists = {{0},       {0, 0, 0},    U32s{1},      {1, 1, 1, 1, 1},       U32s{4}, {4, 4, 8, 12},
                                   {3, 3, 3}, {16, 32, 48}, U32s(20, 5u), U32s{(uint32_t)1 << 23}, {(1u << 24) - 1, 1}};
  for (size_t k = 0; k < lists.size(); ++k) run("list" + S + num(k), lists[k], {}, 1, 0);
  // the plain engine's windows (Pippenger::plan_reduction): bucket (w, b - 1) has
  // weight b in window w; top window: slot k holds a copy of bucket (k mod ntop) + 1
  const int pip[][3] = {{2, 3, 0}, {3, 4, 1}, {5, 3, 2}, {8, 2, 0}, {10, 3, 3}};
  for (const int *c : pip)
    for (int c0 : {0, 8}) {
      const size_t NB = (size_t)1 << (c[0] - 1), W = c[1], NT = W * NB, ntop = NB >> c[2];
      U32s wt(NT), win(NT);
      for (size_t k = 0; k < NT; ++k) {
        const size_t ww = k / NB, b = k % NB;
        wt[k] = (uint32_t)((ww == W - 1 ? b % ntop : b) + 1);
        win[k] = (uint32_t)ww;
      }
      run("pip" + S + num(c[0]) + S + num(c[1]) + S + num(c[2]) + S + num(c0), wt, win, (int)W, c0);
    }
  // the CHES bucket sets with their top copies (Ches::plan_buckets); argv: n_exp:b_size of the golden parameters
  for (int n_exp : {8, 10, 16, 20})
    for (int copies : {1, 3}) {
      name = "ches" + S + num(n_exp) + S + num(copies);
      ChesParams cp;
      CHECK(ches_params_for(n_exp, 0, &cp));
      const std::vector<int> B = ches_bucket_set(1 << cp.q_exp, cp.a_h);
      CHECK((int)B.size() == cp.b_size);
      for (int a = 1; a < argc; ++a) {
        int ne = 0, bs = 0;
        CHECK(sscanf(argv[a], "%d:%d", &ne, &bs) == 2);
        if (ne == n_exp) CHECK((int)B.size() == bs);
      }
      int small = 0;
      for (size_t k = 1; k < B.size() && B[k] <= cp.a_h + 1; ++k) small = (int)k;
      U32s w(B.begin(), B.end());
      for (int c = 1; c < copies; ++c)
        for (int k = 1; k <= small; ++k) w.push_back((uint32_t)B[k]);
      run(name, w, {}, 1, 0);
    }
  // random sparse vectors with zeros, one to four windows, weights up to 2^20
  for (int t = 0; t < 64; ++t) {
    const size_t n = 1 + rnd() % 400;
    const uint32_t maxes[] = {1, 3, 16, 255, 256, 4097, 1u << 20};
    const uint32_t mx = maxes[rnd() % 7];
    const int nwin = 1 + t % 4, c0s[] = {0, 2, 5, 8};
    U32s w(n), win;
    for (uint32_t &x : w) x = rnd() & 1 ? (uint32_t)(rnd() % ((uint64_t)mx + 1)) : 0;
    if (nwin > 1 || (t & 4))
      for (size_t i = 0; i < n; ++i) win.push_back((uint32_t)(rnd() % nwin));
    run("rand" + S + num(t), w, win, nwin, c0s[rnd() % 4]);
  }
  // the chunk rule at its edges: 2 below 600 K lane items, 4 below 1.5 M, else 8; G2 counts two lanes per item.
  // Buckets of weight 3 (s = 1: one low and one high item each) and, for an odd count, one of weight 1
  for (int lf : {1, 2})
    for (size_t thr : {(size_t)600 << 10, (size_t)3 << 19})
      for (int d : {-1, 0, 1}) {
        const size_t items = thr + d, lane_items = items * lf;
        U32s w(items / 2, 3u);
        if (items & 1) w.push_back(1);
        const int want = lane_items >= ((size_t)3 << 19) ? 8 : lane_items >= ((size_t)600 << 10) ? 4 : 2;
        run("chunk" + S + num(lf) + S + num((long)thr) + S + num(d), w, {}, 1, 0, lf, want);
      }
  printf("ok %zu\n", ncases);
  return 0;
}
"""


@pytest.fixture(scope="module")
def plan_run(tmp_path_factory):
    """the program's output: built and run once"""
    if not shutil.which("g++"):
        pytest.fail("g++ missing")
    d = tmp_path_factory.mktemp("reduce_plan")
    src = d / "reduce_plan_main.cpp"
    src.write_text(MAIN)
    exe = d / "reduce_plan_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "msm_blst_amd", "csrc"), str(src),
                    "-o", str(exe)], check=True)
    sizes = []
    for n_exp in (10, 16, 20):
        with open(os.path.join(GOLDEN, f"ches_params_n{n_exp}.json")) as f:
            sizes.append(f"{n_exp}:{json.load(f)['b_size']}")
    r = subprocess.run([str(exe)] + sizes, capture_output=True, text=True, timeout=300)
    return r


def test_steps_under_sanitizers(plan_run):
    """dense 1..N, small lists, the plain engine's windows, the real CHES bucket sets with
    top copies, random sparse vectors and the chunk rule's edges; 1, 2, 3 and 20 MSMs, both
    endings: every step stays inside buffers of exactly the planned size, reads only what
    an earlier step wrote, and every MSM's window sums equal sum w_i S_i; the tables are
    well-formed and read every bucket once per non-zero half of its weight"""
    assert plan_run.returncode == 0, plan_run.stdout[-2000:] + plan_run.stderr[-4000:]
    assert not plan_run.stderr
    last = plan_run.stdout.splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) == 90 + 11 + 10 + 8 + 64 + 12


def test_tables_equal_the_pinned_hashes(plan_run):
    """FNV-1a of every table and number of each case's plan, recorded from the plan code as
    the reducer had it (chunking and permutation still written per phase)"""
    assert plan_run.returncode == 0, plan_run.stdout[-2000:] + plan_run.stderr[-4000:]
    got = {}
    for ln in plan_run.stdout.splitlines():
        if ln.startswith("H "):
            got[ln[2:-17]] = ln[-16:]
    with open(os.path.join(GOLDEN, "reduce_plan.json")) as f:
        want = json.load(f)["hashes"]
    assert got == want
