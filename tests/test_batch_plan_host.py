"""csrc/batch_plan.hpp without a GPU: the plan of an MSM batch and its three issue
schedules (Ches::run_jobs, Pippenger::run_batch), driven by a recording sink in a
stand-alone host program built with ASan + UBSan.  Streams are FIFO queues, events
carry vector clocks, host waits order what the host issues after them; every ring
rule is then a happens-before check in plain integers."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAIN = r"""
#include <array>
#include <cstdio>
#include <cstring>
#include <set>
#include "batch_plan.hpp"
using namespace msm;

typedef std::array<int, kBatchStreams> Clk;
static Clk join(Clk a, const Clk &b) {
  for (int i = 0; i < kBatchStreams; ++i) a[i] = std::max(a[i], b[i]);
  return a;
}
struct Op {
  int stream = 0, seq = 0;
  Clk clk{};
};
static bool hb(const Op &a, const Clk &c) { return c[a.stream] >= a.seq; }  // a happens before a point with clock c

enum Kind { SCAL, FRONT, BUCKET, GBUCKET, RED, OUT };
struct Res {
  bool written = false;
  long tag = -1;
  Op w;
  std::vector<Op> reads;
};

struct Rec {
  const BatchPlan &p;
  bool ches;
  Clk sc[kBatchStreams]{}, host{};
  std::vector<Clk> ev;    // events' clocks
  std::vector<int> nrec;  // times recorded in this call
  size_t seen_max = 0;    // the largest event index named
  std::vector<Res> res[6];  // by Kind: slot group x 8 + set, front set, bucket set, lane x 8 + set, reducer set x 32 + slot, MSM
  std::vector<int> nacc, nl0, ntail, nfront, ncopy;
  long last_tail_end = -1;
  int nlast = 0, fail = 0;
  Rec(const BatchPlan &plan, bool c)
      : p(plan), ches(c), ev(plan.events + 2), nrec(plan.events + 2), nacc(plan.count), nl0(plan.count),
        ntail(plan.count), nfront(plan.nfg), ncopy(plan.count) {
    const size_t sizes[6] = {(plan.nsg + 1) * 8, (size_t)plan.nfr, 3, 16, (size_t)plan.nred * 32, plan.count};
    for (int k = 0; k < 6; ++k) res[k].resize(sizes[k]);
  }
  bool names(size_t e) {  // 5. (an index past the events asked for)
    seen_max = std::max(seen_max, e);
    if (e >= ev.size()) bad(65);
    return e < ev.size();
  }
  void bad(int code) {
    if (!fail) fail = code;
  }
  Op enq(int s) {
    sc[s] = join(sc[s], host);
    Op o;
    o.stream = s, o.seq = ++sc[s][s], o.clk = sc[s];
    return o;
  }
  // 3. a write comes after the earlier write and every read of it; a read after the write it means
  void write(Kind k, long i, long tag, const Op &o) {
    Res &r = res[k].at(i);
    if (r.written && !hb(r.w, o.clk)) bad(30);
    for (const Op &rd : r.reads)
      if (!hb(rd, o.clk)) bad(31 + k);
    r.written = true, r.tag = tag, r.w = o, r.reads.clear();
  }
  void read(Kind k, long i, long tag, const Op &o) {
    Res &r = res[k].at(i);
    if (!r.written || r.tag != tag) return bad(40 + k);
    if (!hb(r.w, o.clk)) bad(50 + k);
    r.reads.push_back(o);
  }
  long tag(Kind k, long i) { return res[k].at(i).written ? res[k].at(i).tag : -1; }

  // 2. every wait names an event recorded earlier in this call
  void wait(int s, size_t e) {
    if (!names(e)) return;
    if (!nrec[e]) return bad(20);
    sc[s] = join(join(sc[s], host), ev[e]);
  }
  void record(size_t e, int s) {
    if (!names(e)) return;
    sc[s] = join(sc[s], host);
    ev[e] = sc[s];
    ++nrec[e];
  }
  void host_wait(size_t e) {
    if (!names(e)) return;
    if (!nrec[e]) return bad(21);
    host = join(host, ev[e]);
  }
  void sync(int s) { host = join(host, sc[s]); }
  void copy_set(size_t g, size_t k) {
    if (!p.host || k < p.fgb[g] || k >= p.fgb[g + 1]) return bad(10);
    ++ncopy[k];
    write(SCAL, (long)((g % p.nsg) * 8 + (k - p.fgb[g])), (long)k, enq(kCopy));
  }
  void front(size_t g) {
    const Op o = enq(kFront);
    ++nfront[g];
    for (size_t k = p.fgb[g]; p.host && k < p.fgb[g + 1]; ++k)
      read(SCAL, (long)((g % p.nsg) * 8 + (k - p.fgb[g])), (long)k, o);
    write(FRONT, (long)(g % p.nfr), (long)g, o);
  }
  void accumulate(int s, size_t g, size_t k, int bset) {
    if (k < p.fgb[g] || k >= p.fgb[g + 1] || p.sched == kAccGroups) return bad(11);
    const Op o = enq(s);
    read(FRONT, (long)(g % p.nfr), (long)g, o);
    write(BUCKET, bset, (long)k, o);
    ++nacc[k];
  }
  void accumulate_group(int s, size_t g, int gb) {
    if (p.sched != kAccGroups) return bad(12);
    const Op o = enq(s);
    read(FRONT, (long)(g % p.nfr), (long)g, o);
    for (size_t k = p.fgb[g]; k < p.fgb[g + 1]; ++k) {
      write(GBUCKET, gb * 8 + (long)(k - p.fgb[g]), (long)k, o);
      ++nacc[k];
    }
  }
  void l0_of(Kind kind, long at, int rset, int slot, const Op &o) {
    const long k = tag(kind, at);  // the MSM whose buckets are there
    if (k < 0 || (int)(p.rg.of(k) % p.nred) != rset || (int)p.rg.slot(k) != slot) return bad(13);
    read(kind, at, k, o);
    write(RED, rset * 32 + slot, k, o);
    ++nl0[k];
  }
  void level0(int s, int bset, int rset, int slot) { l0_of(BUCKET, bset, rset, slot, enq(s)); }
  void level0_group(int s, int gb, size_t off, int rset, int slot0, int m) {
    const Op o = enq(s);
    for (int j = 0; j < m; ++j) l0_of(GBUCKET, gb * 8 + (long)off + j, rset, slot0 + j, o);
  }
  void tail(int s, int rset, size_t first, size_t m, bool last) {
    const Op o = enq(s);
    const size_t q = p.rg.of(first);
    if (first != p.rg.first(q) || first + m != p.rg.first(q + 1) || (int)(q % p.nred) != rset) return bad(14);
    for (size_t j = 0; j < m; ++j) {
      read(RED, rset * 32 + (long)j, (long)(first + j), o);
      write(OUT, (long)(first + j), (long)(first + j), o);
      ++ntail[first + j];
    }
    if (last) ++nlast, last_tail_end = (long)(first + m);
    if (last != (first + m == p.count)) bad(15);
  }
  void combine(size_t first, size_t m) {  // on the host
    if (ches) return bad(16);
    for (size_t k = first; k < first + m; ++k) {
      Res &r = res[OUT].at(k);
      if (!r.written || !hb(r.w, host)) bad(17);
    }
  }
  void prof_begin(int s, size_t) { enq(s); }
  void prof_end(int s, size_t) { enq(s); }
};

static int check(const BatchPlan &p, bool ches) {
  // 1. the groups tile [0, count)
  if (p.fgb.empty() || p.fgb[0] != 0 || p.fgb.back() != p.count || p.nfg + 1 != p.fgb.size()) return 1;
  for (size_t g = 0; g < p.nfg; ++g)
    if (p.fgb[g + 1] <= p.fgb[g] || p.fgb[g + 1] - p.fgb[g] > p.fg_max) return 2;
  const size_t ng = p.rg.groups();
  if (ng != (p.count + p.group_max - 1) / p.group_max || p.rg.first(0) != 0 || p.rg.first(ng) != p.count) return 3;
  for (size_t q = 0; q < ng; ++q) {
    const size_t a = p.rg.first(q), b = p.rg.first(q + 1);
    if (b <= a || b - a > p.group_max) return 4;
    for (size_t k = a; k < b; ++k)
      if (p.rg.of(k) != q || p.rg.slot(k) != k - a || p.rg.ends(k) != (k + 1 == b)) return 5;
  }
  if (ches && (p.nsg + 1 < (size_t)p.nfr || p.nsg > p.slot_groups)) return 6;
  // 5. the event layout: every role its own index, all below the count asked for
  std::set<size_t> idx{p.ev_start()};
  size_t roles = 1;
  for (size_t k = 0; k < p.count; ++k) idx.insert(p.ev_acc(k)), idx.insert(p.ev_l0(k)), roles += 2;
  for (size_t g = 0; g < p.nfg; ++g) {
    idx.insert(p.ev_front(g)), ++roles;
    if (ches) idx.insert(p.ev_copy(g)), ++roles;
  }
  for (size_t q = 0; q < ng; ++q) idx.insert(p.ev_tail(q)), ++roles;
  if (idx.size() != roles || *idx.rbegin() >= p.events) return 7;
  // the join: CHES its own two events past the plan's, the plain engine the start event again
  for (int i = 0; i < 3; ++i)
    if (ches ? (p.join_ev[i] < p.events || p.join_ev[i] > p.events + 1) : p.join_ev[i] != p.ev_start()) return 8;

  Rec r(p, ches);
  BatchIssue<Rec>(p, r).run();
  if (r.fail) return r.fail;
  for (size_t k = 0; k < p.count; ++k)
    if (r.nacc[k] != 1 || r.nl0[k] != 1 || r.ntail[k] != 1 || r.ncopy[k] != (p.host ? 1 : 0)) return 60;
  for (size_t g = 0; g < p.nfg; ++g)
    if (r.nfront[g] != 1) return 61;
  if (r.nlast != 1 || r.last_tail_end != (long)p.count) return 62;
  // 4. after the join the caller's stream is ordered after every operation of the batch
  for (int s = 0; s < kBatchStreams; ++s)
    if (r.sc[kCaller][s] < r.sc[s][s]) return 63;
  // CHES combines on the host after the join: every read-back has landed
  for (size_t k = 0; ches && k < p.count; ++k)
    if (!hb(r.res[OUT].at(k).w, r.host)) return 64;
  if (r.seen_max >= p.events + (ches ? 2 : 0)) return 65;
  for (size_t e = 0; e < r.nrec.size(); ++e)  // one record per event and call, but for the join's
    if (r.nrec[e] > 1 && e != p.join_ev[0] && e != p.join_ev[2]) return 66;
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && !strcmp(argv[1], "knobs")) {
    const BatchKnobs &k = BatchKnobs::env();
    printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", k.tail_coop, k.red_group, k.pip_group, k.bit_tail,
           k.front_group, k.pip_front_group, k.acc_group, k.h2d_slots, k.copy_pace, k.acc_after_l0, k.batch_lanes,
           k.fine_bt, k.pip_fine_bt, k.batch_l0_chunk, k.pip_l0_chunk);
    return 0;
  }
  size_t cases = 0;
  const int fgs[] = {1, 2, 4, 8}, gms[] = {1, 2, 8, 20}, sgs[] = {2, 4, 0};
  for (int fg : fgs)
    for (int gm : gms) {
      BatchKnobs kn;
      kn.front_group = kn.pip_front_group = fg, kn.red_group = kn.pip_group = gm;
      for (size_t count = 1; count <= 70; ++count) {  // the plain engine
        const BatchPlan p = BatchPlan::plain(count, kn);
        if (int rc = check(p, false)) return printf("plain fg %d gm %d count %zu: %d\n", fg, gm, count, rc), 1;
        ++cases;
      }
      for (int lanes = 1; lanes <= 3; ++lanes)
        for (int accg = 0; accg <= (lanes > 1); ++accg)
          for (int host = 0; host <= 1; ++host)
            for (int pace = 0; pace <= (host ? 8 : 0); pace += 8)
              for (int sg : sgs)
                for (size_t nseg = 1; nseg <= 2; ++nseg)
                  for (size_t nsets = 1; nsets * nseg <= 70; ++nsets) {
                    kn.acc_group = accg, kn.copy_pace = pace, kn.h2d_slots = sg;
                    BatchShape z;
                    z.nsets = nsets, z.nseg = nseg, z.n = 4096, z.stride = 32, z.set_stride = nseg * z.n * z.stride;
                    z.h = 3, z.buckets = 1000, z.lanes = lanes, z.group = 1, z.host = host, z.bit_tail_ok = true;
                    z.bucket_bytes = 192, z.out_bytes = 288, z.bit_bytes = 144 * 20;
                    const BatchPlan p = BatchPlan::ches(z, kn);
                    const BatchSchedule want = lanes == 1 ? kOneLane : accg && nseg == 1 ? kAccGroups : kLanes;
                    int rc = p.sched != want || p.count != nsets * nseg || p.fg_max != (size_t)(want == kAccGroups && gm == 1 ? std::min(fg, 4) : fg) ? 9 : check(p, true);
                    if (p.pace != (size_t)(host ? pace : 0) || p.scal_bytes < (host ? p.nsg * p.fg_max * p.sslot : 0)) rc = 9;
                    if (rc)
                      return printf("ches lanes %d accg %d fg %d gm %d host %d pace %d sg %d nseg %zu nsets %zu: %d\n",
                                    lanes, accg, fg, gm, host, pace, sg, nseg, nsets, rc), 1;
                    ++cases;
                  }
    }
  // sets that are not packed cannot share a front pass
  BatchShape z;
  z.nsets = 5, z.nseg = 2, z.n = 64, z.set_stride = 2 * 64 * 32 + 32, z.lanes = 3;
  BatchKnobs kn;
  kn.front_group = 8;
  if (BatchPlan::ches(z, kn).fg_max != 1 || check(BatchPlan::ches(z, kn), true)) return printf("unpacked\n"), 1;
  printf("ok %zu\n", cases + 1);
  return 0;
}
"""


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ missing")
    d = tmp_path_factory.mktemp("batch_plan")
    src = d / "batch_plan_main.cpp"
    src.write_text(MAIN)
    exe = d / "batch_plan_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "msm_blst_amd", "csrc"), str(src),
                    "-o", str(exe)], check=True)
    return str(exe)


def test_schedules_under_sanitizers(plan_exe):
    """every count from 1 to 70 in the three CHES schedules and the plain engine's, lanes
    1 - 3, front groups 1 - 8, reduction groups 1 - 20, host and device scalars, paced and
    unpaced copies, 2 / 4 / default slot groups, one and two segments: the groups tile
    the batch, every wait names an event recorded earlier in the call, every ring slot
    is written after its earlier reads and read after the write meant (happens-before),
    the join orders the caller's stream after everything, the event roles are disjoint"""
    r = subprocess.run([plan_exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and not r.stderr
    assert int(r.stdout.split()[1]) > 70000


KNOBS = ["MSM_TAIL_COOP", "MSM_RED_GROUP", "MSM_PIP_GROUP", "MSM_BIT_TAIL", "MSM_FRONT_GROUP", "MSM_PIP_FRONT_GROUP",
         "MSM_ACC_GROUP", "MSM_H2D_SLOTS", "MSM_COPY_PACE", "MSM_ACC_AFTER_L0", "MSM_BATCH_LANES", "MSM_FINE_BT",
         "MSM_PIP_FINE_BT", "MSM_BATCH_L0_CHUNK", "MSM_PIP_L0_CHUNK"]


@pytest.mark.parametrize("given,want", [
    ({}, [1, 0, 0, 1, 0, 4, 1, 0, 8, -1, 0, 1024, 1024, 8, 0]),
    ({k: "0" for k in KNOBS}, [0, 1, 1, 0, 1, 1, 0, 2, 0, 0, 1, 1024, 1024, 0, 0]),
    ({k: "256" for k in KNOBS}, [1, 32, 32, 1, 8, 8, 1, 256, 32, 1, 3, 256, 256, 64, 64]),
    ({"MSM_RED_GROUP": "2", "MSM_PIP_GROUP": "3", "MSM_FRONT_GROUP": "8", "MSM_H2D_SLOTS": "4", "MSM_BATCH_LANES": "2",
      "MSM_ACC_AFTER_L0": "1"}, [1, 2, 3, 1, 8, 4, 1, 4, 8, 1, 2, 1024, 1024, 8, 0]),
])
def test_knobs_from_the_environment(plan_exe, given, want):
    """BatchKnobs::env(): the defaults, and each knob's range as the batch functions clamped it"""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(given)
    r = subprocess.run([plan_exe, "knobs"], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert [int(x) for x in r.stdout.split()] == want
