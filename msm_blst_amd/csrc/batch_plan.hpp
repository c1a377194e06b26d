// batch_plan.hpp -- the MSM batch pipelines (Ches::run_jobs, Pippenger::run_batch)
// as a plan in plain integers and three issue schedules written against a sink.
// Plain C++, no HIP: the engines supply a sink that turns every operation into
// the one HIP call or launch it stands for, the CPU tests one that records them
// and checks the ring rules by happens-before (tests/test_batch_plan_host.py).
// DESIGN 29.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

namespace msm {

// Front groups of a batch (MSMs [fgb[g], fgb[g + 1]) share one digits + sort
// pass and, for small MSMs, one accumulation launch): 1, 1, 2, 4, then fg_max
// each.  The first accumulation starts after one front, and each group's host
// sets (copied while the earlier groups accumulate: a set copies in ~0.6 ms, an
// MSM accumulates in ~2.3) are in HBM before its front is due -- a first group
// of eight stalled the H2D batch by ~5 ms (the 256-MiB copy, then the front,
// before MSM 1).
inline std::vector<size_t> front_groups(size_t count, size_t fg_max) {
  std::vector<size_t> fgb{0};
  while (fgb.back() < count)
    fgb.push_back(std::min(count, fgb.back() + std::min<size_t>(fg_max, std::max<size_t>(1, fgb.back()))));
  return fgb;
}

// Reduction groups: ceil(count / group_max) groups of balanced size R, group q
// = MSMs [q R, min(count, (q + 1) R)).  The MSMs of a group share one reducer
// set (each its slot) and one tail.
struct RedGroups {
  size_t count = 0, R = 1;
  RedGroups() = default;
  RedGroups(size_t count_, size_t group_max) : count(count_) {
    const size_t ng = (count + group_max - 1) / group_max;
    R = ng ? (count + ng - 1) / ng : 1;
  }
  size_t groups() const { return (count + R - 1) / R; }
  size_t first(size_t q) const { return std::min(count, q * R); }
  size_t of(size_t k) const { return k / R; }
  size_t slot(size_t k) const { return k % R; }
  bool ends(size_t k) const { return (k + 1) % R == 0 || k + 1 == count; }  // the group's last MSM
};

// The knobs of the two batch functions, read from the environment once per
// process (env()); a test constructs them directly.  0 / -1: not set.
struct BatchKnobs {
  // the dense stage of the batch's LAST group runs its adds over 4 waves each
  // (nothing else left to overlap; MSM_TAIL_COOP=0: one lane per add throughout)
  bool tail_coop = true;
  // MSMs per reduction group, MSM_RED_GROUP (CHES) and MSM_PIP_GROUP (plain),
  // 1..32; default ChesBatch::kGroup and PlainBatch::kGroup
  int red_group = 0, pip_group = 0;
  // The batch's LAST reduction group ends in bit sums (WeightedReducer::tail, kEndBits):
  // its tail runs after the last accumulation with the chip otherwise idle, and
  // the bit phase is ~10 latency-bound levels instead of the dense stage's 2 s
  // (profiles/r06_small_trace.txt).  Earlier groups keep the dense stage: their
  // tails run beside accumulations, where the 2 s-Jacobian read-backs cost
  // (DESIGN 5).  MSM_BIT_TAIL=0: dense stage for every group.
  bool bit_tail = true;
  // front group cap, MSM_FRONT_GROUP=<1..8> (BatchPlan::ches has the defaults)
  // and MSM_PIP_FRONT_GROUP=<1..8>, default 4 (1: one MSM per launch)
  int front_group = 0, pip_front_group = 4;
  // accumulation groups for small MSMs; MSM_ACC_GROUP=0: per-MSM lanes
  bool acc_group = true;
  // MSM_H2D_SLOTS=<2..256>: slot groups of device scalar slots (copies issued
  // that far ahead); default by size, BatchPlan::ches
  int h2d_slots = 0;
  // Paced copies (MSM_COPY_PACE=L, default 8; 0 or < 3: all at the batch
  // start): the first L front groups' sets are copied at the batch start, the
  // copy of group g >= L is issued when the accumulation L MSMs before it has
  // finished (a host wait on its event -- no cross-stream wait on the copy
  // stream), so later copies run one per period beside one MSM instead of back
  // to back beside the first five: 2^20 H2D 436.4 / 439.2 / 439.9 vs 432.4 /
  // 436.2 / 436.7 M pairs/s (L = 8 vs all at the start, tools/h2d_ab.py
  // medians, alternating on one box; profiles/r05_copy_pace_ab.txt).
  int copy_pace = 8;
  // One lane: accumulation k waits for level 0 of MSM k - 1, so level 0 runs
  // beside the fronts, never beside the next accumulation.  Without this wait
  // the batch fell, in about one run in three, into a schedule where fronts ran
  // two MSMs ahead and every accumulation started at once beside the previous
  // level 0: level 0 then took 0.5-1.2 ms instead of 0.41, the accumulations
  // 2.2-2.7 ms instead of 1.8, and the H2D headline 342-386 M pairs/s instead of
  // ~420 (kernel traces, profiles/archive_r01_r04.txt (r03_spread_trace.txt));
  // with it 19 of 19 runs on three boxes gave 410-422 M
  // (profiles/archive_r01_r04.txt (r03_ab_studies.txt) r03a0*).  G2 (5-ms
  // accumulations, 1.2-ms level 0) never showed the slow mode and runs 1.5 %
  // faster free-running (r03a0g2), so the wait is the G1 default;
  // MSM_ACC_AFTER_L0=0 / =1 forces either schedule for both groups.
  int acc_after_l0 = -1;
  int batch_lanes = 0;  // MSM_BATCH_LANES=1|2|3 (default by size, Ches::batch_lanes)
  // the batch fronts' fine-pass workgroup (bucket_sort.hpp k_bs_fine): 1024
  // threads; MSM_FINE_BT=256 (MSM_PIP_FINE_BT for the plain engine) selects the
  // variant that fits beside three accumulation waves per SIMD -- measured
  // slower (H2D 408-411 vs 415-420 M, resident 423-429 vs 434-440 M pairs/s,
  // profiles/archive_r01_r04.txt (r04_fine_bt_ab.txt))
  int fine_bt = 1024, pip_fine_bt = 1024;
  // the batch reducer's level-0 chunk: MSM_BATCH_L0_CHUNK=<2..64>, default 8,
  // 0: the synchronous reducer's (Ches::plan_buckets); MSM_PIP_L0_CHUNK, default 0
  int batch_l0_chunk = 8, pip_l0_chunk = 0;

  static int env_int(const char *name, int unset, int lo, int hi) {
    const char *e = getenv(name);
    return e ? std::max(lo, std::min(hi, atoi(e))) : unset;
  }
  static int env_flag(const char *name, int unset) {
    const char *e = getenv(name);
    return e ? atoi(e) != 0 : unset;
  }
  static int env_bt(const char *name) {
    const char *e = getenv(name);
    return e && atoi(e) == 256 ? 256 : 1024;
  }
  static const BatchKnobs &env() {
    static const BatchKnobs k = [] {
      BatchKnobs b;
      b.tail_coop = env_flag("MSM_TAIL_COOP", 1);
      b.red_group = env_int("MSM_RED_GROUP", 0, 1, 32);
      b.pip_group = env_int("MSM_PIP_GROUP", 0, 1, 32);
      b.bit_tail = env_flag("MSM_BIT_TAIL", 1);
      b.front_group = env_int("MSM_FRONT_GROUP", 0, 1, 8);
      b.pip_front_group = env_int("MSM_PIP_FRONT_GROUP", 4, 1, 8);
      b.acc_group = env_flag("MSM_ACC_GROUP", 1);
      b.h2d_slots = env_int("MSM_H2D_SLOTS", 0, 2, 256);
      b.copy_pace = env_int("MSM_COPY_PACE", 8, 0, 32);
      b.acc_after_l0 = env_flag("MSM_ACC_AFTER_L0", -1);
      b.batch_lanes = env_int("MSM_BATCH_LANES", 0, 1, 3);
      b.fine_bt = env_bt("MSM_FINE_BT");
      b.pip_fine_bt = env_bt("MSM_PIP_FINE_BT");
      b.batch_l0_chunk = env_int("MSM_BATCH_L0_CHUNK", 8, 0, 64);
      b.pip_l0_chunk = env_int("MSM_PIP_L0_CHUNK", 0, 0, 64);
      return b;
    }();
    return k;
  }
};

// the constants of the CHES batch (Ches<G> names them as its own)
struct ChesBatch {
  // MSMs per reduction group.  20: a batch of up to 20 runs one tail, after its
  // last accumulation, instead of tails beside accumulations (each costs the one
  // beside it ~0.3 ms); 20 vs 8 measured +1.2 %
  // (profiles/archive_r01_r04.txt (r04_red_group_ab.txt))
  static constexpr int kGroup = 20;
  static constexpr int kFrontGroup = 8;  // largest front group (ramping up 1, 1, 2, 4, 8)
  static constexpr int kFrontGroupDefault = 1;
  // front k+1 may start when accumulation k-2 ends (slack for the copies); the
  // lane schedules of small MSMs rotate kFrontsMax sets (fronts further ahead)
  static constexpr int kFronts = 3, kFrontsMax = 5;
  // bucket sets of the one-lane schedule: MSM k accumulates into set k % kBSets
  // while the reduction of MSM k-1 still reads the other one
  static constexpr int kBSets = 2;
};
// and of the plain engine's.  kGroup 10 (two tails for the 20-MSM configs[1]
// batch) since the host Horner of a group runs on the worker threads: 0.327-
// 0.339 vs 0.341-0.353 ms per 2^16 MSM with 8 (profiles/r05_pip_group_ab.txt)
struct PlainBatch {
  static constexpr int kFronts = 5, kGroup = 10, kRedSets = 4;
};

// The streams of a batch.  CHES: the caller's, tails_[0], tails_[1], fstream_,
// cstream_; the plain engine: the caller's, lane1_, tstream_, fstream_.
enum BatchStream { kCaller = 0, kLane1 = 1, kLane2 = 2, kFront = 3, kCopy = 4, kBatchStreams = 5 };

// Which issue loop runs (BatchIssue):
//  kAccGroups  small MSMs, one table for every job: front group g's sets
//              accumulate in ONE launch on lane stream g % 2 (kCaller, kLane1),
//              then ONE level-0 launch per reduction group they touch; the
//              group tails run on kLane2.  A small MSM's own grid fills the
//              chip's wave slots about one round deep and its last waves run
//              with the chip half idle; side-by-side lanes left the
//              accumulations at ~0.55 of the madd rate (2^17: 0.65 ms each, 1.5
//              running at a time; profiles/r05_small_trace.txt).  The plain
//              engine's only schedule.
//  kLanes      per-MSM lanes (MSM_ACC_GROUP=0, or several segments): MSM k
//              accumulates into bucket set k % lanes on stream k % lanes and its
//              level 0 follows on the same stream; the group tails run on
//              kLane2, with three lanes on kFront (the process has 4 hardware
//              queues by default: one stream per queue).
//  kOneLane    the 2^20 headline: accumulations back to back on kCaller, the
//              VALU-bound critical path; level 0 and the tails of reduction
//              group q on kLane1 + q % 2, so group q + 1's level 0s never queue
//              behind group q's tail.  One accumulation launch per MSM: alone,
//              two 2^20 sets in one grid accumulate in 1.70 ms per set vs 1.96
//              for one (profiles/r05_acc_rate.txt), but in the batch the front
//              and level 0 beside it fill that tail: groups of 2 per launch
//              measured 427 vs 431-433 M pairs/s with H2D
//              (profiles/r05_head_front_group_ab.txt).
enum BatchSchedule { kAccGroups, kLanes, kOneLane };

// what BatchPlan::ches is computed from
struct BatchShape {
  size_t nsets = 0, nseg = 1;        // jobs k = set (k / nseg), segment (k % nseg)
  size_t n = 0, stride = 32, set_stride = 0;
  int h = 1;                         // digits per scalar (front set sizing)
  size_t buckets = 0;                // per MSM
  int lanes = 1, group = 1;          // Ches::batch_lanes(), G
  bool host = false, dev_out = false, bit_tail_ok = false;
  size_t bucket_bytes = 0, out_bytes = 0, bit_bytes = 0;  // one bucket; one MSM's read-back, dense and bits
};

struct BatchPlan {
  size_t count = 0, nseg = 1;
  BatchSchedule sched = kOneLane;
  int lanes = 1;
  bool host = false;            // scalar sets are copied from host memory (kCopy)
  bool combine_per_group = false;  // plain engine: host combine of group q after its tail, no stream syncs
  // a front group of several jobs reads their scalars with one stride: the
  // segments' slices are n strings apart, so groups > 1 need packed sets
  size_t jstride = 0;
  bool packed = true;
  RedGroups rg;
  size_t group_max = 1;
  bool bit_tail = false, tail_coop = true, l0_first = false;
  int fine_bt = 1024;
  size_t fg_max = 1, nfg = 0;
  std::vector<size_t> fgb;
  // Rings.  Front sets g % nfr: the lane schedules (small MSMs, periods of a
  // few hundred us) keep fronts further ahead.  Reducer sets q % nred: with
  // lanes group q reuses set q % 4 after tail q - 4 (a tail is ~30 latency-
  // bound launches, ~1 ms beside the accumulations: with 2 sets group q + 2
  // waited for it, profiles/archive_r01_r04.txt (r04_batch_trace_2p17.txt)).
  // Bucket sets k % bsets (one lane), k % lanes (lanes), g % 2 (groups).
  int nfr = 3, nred = 2, bsets = 2;
  // Host sets: device slots for up to 32 front groups (<= 2 GiB, at least 4),
  // so a batch of up to 32 groups issues every copy at its start and the copy
  // stream runs them back to back, ahead of the fronts; a longer batch copies
  // group g once group g - nsg's front has consumed its slots.  With 4 slots
  // (copies issued 4 MSMs ahead, each after a front event) the 2^20 H2D
  // headline fell into a slow schedule in about half the runs (372-391 vs
  // 411-417 M pairs/s, more often after a 3-set warm-up); with a slot per set
  // every run gave 418-423 M (profiles/archive_r01_r04.txt (r04_h2d_slots_ab.txt)).
  // Every group's copies are enqueued before its front: nsg >= nfr - 1.
  size_t sslot = 0, slot_groups = 0, nsg = 0, pace = 0;
  // the accumulations of the released group a front waits on: its last and the
  // front_waits - 1 before it (the other lanes'); the plain engine's waits on 1
  int front_waits = 1;
  // Buffers the set-up ensures before the first launch (an allocation inside
  // the issue loop could synchronise the device), sized for the knobs' maxima
  // whatever this batch's length: a short warm-up batch must leave nothing to
  // allocate inside a longer one.
  size_t out_need = 0, out_alloc = 0, bits_need = 0, bits_alloc = 0;
  size_t bucket_set_bytes = 0;  // kAccGroups: each of the two lanes' group sets; else each of bucket_sets sets
  int bucket_sets = 2;
  size_t scal_bytes = 0, scal_dummy_bytes = 0, sorted_min = 0;
  // Events, indices into the engine's event vector: one start, per MSM its
  // accumulation and level 0, per front group its front and copy, per reduction
  // group its tail.  The join uses join_ev on join_stream in order: CHES its
  // two own join events (indices events, events + 1), the plain engine the
  // start event again.
  size_t events = 0, events_floor = 0, ev_front0 = 0, ev_copy0 = 0, ev_tail0 = 0;
  size_t ev_start() const { return 0; }
  size_t ev_acc(size_t k) const { return 1 + k; }
  size_t ev_l0(size_t k) const { return 1 + count + k; }
  size_t ev_front(size_t g) const { return ev_front0 + g; }
  size_t ev_copy(size_t g) const { return ev_copy0 + g; }
  size_t ev_tail(size_t q) const { return ev_tail0 + q; }
  size_t join_ev[3] = {0, 0, 0};
  static constexpr BatchStream join_stream[3] = {kFront, kLane1, kLane2};

  // kAccGroups issues a front group's level 0s before the tails of the
  // reduction groups that end in it, and level 0 of group q waits for tail
  // q - nred: a front group may span at most nred reduction groups, or that
  // wait names a tail not yet issued (reduction groups of 1 with front groups
  // of 8: the CPU schedule test found it; no other pair of values it sweeps is capped)
  static size_t acc_group_cap(int nred, size_t group_max) { return (size_t)nred * group_max; }

  static BatchPlan ches(const BatchShape &z, const BatchKnobs &kn) {
    BatchPlan p;
    p.count = z.nsets * z.nseg, p.nseg = z.nseg, p.lanes = z.lanes, p.host = z.host;
    p.jstride = z.nseg == 1 ? z.set_stride : z.n * z.stride;
    p.packed = z.nseg == 1 || z.set_stride == z.nseg * z.n * z.stride;
    p.group_max = (size_t)(kn.red_group ? kn.red_group : ChesBatch::kGroup);
    p.rg = RedGroups(p.count, p.group_max);
    p.bit_tail = kn.bit_tail && !z.dev_out && z.bit_tail_ok;
    p.tail_coop = kn.tail_coop, p.fine_bt = kn.fine_bt;
    p.l0_first = kn.acc_after_l0 < 0 ? z.group == 1 : kn.acc_after_l0 == 1;
    const int nl = z.lanes;
    const bool acc_groups = nl >= 2 && z.nseg == 1 && kn.acc_group;
    p.sched = acc_groups ? kAccGroups : nl >= 2 ? kLanes : kOneLane;
    // small MSMs on lanes: groups of 2 on two lanes -- half the front launches,
    // measured 0.551 -> 0.530 ms per 2^17 MSM and 0.874 -> 0.845 at 2^18 -- and 4
    // on three lanes (profiles/archive_r01_r04.txt (r04_small_lanes_ab.txt)); the
    // 2^20 batch keeps 1, its wider fronts starve the accumulation
    // (r03_front_group_ab.txt and r04_front_group_ab.txt: resident 2.33-2.38 ms
    // per MSM with groups of 8 vs 2.26-2.27 with groups of 1)
    p.fg_max = !p.packed ? 1 : kn.front_group ? (size_t)kn.front_group : acc_groups ? 4 : nl >= 3 ? 4 : nl == 2 ? 2
                                                                       : (size_t)ChesBatch::kFrontGroupDefault;
    p.nfr = nl >= 2 ? ChesBatch::kFrontsMax : ChesBatch::kFronts;
    p.nred = nl >= 2 ? 4 : 2;
    if (acc_groups) p.fg_max = std::min(p.fg_max, acc_group_cap(p.nred, p.group_max));
    p.fgb = front_groups(p.count, p.fg_max);
    p.nfg = p.fgb.size() - 1;
    p.bsets = ChesBatch::kBSets;
    p.front_waits = nl;
    p.sslot = z.n * z.stride;
    p.slot_groups = std::max<size_t>(
        kn.h2d_slots ? (size_t)kn.h2d_slots
                     : std::max<size_t>(4, std::min<size_t>(32, ((size_t)2 << 30) / std::max<size_t>(1, p.fg_max * p.sslot))),
        (size_t)p.nfr - 1);
    p.nsg = std::max<size_t>(std::min(p.slot_groups, p.nfg), (size_t)p.nfr - 1);
    p.pace = z.host && kn.copy_pace >= 3 ? (size_t)kn.copy_pace : 0;
    // at least 256 MSMs' worth of read-back slots (a few hundred KiB): no regrowth per batch size
    p.out_need = p.count * z.out_bytes, p.out_alloc = std::max<size_t>(p.count, 256) * z.out_bytes;
    p.bits_need = p.bit_tail ? p.group_max * z.bit_bytes : 0;
    p.bits_alloc = std::max<size_t>(p.group_max, 32) * z.bit_bytes;
    p.bucket_sets = acc_groups ? 2 : std::max(ChesBatch::kBSets, nl);
    p.bucket_set_bytes = (acc_groups ? p.fg_max : 1) * z.buckets * z.bucket_bytes;
    p.scal_bytes = z.host ? p.slot_groups * p.fg_max * p.sslot + 16 : 0;
    p.scal_dummy_bytes = p.fg_max * p.sslot + 16;
    p.sorted_min = z.n * (size_t)z.h * p.fg_max * 4;
    p.layout(true);
    // created once for at least 64 MSMs (not inside a timed batch), and with one spare per MSM
    p.events_floor = std::max<size_t>(p.events + p.count, 3 * 64 + 3 * 64 + 1);
    p.join_ev[0] = p.join_ev[1] = p.events, p.join_ev[2] = p.events + 1;
    return p;
  }

  // the plain engine: accumulation groups over device sets, three streams
  static BatchPlan plain(size_t count, const BatchKnobs &kn) {
    BatchPlan p;
    p.count = count, p.lanes = 2, p.sched = kAccGroups, p.combine_per_group = true;
    p.group_max = (size_t)(kn.pip_group ? kn.pip_group : PlainBatch::kGroup);
    p.rg = RedGroups(count, p.group_max);
    p.tail_coop = kn.tail_coop, p.fine_bt = kn.pip_fine_bt;
    p.nfr = PlainBatch::kFronts, p.nred = PlainBatch::kRedSets;
    p.fg_max = std::min((size_t)kn.pip_front_group, acc_group_cap(p.nred, p.group_max));
    p.fgb = front_groups(count, p.fg_max);
    p.nfg = p.fgb.size() - 1;
    p.nsg = p.nfg;
    p.layout(false);
    return p;
  }

 private:
  void layout(bool copy_events) {
    ev_front0 = 1 + 2 * count;
    ev_copy0 = ev_front0 + nfg;
    ev_tail0 = ev_copy0 + (copy_events ? nfg : 0);
    events = ev_tail0 + rg.groups();
  }
};

// The issue loops.  Sink (streams are BatchStream values, events plan indices):
//   wait(stream, ev)  record(ev, stream)  host_wait(ev)  sync(stream)
//   copy_set(g, k)              scalar set k into its slot of slot group g % nsg, on kCopy
//   front(g)                    digits + sort of front group g into front set g % nfr, on kFront
//   accumulate(s, g, k, bset)   MSM k (set k - fgb[g] of front set g % nfr) into bucket set bset
//   accumulate_group(s, g, gb)  front group g in one launch into lane gb's bucket sets
//   level0(s, bset, rset, slot)              one MSM's buckets into its slot of reducer set rset
//   level0_group(s, gb, off, rset, slot0, m) m MSMs from lane gb's sets off .. off + m - 1
//   tail(s, rset, first, m, last)            the group's tail levels and its read-back
//   combine(first, m)           plain engine: the host combine of a finished group
//   prof_begin(s, k)  prof_end(s, k)         profiling records around an accumulation
// Rules, held by the CPU test for every shape it sweeps:
//  - every wait names an event recorded earlier in this call;
//  - a ring slot (front set, bucket set, reducer slot, scalar slot group) is
//    written only after every earlier read of it, by the events named at each wait;
//  - front g + 1 is enqueued before accumulation g + 1 waits on it: fronts run up
//    to nfr - 1 groups ahead on their stream, but each is ENQUEUED after the
//    accumulation before it (enqueuing the first nfr - 1 fronts, 7 launches
//    each, before the first accumulation cost ~0.3 ms of host time at the start
//    of a small-MSM batch, profiles/r05_small_trace.txt);
//  - no host wait inside the loops but the paced copies': every MSM has its own
//    read-back slot, and every launch beside an accumulation costs it ~10-20 us
//    (profiles/archive_r01_r04.txt (r02_batch_sched2.txt)), so the ~35 latency-
//    bound tail levels are paid once per reduction group, not once per MSM.
template <class Sink>
struct BatchIssue {
  const BatchPlan &p;
  Sink &o;
  size_t fronts_issued = 0;
  size_t acc_enq = 0;  // accumulations whose event is recorded in this batch
  BatchIssue(const BatchPlan &plan, Sink &sink) : p(plan), o(sink) {}

  void run() {
    start();
    if (p.sched == kAccGroups) acc_groups();
    if (p.sched == kLanes) lanes();
    if (p.sched == kOneLane) one_lane();
    join();
  }

  // The batch starts after prior work on the caller's stream.  The copy stream
  // does NOT wait on the start event: an SDMA copy enqueued behind a cross-
  // stream event wait now and then blocked the issuing thread -- the one that
  // enqueues the whole pipeline -- for 7-9 ms (rocprofv3 HIP API traces of
  // bench.py: the batch's second hipMemcpyAsync took 7.4 ms in 3 of 5 traced
  // runs, the GPU idle meanwhile; tools/microbench/copy_block.hip: blocked calls
  // only with the wait; profiles/r05_h2d_block.txt).  Prior work on the caller's
  // stream (which may write the host sets) is awaited on the host instead; the
  // device slots are only read by this engine's batches, which end synchronised.
  void start() {
    o.record(p.ev_start(), kCaller);
    o.wait(kFront, p.ev_start());
    if (p.host) o.host_wait(p.ev_start());
    o.wait(kLane1, p.ev_start());
    o.wait(kLane2, p.ev_start());
    for (size_t g = 0; g < (p.pace ? std::min(p.nsg, p.pace) : p.nsg); ++g) copy_group(g);
    issue_fronts(0);
  }

  void copy_group(size_t g) {
    if (!p.host || g >= p.nfg) return;
    if (g >= p.nsg) o.wait(kCopy, p.ev_front(g - p.nsg));  // slots consumed by front g - nsg
    for (size_t k = p.fgb[g]; k < p.fgb[g + 1]; ++k) o.copy_set(g, k);
    o.record(p.ev_copy(g), kCopy);
  }

  // A paced copy waits (on the host) for MSM fgb[g] - pace clamped to the last
  // accumulation already enqueued in THIS batch: in the accumulation-group
  // schedule front g is issued when only the groups up to g - nfr + 1 are
  // enqueued, so it never waits on a stale or unrecorded event and cannot deadlock.
  void front_group(size_t g) {
    if (g >= p.nfg) return;
    if (p.pace && g >= p.pace && g < p.nsg) {
      if (acc_enq) o.host_wait(p.ev_acc(std::min(p.fgb[g] - p.pace, acc_enq - 1)));
      copy_group(g);
    }
    if (p.host) o.wait(kFront, p.ev_copy(g));
    if (g >= (size_t)p.nfr) {  // front set g % nfr: every accumulation of group g - nfr has read it
      const size_t last = p.fgb[g - p.nfr + 1] - 1;
      o.wait(kFront, p.ev_acc(last));
      for (size_t d = 1; d < (size_t)p.front_waits && last >= d && last - d >= p.fgb[g - p.nfr]; ++d)
        o.wait(kFront, p.ev_acc(last - d));
    }
    o.front(g);
    o.record(p.ev_front(g), kFront);
  }
  void issue_fronts(size_t upto) {  // every front group <= upto not yet enqueued
    for (; fronts_issued <= upto && fronts_issued < p.nfg; ++fronts_issued) front_group(fronts_issued);
  }

  // Bucket sets gb are reused by lane gb only, in stream order; reducer set
  // q % nred by group q + nred after tail q.
  void acc_groups() {
    for (size_t g = 0; g < p.nfg; ++g) {
      copy_group(g + p.nsg);
      const size_t k0 = p.fgb[g], k1 = p.fgb[g + 1];
      const int gb = (int)(g & 1), L = gb ? kLane1 : kCaller;
      o.wait(L, p.ev_front(g));
      o.prof_begin(L, k0);
      o.accumulate_group(L, g, gb);
      o.prof_end(L, k0);
      for (size_t k = k0; k < k1; ++k) o.record(p.ev_acc(k), L);
      acc_enq = k1;
      for (size_t a = k0; a < k1;) {  // level 0, one launch per reduction group touched
        const size_t q = p.rg.of(a), b = std::min(k1, p.rg.first(q + 1));
        if (q >= (size_t)p.nred) o.wait(L, p.ev_tail(q - p.nred));  // reducer set free again
        o.level0_group(L, gb, a - k0, (int)(q % p.nred), (int)p.rg.slot(a), (int)(b - a));
        a = b;
      }
      for (size_t k = k0; k < k1; ++k) o.record(p.ev_l0(k), L);
      for (size_t k = k0; k < k1; ++k) {  // tails of the reduction groups ending in [k0, k1)
        if (!p.rg.ends(k)) continue;
        const size_t q = p.rg.of(k), first = p.rg.first(q);
        o.wait(kLane2, p.ev_l0(k));                                       // this lane's level 0s of group q
        if (k0 >= 1 && k0 - 1 >= first) o.wait(kLane2, p.ev_l0(k0 - 1));  // the other lane's
        o.tail(kLane2, (int)(q % p.nred), first, k - first + 1, k + 1 == p.count);
        o.record(p.ev_tail(q), kLane2);
      }
      issue_fronts(g + p.nfr - 1);
    }
  }

  void lanes() {
    const int nl = p.lanes, ts = nl == 3 ? kFront : kLane2;
    for (size_t g = 0; g < p.nfg; ++g) {
      copy_group(g + p.nsg);
      for (size_t k = p.fgb[g]; k < p.fgb[g + 1]; ++k) {
        const size_t q = p.rg.of(k);
        const int L = (int)(k % nl), bset = L, slot = (int)p.rg.slot(k), rset = (int)(q % p.nred);
        o.wait(L, p.ev_front(g));
        if (q >= (size_t)p.nred && slot < nl) o.wait(L, p.ev_tail(q - p.nred));  // reducer set free again
        o.prof_begin(L, k);
        o.accumulate(L, g, k, bset);
        o.prof_end(L, k);
        o.record(p.ev_acc(k), L);
        acc_enq = k + 1;
        o.level0(L, bset, rset, slot);
        o.record(p.ev_l0(k), L);
        if (p.rg.ends(k)) {  // the group's level 0s are done on every lane
          for (int d = 0; d < nl && d <= slot; ++d) o.wait(ts, p.ev_l0(k - d));
          o.tail(ts, rset, k - slot, (size_t)slot + 1, k + 1 == p.count);
          o.record(p.ev_tail(q), ts);
        }
      }
      issue_fronts(g + p.nfr - 1);
    }
  }

  // Reducer set t is reused by group q + 2 only after group q's tail: both are
  // in order on kLane1 + t.
  void one_lane() {
    for (size_t g = 0; g < p.nfg; ++g) {
      copy_group(g + p.nsg);
      o.wait(kCaller, p.ev_front(g));
      for (size_t k = p.fgb[g]; k < p.fgb[g + 1]; ++k) {
        const int bset = (int)(k % p.bsets), slot = (int)p.rg.slot(k), rset = (int)(p.rg.of(k) % p.nred);
        const int ts = kLane1 + rset;
        if (k >= (size_t)p.bsets) o.wait(kCaller, p.ev_l0(k - p.bsets));  // bucket set free again
        if (p.l0_first && k >= 1) o.wait(kCaller, p.ev_l0(k - 1));
        o.prof_begin(kCaller, k);
        o.accumulate(kCaller, g, k, bset);
        o.prof_end(kCaller, k);
        o.record(p.ev_acc(k), kCaller);
        acc_enq = k + 1;
        o.wait(ts, p.ev_acc(k));
        o.level0(ts, bset, rset, slot);
        o.record(p.ev_l0(k), ts);
        if (p.rg.ends(k)) o.tail(ts, rset, k - slot, (size_t)slot + 1, k + 1 == p.count);
      }
      issue_fronts(g + p.nfr - 1);
    }
  }

  // the caller's stream observes completion of every stream of the batch
  void join() {
    // plain engine: the host Horner of group q (one per MSM) overlaps the GPU
    // work of later groups
    for (size_t q = 0; p.combine_per_group && q < p.rg.groups(); ++q) {
      o.host_wait(p.ev_tail(q));
      o.combine(p.rg.first(q), p.rg.first(q + 1) - p.rg.first(q));
    }
    for (int i = 0; i < 3; ++i) {
      o.record(p.join_ev[i], BatchPlan::join_stream[i]);
      o.wait(kCaller, p.join_ev[i]);
    }
    if (p.combine_per_group) return;
    o.sync(kLane1);
    o.sync(kLane2);
    o.sync(kFront);  // three lanes: the group read-backs ran on the front stream
  }
};

}  // namespace msm
