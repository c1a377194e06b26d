"""Accumulations, level 0 and the gaps between accumulations of the last CHES
batch in a rocprofv3 kernel trace of bench.py's headline (G1 n = 2^20): per MSM
the k_accumulate<1> time, the time of the level-0 k_segsum<1> that follows it
(the segment sum with the largest grid before the next accumulation starts) and
the gap from the accumulation's end to the next one's start.  The table of
profiles/first_pair_l0_trace.txt and profiles/xyzz_add_trace.txt.
usage: python tools/l0_trace.py run_kernel_trace.csv [K=20]"""
import csv
import statistics
import sys


def grid(r):
    for k in ("Grid_Size_X", "Grid_Size"):
        if k in r and r[k]:
            return int(r[k])
    return 0


def main(path, K=20):
    rows = list(csv.DictReader(open(path)))
    ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], grid(r)) for r in rows)
    # (demangled or mangled names; k_segsum2p and the _c forms do not match)
    acc = [e for e in ev if "k_accumulate<" in e[2] or "k_accumulateILi" in e[2]][-K:]
    seg = [e for e in ev if "k_segsum<" in e[2] or "k_segsumILi" in e[2]]
    t0 = acc[0][0]
    print(" k  start_ms  acc_ms   l0_ms  gap_ms  l0_start_after_acc_us  next_acc_after_l0_us")
    accs, l0s, gaps, d1, d2 = [], [], [], [], []
    for k, (s, e, _, _) in enumerate(acc):
        nxt = acc[k + 1][0] if k + 1 < len(acc) else None
        cand = [x for x in seg if x[0] >= e and (nxt is None or x[0] < nxt)]
        if nxt is None:  # the last MSM: its level 0 is the first large segment sum after it
            cand = cand[:4]
        l0 = max(cand, key=lambda x: x[3]) if cand else None
        gap = (s - acc[k - 1][1]) / 1e6 if k else 0.0
        a_ms = (e - s) / 1e6
        l_ms = (l0[1] - l0[0]) / 1e6 if l0 else float("nan")
        u1 = (l0[0] - e) / 1e3 if l0 else float("nan")
        u2 = (nxt - l0[1]) / 1e3 if l0 and nxt is not None else float("nan")
        print(f"{k:2d} {(s - t0) / 1e6:9.3f} {a_ms:7.3f} {l_ms:7.3f} {gap:7.3f} {u1:10.1f} {u2:10.1f}")
        accs.append(a_ms)
        if l0:
            l0s.append(l_ms)
            d1.append(u1)
        if k:
            gaps.append(gap)
        if u2 == u2:
            d2.append(u2)
    span = (acc[-1][1] - t0) / 1e6
    print(f"span {span:.3f} ms  per MSM {span / len(acc):.3f}  sum(acc) {sum(accs):.3f}  sum(gaps) {sum(gaps):.3f}")
    med = statistics.median
    print(f"medians: acc {med(accs):.3f} ms  l0 {med(l0s):.4f} ms  gap {med(gaps):.4f} ms  "
          f"acc->l0 {med(d1):.1f} us  l0->acc {med(d2):.1f} us")


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 20)
