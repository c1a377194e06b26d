"""Compare the HIP runtime API traces of two builds call for call.

Input: the JSON results of `rocprofv3 --hip-runtime-trace --output-format json`
(alone: no counters, no other tracing) of the same script on two builds.  Per
thread, in issue order, every call is reduced to what must not change between
builds of one schedule: the API name, the stream and the event it names
(handles numbered by first appearance, so two runs' addresses compare), the
direction and byte count of a copy or memset, and the kernel (by name where the
trace maps its host function, else numbered by first appearance) with grid and
block of a launch.  Addresses of buffers, and everything else, are left out.

usage: hip_trace_compare.py <a_results.json> <b_results.json> [--show N] [--no-alloc]
       --no-alloc leaves hipMalloc / hipFree out (two builds that size or allocate their buffers differently)
       hip_trace_compare.py --reduce <results.json> <out.json.gz>   (a smaller file the first form also reads)
prints EQUAL and the call count, or the first N differing calls; exit status 1
if the traces differ."""
import gzip
import json
import sys

HANDLES = {"stream": "s", "hStream": "s", "event": "e", "start": "e", "stop": "e"}
PLAIN = ("kind", "sizeBytes", "size", "count", "value", "flags", "priority", "numBlocks", "dimBlocks", "gridDim", "blockDim",
         "sharedMemBytes", "sharedMem")
# calls that hand a new handle back through a pointer: the argument is an address on the caller's stack
CREATES = ("hipStreamCreate", "hipEventCreate")


def load(path):
    doc = json.load(gzip.open(path) if path.endswith(".gz") else open(path))
    if "reduced" in doc:  # written by --reduce
        return doc["reduced"], {int(k): v for k, v in doc["kernels"].items()}
    t = doc["rocprofiler-sdk-tool"][0]
    names = {}
    for i, k in enumerate(t["strings"]["buffer_records"]):
        names[i] = k["operations"]
    kernels = {}
    for h in t.get("host_functions", []):  # host function address -> kernel name, where the trace has it
        addr = h.get("host_function")
        addr = addr.get("handle") if isinstance(addr, dict) else addr
        name = h.get("device_function")
        if addr is not None and name:
            kernels[int(addr, 0) if isinstance(addr, str) else addr] = name
    threads = {}
    for r in sorted(t["buffer_records"]["hip_api"], key=lambda r: r["correlation_id"]["internal"]):
        args = [{"name": a["name"], "value": a.get("value")} for a in r.get("args", [])]
        threads.setdefault(r["thread_id"], []).append((names[r["kind"]][r["operation"]], args))
    return list(threads.values()), kernels


ALLOC = ("hipMalloc", "hipFree")


def reduce_calls(calls, kernels, no_alloc=False):
    seen = {"s": {}, "e": {}, "k": {}}
    count = {"s": 0, "e": 0, "k": 0}

    def number(cls, v):
        if v not in seen[cls]:
            seen[cls][v] = count[cls]
            count[cls] += 1
        return f"{cls}{seen[cls][v]}"

    out = []
    for name, args in calls:
        if no_alloc and name in ALLOC:
            continue
        item = [name]
        for a in args:
            n, v = a["name"], a.get("value")
            if n in HANDLES and not name.startswith(CREATES):
                item.append(f"{n}={number(HANDLES[n], v)}")
            elif n in ("function_address", "f", "hostFunction"):
                try:
                    k = kernels.get(int(v, 0))
                except (TypeError, ValueError):
                    k = None
                item.append(f"kernel={k or number('k', v)}")
            elif n in PLAIN and not str(v).startswith("0x"):  # (a pointer under a plain name: hipGetDeviceCount's count)
                item.append(f"{n}={v}")
        out.append(" ".join(item))
        if name in ("hipEventDestroy", "hipStreamDestroy"):  # the address may come back as a new handle
            for a in args:
                if a["name"] in HANDLES:
                    seen[HANDLES[a["name"]]].pop(a.get("value"), None)
    return out


def main():
    if sys.argv[1] == "--reduce":  # <results.json> <out.json.gz>: names and argument values only, to keep or move
        threads, kernels = load(sys.argv[2])
        with gzip.open(sys.argv[3], "wt") as f:
            json.dump({"reduced": threads, "kernels": kernels}, f)
        return 0
    show = int(sys.argv[sys.argv.index("--show") + 1]) if "--show" in sys.argv else 5
    no_alloc = "--no-alloc" in sys.argv
    (ta, ka), (tb, kb) = load(sys.argv[1]), load(sys.argv[2])
    if len(ta) != len(tb):
        print(f"DIFFER threads that call HIP: {len(ta)} vs {len(tb)}")
        return 1
    total = diffs = 0
    for i, (ca, cb) in enumerate(zip(ta, tb)):
        ra, rb = reduce_calls(ca, ka, no_alloc), reduce_calls(cb, kb, no_alloc)
        total += len(ra)
        if len(ra) != len(rb):
            print(f"DIFFER thread {i}: {len(ra)} vs {len(rb)} calls")
            diffs += 1
        for j, (x, y) in enumerate(zip(ra, rb)):
            if x != y:
                diffs += 1
                if diffs <= show:
                    print(f"DIFFER thread {i} call {j}:\n  a: {x}\n  b: {y}")
    if diffs:
        print(f"DIFFER {diffs} of {total} calls")
        return 1
    print(f"EQUAL {total} calls, {len(ta)} threads, kernels by {'name' if ka and kb else 'first appearance'}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
