"""GPU parity of the one-lane CHES batch at the smallest shape that reuses both
reducer sets (Ches::run_jobs, ches.hip: accumulation k on the caller's stream,
level 0 of MSM k on the tail stream of its reduction group, accumulation k + 1
after it; reducer set q % 2 written again by group q + 2 behind tail q).

A child process with MSM_BATCH_LANES=1 MSM_RED_GROUP=2 (both read once per
process) takes the one-lane schedule at n = 2^10 with reduction groups of two:
a batch of 7 sets is four groups (2, 2, 2, 1), so each reducer set is written a
second time while the batch runs.  The batch runs from page-locked host memory
and from device memory, twice each (every ring reused); each result must equal
the synchronous MSM of its set and set 0 the reference's golden key.  The real
size is test_gpu_batch_one_lane.py::test_one_lane_batch_2p20.

(Level 0 on the accumulation's own stream was measured beside this placement
and not adopted; this test is the shape that change
would have to pass.)
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SCRIPT = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch
import msm_blst_amd as m
n, K = 1 << 10, 7
ctx = m.CHESContext(1, 0, n_exp=10)
ctx.build_table(m.fixed_points(1, n), n)
print("LANES", ctx.batch_lanes())
host = torch.empty(K * n * 32, dtype=torch.uint8, pin_memory=True)
for k in range(K):
    host.numpy()[k * n * 32:(k + 1) * n * 32] = np.frombuffer(m.gen_scalars(n, 1 if k == 0 else 900 + k), dtype=np.uint8)
dev = host.to("cuda:0")
torch.cuda.synchronize()
want = [m.compress(1, ctx.mult(dev.data_ptr() + k * n * 32, on_device=True)).hex() for k in range(K)]
ok = True
for rep in range(2):
    got_h = [m.compress(1, r).hex() for r in ctx.mult_batch(host.data_ptr(), K, set_stride=n * 32, on_device=False)]
    got_d = [m.compress(1, r).hex() for r in ctx.mult_batch(dev.data_ptr(), K, set_stride=n * 32, on_device=True)]
    ok = ok and got_h == want and got_d == want
ctx.close()
print("SET0", want[0])
print("OK" if ok else "MISMATCH")
"""


def test_one_lane_four_reduction_groups(golden):
    env = dict(os.environ, MSM_BATCH_LANES="1", MSM_RED_GROUP="2")
    r = subprocess.run([sys.executable, "-c", _SCRIPT, REPO], capture_output=True, text=True, env=env, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    out = dict(ln.split(" ", 1) for ln in r.stdout.splitlines() if " " in ln)
    assert out.get("LANES") == "1", r.stdout[-2000:]
    want = [c["compressed"] for c in golden("msm_g1.json")["cases"]
            if c["n"] == 1024 and c["seed"] == 1 and c["case"] == "rand" and c["nbits"] == 255][0]
    assert out.get("SET0") == want, r.stdout[-2000:]
    assert r.stdout.strip().endswith("OK"), r.stdout[-2000:]
