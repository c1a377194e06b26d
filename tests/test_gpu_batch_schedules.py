"""GPU parity of the batch schedules of csrc/batch_plan.hpp with short reduction groups,
so that every ring wraps inside a small batch: K = 19 MSMs, G1 at 2^12 and G2 at 2^10,
scalar sets in device and in page-locked host memory, two batches per context, every
result against the synchronous MSM of its set (tools/batch_cases.py).

With reduction groups of 2 a batch of 19 has ten groups over four reducer sets (two in
the one-lane schedule), and its front groups 1, 1, 2, 4, 4, ... cross group boundaries.
The knobs are read once per process, so each setting runs in a child process."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("MSM_RED_GROUP", "MSM_PIP_GROUP", "MSM_ACC_GROUP", "MSM_BATCH_LANES", "MSM_FRONT_GROUP", "MSM_PIP_FRONT_GROUP",
         "MSM_H2D_SLOTS", "MSM_COPY_PACE", "MSM_BIT_TAIL", "MSM_TAIL_COOP", "MSM_ACC_AFTER_L0")


@pytest.mark.parametrize("kind,env,lanes", [
    ("ches", {"MSM_RED_GROUP": "2"}, None),                                                  # accumulation groups
    ("ches", {"MSM_RED_GROUP": "2", "MSM_ACC_GROUP": "0", "MSM_BATCH_LANES": "3"}, 3),  # per-MSM lanes
    ("ches", {"MSM_RED_GROUP": "2", "MSM_ACC_GROUP": "0", "MSM_BATCH_LANES": "2"}, 2),
    ("plain", {"MSM_PIP_GROUP": "2"}, None),
], ids=["acc_groups", "lanes3", "lanes2", "plain"])
def test_short_reduction_groups(kind, env, lanes):
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "batch_cases.py"), REPO, kind, "19"],
                       capture_output=True, text=True, env=e, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    calls = [ln for ln in r.stdout.splitlines() if ln.startswith("CALL ")]
    assert len(calls) == 4 and all(ln.endswith(" ok") for ln in calls), r.stdout[-2000:]
    if lanes:
        assert all(f" lanes={lanes} " in ln for ln in calls), r.stdout[-2000:]
    assert r.stdout.strip().endswith("OK")
