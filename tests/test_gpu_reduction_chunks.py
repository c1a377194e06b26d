"""GPU parity of the weighted reduction under level-0 chunk lengths that change
the number and parity of its levels (MSM_L0_CHUNK; csrc/reduce_plan.hpp): the
partials ping-pong between two buffers with different per-MSM strides, and which
buffer a level reads, and with which stride, follows from how many levels came
before it.  No other test sets the knob: chunks of 3 and of 64 move the level
count away from that of the default chunks (2 or 8) for the synchronous tail (bit
sums) and for the group tails of a batch (dense stage, bit sums for the last
group).

In child processes (the knob is read once per process): CHES G1 at 2^10, CHES G2
at 2^8 and the plain engine at n = 256, one synchronous MSM and a batch of 3 sets
each, every result against the oracle's naive MSM (oracle/msm_oracle.c), the
reference's own check of every method (ref main_p1.cpp:470-580)."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

import oracle_ffi as of

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 3
SHAPES = [("ches", 1, 1 << 10), ("ches", 2, 1 << 8), ("plain", 1, 256)]

CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import torch
torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py _torch_hip_first)
import msm_blst_amd as m
out = []
for kind, group, n in json.loads(sys.argv[2]):
    if kind == "ches":
        ctx, kw = m.CHESContext(group, 0, n_exp=n.bit_length() - 1), {}
        ctx.build_table(m.fixed_points(group, n), n)
    else:
        ctx, kw = m.MSMContext(group, 0, 10), {"nbits": 255}
        ctx.set_points(m.fixed_points(group, n), n)
    sets = [bytes(m.gen_scalars(n, 700 + k)) for k in range(int(sys.argv[3]))]
    sync = m.compress(group, ctx.mult(sets[0], **kw)).hex()
    batch = [m.compress(group, r).hex() for r in ctx.mult_batch(b"".join(sets), len(sets), **kw)]
    ctx.close()
    out.append({"sync": sync, "batch": batch})
print("RESULT", json.dumps(out))
"""


@pytest.fixture(scope="module")
def want():
    """the oracle's naive MSM of every shape and scalar set, computed once"""
    import msm_blst_amd as m
    res = []
    for _, group, n in SHAPES:
        pts = bytes(m.fixed_points(group, n))
        P = (ctypes.c_uint8 * len(pts)).from_buffer_copy(pts)
        row = []
        for k in range(K):
            sc = bytes(m.gen_scalars(n, 700 + k))
            S = (ctypes.c_uint8 * len(sc)).from_buffer_copy(sc)
            row.append(of.compress(group, of.msm(group, P, S, n, 255, "naive")))
        res.append(row)
    return res


@pytest.mark.parametrize("chunk", [3, 64])
def test_chunked_reductions_vs_oracle(want, chunk):
    env = dict(os.environ, MSM_L0_CHUNK=str(chunk))
    r = subprocess.run([sys.executable, "-c", CHILD, REPO, json.dumps(SHAPES), str(K)], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, r.stdout[-2000:] + r.stderr[-2000:]
    got = json.loads(line[0][7:])
    for shape, g, w in zip(SHAPES, got, want):
        assert g["sync"] == w[0], (shape, chunk)
        assert g["batch"] == w, (shape, chunk)
