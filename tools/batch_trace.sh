#!/bin/bash
# HIP runtime API traces of every MSM batch schedule of one build:
# each case of tools/batch_cases.py in its own process (the batch knobs are read
# once per process) under `rocprofv3 --hip-runtime-trace` alone, JSON output,
# each under its own time limit; the first failure ends the script.  Run it on
# two builds and compare case by case with tools/hip_trace_compare.py.
# usage: bash tools/batch_trace.sh <tree whose msm_blst_amd is built> <output dir>
TREE=$(cd "$1" && pwd)
OUT=$2
HERE=$(cd "$(dirname "$0")" && pwd)
mkdir -p "$OUT"
t() {  # name, "ENV=..." list, then the arguments of batch_cases.py
  local name=$1 envs=$2
  shift 2
  env $envs timeout -k 10 150 rocprofv3 --hip-runtime-trace --output-format json -d "$OUT/$name" -o t -- \
    python3 "$HERE/batch_cases.py" "$TREE" "$@" > "$OUT/$name.txt" 2>&1 || { tail -5 "$OUT/$name.txt"; echo "FAILED $name"; exit 1; }
  echo "$name: $(grep -c "^CALL" "$OUT/$name.txt") calls, $(grep -E "^(OK|MISMATCH)" "$OUT/$name.txt")"
}
# CHES, accumulation groups (the default for small MSMs); then the reducer ring of 4 wrapping
t ches_default "" ches 19 device pinned pageable
t ches_red2 "MSM_RED_GROUP=2" ches 19 device pinned pageable
# per-MSM lanes
t lanes3 "MSM_ACC_GROUP=0 MSM_BATCH_LANES=3 MSM_RED_GROUP=2" ches 19 device pinned
t lanes2 "MSM_ACC_GROUP=0 MSM_BATCH_LANES=2 MSM_RED_GROUP=2" ches 19 device pinned
# one lane, 40 host sets: the slot groups wrap and the paced copies run
t one_lane "MSM_BATCH_LANES=1" ches 40 pinned
t one_lane_slots4 "MSM_BATCH_LANES=1 MSM_H2D_SLOTS=4" ches 40 pinned
t one_lane_pace0 "MSM_BATCH_LANES=1 MSM_COPY_PACE=0" ches 40 pinned
t one_lane_free "MSM_BATCH_LANES=1 MSM_ACC_AFTER_L0=0" ches 40 pinned
t one_lane_dense "MSM_BATCH_LANES=1 MSM_BIT_TAIL=0" ches 40 pinned
t one_lane_nocoop "MSM_BATCH_LANES=1 MSM_TAIL_COOP=0" ches 40 pinned
t one_lane_fg8 "MSM_BATCH_LANES=1 MSM_FRONT_GROUP=8" ches 40 pinned
# profiling in each schedule
t prof_groups "" profile 19 device
t prof_lanes "MSM_ACC_GROUP=0" profile 19 device
t prof_one_lane "MSM_BATCH_LANES=1" profile 19 device
# two segments per set: two shards on one device
t segments "" segments 5 pinned
# the plain engine
t plain "" plain 19 device pinned
t plain_group2 "MSM_PIP_GROUP=2" plain 19 device pinned
t plain_fg1 "MSM_PIP_FRONT_GROUP=1" plain 19 device pinned
t plain_fg8 "MSM_PIP_FRONT_GROUP=8" plain 19 device pinned
# no batch: one synchronous MSM per engine (compare with --no-alloc: the reducer's buffer sizing)
t sync "" sync
