#!/bin/bash
# Instruction counts of the device code (CPU only: hipcc -S for gfx950):
# one Montgomery product / square / two-product sum, one xyzz madd and one general
# xyzz add (G1, G2 lane pair), the accumulation kernels and the reduction's
# segment sums as built.  usage: bash tools/isa_report.sh > profiles/<round>_isa_counts.txt
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d)
HIPCC="/opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S -I$R/include"
$HIPCC -o $T/ops.s $R/tools/microbench/isa_ops.hip
$HIPCC -DMSM_GROUP=1 -o $T/ches1.s $R/msm_blst_amd/csrc/ches.hip
$HIPCC -DMSM_GROUP=2 -o $T/ches2.s $R/msm_blst_amd/csrc/ches.hip
echo "# gfx950 ISA instruction counts ($(date -u +%F), $(git -C $R rev-parse --short HEAD))"
echo "# per-op kernels: tools/microbench/isa_ops.hip (one op between a load and a store)"
for k in _Z11k_op_fp_mulP k_op_fp_sqr k_op_fp_mul2 k_op_g2l_mul_bs k_op_g2l_sqr k_op_g2l_mul_sub k_op_g1_madd k_op_g2l_madd k_op_g1_add k_op_g2l_add k_op_fp_mul_chain k_op_fp_sqr_chain k_op_fp_mul2_chain k_op_g1_madd_chain k_op_g1_add_chain; do python3 $R/tools/isa_count.py $T/ops.s $k; done
echo "# accumulation kernels as built (ches.hip, MSM_GROUP=1 / 2)"
python3 $R/tools/isa_count.py $T/ches1.s k_accumulate
python3 $R/tools/isa_count.py $T/ches2.s k_accumulate2p
echo "# segment sums of the reduction as built (level 0: k_segsum; G2: k_segsum2p)"
python3 $R/tools/isa_count.py $T/ches1.s 8k_segsumI
python3 $R/tools/isa_count.py $T/ches2.s 10k_segsum2p
echo "# registers and occupancy (waves per SIMD) of the same kernels"
python3 $R/tools/kernel_resources.py $T/ches1.s 8k_segsumI
python3 $R/tools/kernel_resources.py $T/ches2.s 10k_segsum2p
python3 $R/tools/kernel_resources.py $T/ches1.s 12k_accumulateILi1
# the G1 kernels under the column-form knobs (MSM_ACC_CHAIN, MSM_SEGSUM_CHAIN; fp.hpp MulChain)
# and the accumulation at 4 waves per SIMD
for cfg in "-DMSM_ACC_CHAIN=0 -DMSM_SEGSUM_CHAIN=0" "-DMSM_ACC_CHAIN=1 -DMSM_SEGSUM_CHAIN=0" \
           "-DMSM_ACC_CHAIN=0 -DMSM_SEGSUM_CHAIN=1" "-DMSM_ACC_CHAIN=1 -DMSM_SEGSUM_CHAIN=0 -DMSM_ACC_WAVES=4"; do
  $HIPCC -DMSM_GROUP=1 $cfg -o $T/ches1v.s $R/msm_blst_amd/csrc/ches.hip
  echo "# column forms: $cfg"
  for k in 12k_accumulateILi1 8k_segsumI; do
    python3 $R/tools/isa_count.py $T/ches1v.s $k
    python3 $R/tools/kernel_resources.py $T/ches1v.s $k
  done
done
rm -rf $T
