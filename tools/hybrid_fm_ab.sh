#!/bin/bash
# Tile height of the pair products (sarssl_gemm_split, csrc/gemm.hip launch_seg): the library's rule against both forced heights, per shape,
# inside single-stream training steps.  Needs a probe build (-DSARSSL_PROBE_ENV, tools/probe_lib.py): the shipped library has the rule only.
#   bash tools/hybrid_fm_ab.sh
set -e
export SARSSL_HIP_LIB=$(python tools/probe_lib.py envprobe -DSARSSL_PROBE_ENV)
for fm in 0 1 2; do
  echo "== SARSSL_SPLIT_FM=$fm (0: the library's rule)"
  SARSSL_SPLIT_FM=$fm python tools/step_gemm_table.py --precision hybrid 2>&1 | grep -E "gemm_split\["
done
