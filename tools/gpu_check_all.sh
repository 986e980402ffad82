#!/bin/bash
# kernel + encode + topk parity, then the whole benchmark (development aid)
cd "$(dirname "$0")/.."                       # the repository root
out=${CLIPMI_OUT:-tools_out}; mkdir -p "$out"   # where every file of the run goes
tag=${1:-chk}
timeout -k 10 900 python -m pytest tests/test_kernels_gpu.py tests/test_encode_gpu.py tests/test_topk_gpu.py -q -m gpu -x > $out/${tag}_test.log 2>&1; rc=$?
tail -3 $out/${tag}_test.log
[ $rc -ne 0 ] && exit $rc
bash tools/gpu_full.sh ${tag} bench
