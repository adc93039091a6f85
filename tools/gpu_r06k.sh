#!/bin/bash
# round 6, step k: K2's epilogue -- K2E 4 + operands before the walk (new
# default) / K2E 4 without (_pre0) / round 5's K2E 8 (_old): the BB tests on
# the default build, then C3 + C5 whole iterations and the 8-way C5 rank-0
# rehearsal, alternating builds
set -o pipefail
cd "${GRAFT_REPO_ROOT:-/root/repo}"
OUT="${OUT:-bench_out}"
mkdir -p $OUT
timeout -k 10 900 python -u -m pytest -x -q --timeout 600 --timeout-method thread tests/test_gpu_bb.py tests/test_gpu_fullsize.py tests/test_gpu_c5.py tests/test_gpu_shard_native.py tests/test_gpu_deep.py > $OUT/r6k_tests.log 2>&1 || exit 1
: > $OUT/r6k_summary.txt
for rep in 1 2; do
for V in "" _pre0 _old; do
  L=$PWD/block-simplex-least-squares_amd/lib/libbsls_hip$V.so
  BSLS_LIB=$L timeout -k 10 300 python -u bench.py --full --legs main,c5 --steps 200 --warmup 20 --windows 5 > $OUT/r6k_b$V.json 2> $OUT/r6k_b$V.err || exit 1
  python -c "
import json; d = json.loads(open('$OUT/r6k_b$V.json').read().strip().splitlines()[-1])
k = d['kernels']; c = d['c5']['kernels']
print('lib=$V C3 it/s %.0f K2 %.2f K1 %.2f K3 %.2f | C5 it/s %.1f K2 %.2f' % (d['value'], k['K2_spmvT_Nt_dots']['avg_us'], k['K1_spmv_A']['avg_us'], k['K3_pava_clip_z2x']['avg_us'], d['c5']['value'], c['K2_spmvT_Nt_dots']['avg_us']))
" >> $OUT/r6k_summary.txt
  BSLS_LIB=$L timeout -k 10 300 python -u bench.py --full --rehearse-shard 8 --steps 200 --warmup 20 --windows 5 > $OUT/r6k_r8$V.json 2> $OUT/r6k_r8$V.err || exit 1
  python -c "
import json; d = json.loads(open('$OUT/r6k_r8$V.json').read().strip().splitlines()[-1])
k = d['kernels']
print('lib=$V C5/8 rank0 us/it %.1f K2 %.2f K1 %.2f' % (d['ms_per_step'] * 1e3, k['K2_spmvT_Nt_dots']['avg_us'], k['K1_spmv_A']['avg_us']))
" >> $OUT/r6k_summary.txt
done
done
