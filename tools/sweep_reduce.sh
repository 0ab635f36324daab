# level 1 of the bucket reduction of one MSM alone at 2^20: SBN_RED_L = buckets per lane (any value; default: chosen so the chunks spread evenly over
# the SIMDs).
# First the MSM parity tests under the odd values (ragged last chunk), then the timings.
for L in 3 5 7; do
  SBN_RED_L=$L timeout -k 10 300 python -m pytest tests/test_gpu_msm.py -m gpu -x -q 2>&1 | tail -1 || exit 1
done
for L in - 3 4 5 6 8; do
  if [ "$L" = "-" ]; then unset SBN_RED_L; else export SBN_RED_L=$L; fi
  python bench.py --full --steps 12 --warmup 3 --blocks none --no-cpu-baseline --inflight 1 2>/dev/null | python -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1]); k=d['serial_reference']['kernels_avg_ms']
print('L=$L ms_per_step', d['ms_per_step'], 'l1', k['k_reduce_l1'], 'combine', k['k_reduce_combine'], 'acc', k['k_acc_first'])"
done
