# bench.py --skip-pull tend.u. on two ranks of the one GPU, N times: the first attempt must fail its
# one-block verification and the rerun over send / receive buffers must pass.  BENCH=<script> runs
# another copy of bench.py (e.g. one without the barrier between the two contexts).
set -o pipefail
mkdir -p gpurun_out
B=${BENCH:-bench.py}
for i in $(seq 1 ${N:-8}); do
  timeout -k 10 150 python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 --master-port $((29600 + i)) \
    $B --gpus 2 --same-device --ncells 10242 --steps 3 --warmup 1 --full --no-cpu-baseline --no-configs1 \
    --acoustic-reps 3 --skip-pull tend.u. > gpurun_out/skip_$i.log 2>&1
  r=$?
  python -c "
import json
l=[x for x in open('gpurun_out/skip_$i.log') if x.startswith('{')]
v=json.loads(l[-1])['verify'] if l else {}
print('$B run $i rc=$r', 'first', v.get('first_attempt',{}).get('bitwise_vs_one_block'), 'rerun', v.get('bitwise_vs_one_block'), v.get('max_rel_linf',{}).get('u'))
" | tee -a gpurun_out/skiploop.log
  [ $r -eq 0 ] || [ $r -eq 1 ] || exit $r
done
