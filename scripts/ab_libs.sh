#!/bin/bash
# Interleaved A/B of library variants on ONE box:  scripts/ab_libs.sh REPS name1 name2 ...
#   "main" = the in-tree build, NAME = elasticreconstruction_amd/_ab/liber_hip_NAME.so; NAME@Q runs with GPU_MAX_HW_QUEUES=Q
#   AB_ALONE=1: also the extra pass that runs k_integrate alone (one launch at a time)
#   AB_PLAIN=1: the headline command itself (bench.py --gpus 1 --steps 20 --warmup 2) instead of the --full pass with the roofline figures
#   AB_ICP=N: the --full pass with its ICP leg of N pairs (no CPU sample, no other leg): headline frames/s and the leg's pairs/s
#   AB_TIMEOUT=seconds: time limit of each run (default 240).  A run that fails or runs out of time ends the job: nothing more is started.
set -o pipefail
reps=$1; shift
alone="--no-alone"; [ -n "$AB_ALONE" ] && alone=""
limit="${AB_TIMEOUT:-240}"
for i in $(seq $reps); do
  for vq in "$@"; do
    v="${vq%@*}"
    if [ "$vq" != "$v" ]; then export GPU_MAX_HW_QUEUES="${vq#*@}"; else unset GPU_MAX_HW_QUEUES; fi
    if [ "$v" = main ]; then unset ER_HIP_LIB; else export ER_HIP_LIB=$PWD/elasticreconstruction_amd/_ab/liber_hip_$v.so; fi
    if [ -n "$AB_ICP" ]; then
      timeout -k 10 "$limit" python bench.py --full --steps 20 --warmup 2 --cpu-sample 0 --icp-pairs "$AB_ICP" --no-streamed --no-alone --other-configs 0 --boundary 0 --min-seconds 0.3 2>/dev/null | python -c "
import json,sys
d=json.loads(sys.stdin.readline())
print('%-10s value %8.0f fps  icp %8.1f pairs/s' % ('$vq', d['value'], d['icp']['pairs_per_s']))" || { echo "$vq: run $i failed -- stopping" >&2; exit 1; }
    elif [ -n "$AB_PLAIN" ]; then
      timeout -k 10 "$limit" python bench.py --gpus 1 --steps 20 --warmup 2 2>/dev/null | python -c "
import json,sys
d=json.loads(sys.stdin.readline())
print('%-10s value %8.0f fps  ms/step %.3f' % ('$vq', d['value'], d['ms_per_step']))" || { echo "$vq: run $i failed -- stopping" >&2; exit 1; }
    else
      timeout -k 10 "$limit" python bench.py --full --steps 20 --warmup 2 --cpu-sample 0 --icp-pairs 0 --no-streamed $alone --other-configs 0 --min-seconds 0.3 2>/dev/null | python -c "
import json,sys
d=json.loads(sys.stdin.readline()); r=d['roofline']; a=r.get('kernel_alone')
print('%-10s value %8.0f fps  ms/step %.3f  k_integrate %.3f ms  frac %.3f%s' % ('$vq', d['value'], d['ms_per_step'], r['avg_launch_ms'], r['frac'], ('  alone %.3f ms' % a['avg_launch_ms']) if a else ''))" || { echo "$vq: run $i failed -- stopping" >&2; exit 1; }
    fi
  done
done
unset GPU_MAX_HW_QUEUES ER_HIP_LIB
