#!/bin/bash
# usage: RTMI_COMMIT=<sha> [RTMI_PMC_CONFIG='{json}'] [RTMI_PMC_OUT=<dir>] tools/pmc_run.sh <tag> <bench args...>   (on the GPU machine)
# Separate rocprofv3 --pmc passes (no tracing domains combined with counters), CSV output under RTMI_PMC_OUT (default:
# build/pmc_<tag> in this repository).  Profiles the bench.py of the repository the script lives in.
# The profiled frame runs on ONE internal stream (RTMI_STREAMS=1): every launch has the GPU to itself, the launch set bench.py's
# roofline object times.
export RTMI_STREAMS=1
ROOT=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
tag=$1; shift
out=${RTMI_PMC_OUT:-$ROOT/build/pmc_$tag}
mkdir -p $out
cd /tmp && export TMPDIR=/tmp
i=0
for set in "SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_VMEM SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY" \
           "SQ_ACTIVE_INST_VALU SQ_THREAD_CYCLES_VALU SQ_ACTIVE_INST_ANY SQ_BUSY_CYCLES SQ_INSTS_SMEM SQ_ACTIVE_INST_VMEM SQ_ACTIVE_INST_LDS SQ_INST_CYCLES_VMEM" \
           "FETCH_SIZE" \
           "WRITE_SIZE TCC_HIT_sum TCC_MISS_sum" \
           "TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_sum GRBM_GUI_ACTIVE"; do
  i=$((i+1))
  # a failed pass (fault, abort, time limit) ends the run: nothing more is started on the GPU after it
  if ! timeout -k 10 300 rocprofv3 --pmc $set --output-format csv -d $out/p$i -- python3 $ROOT/bench.py --steps 1 --warmup 0 --no-cpu-baseline --no-counters --no-d2h-leg "$@" > $out/p$i.log 2>&1; then
    echo "pass $i failed: $(tail -2 $out/p$i.log)"
    exit 1
  fi
done
python3 $ROOT/tools/pmc_summarize.py $out ${RTMI_PMC_CONFIG:+"$RTMI_PMC_CONFIG"}
