#!/bin/bash
# GPU: shader instruction-cache and instruction-fetch counters of one C2 stream replay
# (k_stream), a pass of their own (no tracing beside it).
# usage: tools/pmc_icache.sh OUTDIR [n_tasks]
OUT=$1; N=${2:-1000000}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -s KILL 120 rocprofv3 --pmc SQC_ICACHE_REQ SQC_ICACHE_HITS SQ_IFETCH SQ_BUSY_CYCLES --output-format csv -d $OUT/icache -o run -- python3 tools/stream_once.py $N > $OUT/icache.log 2>&1
rc=$?; tail -2 $OUT/icache.log
exit $rc
