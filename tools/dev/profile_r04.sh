#!/bin/bash
# rocprofv3 passes behind profiles/r04_* (run on the GPU box from the repo root; each pass is its own run: PMC passes carry no trace domains).
# pass 1: kernel trace of the pipelined job. passes 2-6: with every K1 kernel in line on one stream and K1 of a tile not overlapped with the
# previous tile's consumers (NGSQC_K1_SERIAL=1 NGSQC_PIPELINE=0), so that a dispatch's counters are not mixed with a concurrent kernel's.
set -u
R=${GRAFT_REPO_ROOT:-$(pwd)}; O=$R/gpurun_out; mkdir -p $O
export NGSQC_BENCH_NO_STRONG=1 NGSQC_BENCH_NO_E2E=1
CMD="python $R/bench.py --full --reads 48000000 --steps 3 --warmup 1 --no-cpu-baseline --image-cache /tmp/ngsqc_prof_48m.bam"
cd /tmp && export TMPDIR=/tmp
timeout 400 rocprofv3 --kernel-trace --stats -d $O/r4_trace -o t -- $CMD > $O/r4_trace.log 2>&1
export NGSQC_K1_SERIAL=1 NGSQC_PIPELINE=0
timeout 400 rocprofv3 --kernel-trace --stats -d $O/r4_trace_serial -o t -- $CMD > $O/r4_trace_serial.log 2>&1
timeout 400 rocprofv3 --pmc FETCH_SIZE -d $O/r4_fetch -o f -- $CMD > $O/r4_fetch.log 2>&1
timeout 400 rocprofv3 --pmc WRITE_SIZE -d $O/r4_write -o w -- $CMD > $O/r4_write.log 2>&1
timeout 400 rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_ANY -d $O/r4_sq -o s -- $CMD > $O/r4_sq.log 2>&1
timeout 400 rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_ACTIVE_INST_LDS -d $O/r4_sq2 -o s -- $CMD > $O/r4_sq2.log 2>&1
cd $R
python tools/dev/save_profile.py r04 > $O/r4_save.log 2>&1
tail -2 $O/r4_*.log | cut -c1-300
