#!/bin/bash
# rocprofv3 evidence for bench.py --full (label path): kernel-trace stats + FETCH_SIZE / WRITE_SIZE passes, on an MI355X.
# Usage: prof_label.sh <tag> <output folder>; everything it writes goes under the output folder.
set -u
R=${GRAFT_REPO_ROOT:-/root/repo}
TAG=${1:-r2}
mkdir -p "${2:?usage: prof_label.sh <tag> <output folder>}" && OUT=$(cd "$2" && pwd)
cd /tmp && export TMPDIR=/tmp
ARGS="--full --steps 20 --warmup 5 --cpu-seconds 0 --parity-frames 0 --no-secondary --timed-only"
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${TAG}_trace -- python3 $R/bench.py $ARGS > $OUT/prof_${TAG}_trace.log 2>&1
# the counter passes need --full: its single-stream pass gives the whole-batch launches scripts/summarize_prof.py reads
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/prof_${TAG}_fetch -- python3 $R/bench.py --full --steps 2 --warmup 1 --cpu-seconds 0 --parity-frames 0 --no-secondary > $OUT/prof_${TAG}_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/prof_${TAG}_write -- python3 $R/bench.py --full --steps 2 --warmup 1 --cpu-seconds 0 --parity-frames 0 --no-secondary > $OUT/prof_${TAG}_write.log 2>&1
cd $OUT && find . -name "*.csv" | head -30; tail -2 prof_${TAG}_trace.log | cut -c1-300
# keep the merge small: drop the per-dispatch traces of the long run, keep stats + pmc csv
find prof_${TAG}_trace -name "*kernel_trace.csv" -size +20M -delete
