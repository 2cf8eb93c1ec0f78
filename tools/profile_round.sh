#!/bin/bash
# usage (on the GPU box): tools/profile_round.sh <tag> [bench.py args, e.g. --config C4]
# The full bench line (bench.py --full), the rocprofv3 kernel-trace summary of the same command and the HBM
# traffic counters (separate --pmc passes), all under $PROFILE_OUT/<tag>_* (default build/profile); afterwards:
#   python tools/summarize_prof.py <tag> <reads per launch> $PROFILE_OUT/<tag>_stats $PROFILE_OUT/<tag>_fetch $PROFILE_OUT/<tag>_write $PROFILE_OUT/<tag>_sq
tag=${1:?tag}
shift
cd "$(dirname "$0")/.." && export TMPDIR=/tmp || exit 1
out=${PROFILE_OUT:-build/profile}
mkdir -p "$out" || exit 1
# (the profiled runs are plain runs, ONE config: the short legs of the full run launch the same kernel instantiations on other batches)
python bench.py --full "$@" > "$out/${tag}_bench.json.log" 2> "$out/${tag}_bench.err" || exit 1
rocprofv3 --kernel-trace --stats -d "$out/${tag}_stats" -o p --output-format csv -- python bench.py "$@" > "$out/${tag}_stats.log" 2>&1 || exit 1
rocprofv3 --pmc FETCH_SIZE -d "$out/${tag}_fetch" -o p --output-format csv -- python bench.py --steps 2 --warmup 1 "$@" > "$out/${tag}_fetch.log" 2>&1 || exit 1
rocprofv3 --pmc WRITE_SIZE -d "$out/${tag}_write" -o p --output-format csv -- python bench.py --steps 2 --warmup 1 "$@" > "$out/${tag}_write.log" 2>&1 || exit 1
rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_INSTS_LDS -d "$out/${tag}_sq" -o p --output-format csv -- python bench.py --steps 2 --warmup 1 "$@" > "$out/${tag}_sq.log" 2>&1 || exit 1
cat "$out/${tag}_bench.json.log"
rocprofv3 --pmc SQ_BUSY_CYCLES SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT SQ_WAIT_INST_LDS SQ_INSTS_SALU SQ_INSTS_SMEM SQ_WAIT_INST_ANY SQ_INSTS_VMEM -d "$out/${tag}_sq2" -o p --output-format csv -- python bench.py --steps 2 --warmup 1 "$@" > "$out/${tag}_sq2.log" 2>&1 || exit 1
