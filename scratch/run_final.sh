#!/bin/bash
# the round's final evidence set in one call: bash scratch/run_final.sh <tag>
TAG=${1:-r05z}
export RUN_DIR=${RUN_DIR:-out/$TAG}     # where the logs and bench lines of this run go (run_profiles.sh writes there too)
bash scratch/run_profiles.sh $TAG
timeout -k 10 300 python bench.py --arch squeezedetplus --batch 16 --full --no-cpu-baseline --no-pipeline > $RUN_DIR/bench_squeezedetplus.json 2> $RUN_DIR/bench_squeezedetplus.err; echo "plus rc $?"
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $RUN_DIR/smoke.log 2>&1; echo "smoke rc $?"; tail -1 $RUN_DIR/smoke.log
timeout -k 10 330 python tools/fuzz_conv.py 150 20261006 > $RUN_DIR/fuzz_conv.log 2>&1; echo "fuzz_conv rc $?"; tail -2 $RUN_DIR/fuzz_conv.log
