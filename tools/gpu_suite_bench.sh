#!/bin/bash
# GPU round step: the -m gpu suite (one pytest process, per-test timeout), then the whole bench
# line (bench.py --full). Outputs go to $OUT/$TAG (OUT defaults to out/ in the repository root).
#   TAG=r6x bash tools/gpu_suite_bench.sh [test files]
cd $GRAFT_REPO_ROOT
TAG=${TAG:-r6}; O=${OUT:-out}/$TAG; mkdir -p $O
FILES=${*:-tests}
timeout -k 10 900 python -u -m pytest -m gpu -x -v --timeout 300 --timeout-method thread $FILES > $O/gpu_tests.log 2>&1
rc=$?
tail -30 $O/gpu_tests.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python -u bench.py --full > $O/bench.json 2> $O/bench.err
rc=$?
tail -c 3000 $O/bench.json; tail -5 $O/bench.err
exit $rc
