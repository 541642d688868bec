#!/bin/bash
# One GPU pass over the tree: the GPU suite, smoke, and the full bench line (logs tagged $1; the bench's
# detail file at its default path).  Stops at the first step that faults, aborts or times out.
set -u
TAG=${1:-run}
step() {  # name, timeout, command...
  local name=$1 t=$2; shift 2
  timeout -k 10 "$t" "$@" > "gpurun_out/${TAG}_${name}.txt" 2>&1
  local rc=$?
  echo "$name rc=$rc"
  if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
}
step gpu_tests 900 python -u -m pytest -x -v --timeout 300 --timeout-method thread tests -m gpu
step smoke 300 python -u -c "import __graft_entry__ as g; g.smoke()"
step bench 900 python -u bench.py --full
