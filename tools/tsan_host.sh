#!/usr/bin/env bash
# Host ThreadSanitizer run of the threading contract (include/fhe_rocm.h, "Threading"): builds the
# thread-sanitizer variant of libfhe_rocm.so (`make -C fhe-sign_amd tsan`, -fsanitize=thread on the host
# compilation only), compiles tools/threads_host_check.c -- a stand-alone program with its own main that links
# the sanitizer runtime itself -- against it and runs it: four threads, a simulated context each, the first
# use of every radix algorithm behind a barrier.  Nothing is preloaded and no Python runs under this build.
# CPU only: simulated contexts make no GPU call, and this is not for a GPU machine.
# The run takes about a minute.  A race needs the two threads' accesses close together to be seen: the first
# encrypted shift's (profiles/r21/tsan_host_parent.log) showed in most runs of the tool on that tree, not in all.
# Fails on any ThreadSanitizer report or a non-zero exit status of the program (1: a threaded result differs
# from its sequential one or from its expected value; 66: the sanitizer reported).
# Usage: tools/tsan_host.sh [log]   (default log: profiles/r21/tsan_host_tree.log)
set -euo pipefail
cd "$(dirname "$0")/.."
LOG=${1:-profiles/r21/tsan_host_tree.log}
mkdir -p "$(dirname "$LOG")"
CLANG=${CLANG:-/opt/rocm/lib/llvm/bin/clang}
make -C fhe-sign_amd tsan -j16 >/dev/null
RTDIR=$(dirname "$("$CLANG" -print-file-name=libclang_rt.tsan-x86_64.so)")
EXE=fhe-sign_amd/build_tsan/threads_host_check
"$CLANG" -g -O1 -pthread -fsanitize=thread -shared-libsan -Iinclude tools/threads_host_check.c \
  -Lfhe-sign_amd/lib_tsan -lfhe_rocm -Wl,-rpath,"$PWD/fhe-sign_amd/lib_tsan" -Wl,-rpath,"$RTDIR" -o "$EXE"
REV=nogit
if git rev-parse --short HEAD >/dev/null 2>&1; then
  REV=$(git rev-parse --short HEAD)
  git diff --quiet HEAD || REV="$REV + uncommitted changes"
fi
{
  echo "# host thread-sanitizer run: $(date -u +%FT%TZ), $REV"
  echo "# flags: -fsanitize=thread (host code only), halt_on_error=0:exitcode=66"
  st=0
  TSAN_OPTIONS=halt_on_error=0:exitcode=66 \
    timeout -k 10 600 "$EXE" 2>&1 || st=$?
  echo "# exit status: $st"
} | sed "s#$PWD/##g" > "$LOG"   # paths relative to the checkout: logs of two trees compare
grep "SUMMARY: ThreadSanitizer\|# exit status\|^threaded host check" "$LOG" || true
grep -q "ThreadSanitizer" "$LOG" && { echo "sanitizer findings, see $LOG"; exit 1; }
grep -q "# exit status: 0" "$LOG"
