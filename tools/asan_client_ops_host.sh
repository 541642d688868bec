#!/usr/bin/env bash
# Host AddressSanitizer + UBSan run of the resident client key's host code: builds the sanitizer
# variant of libfhe_rocm.so (`make -C fhe-sign_amd asan`, -fsanitize on the host compilation only), compiles
# tools/client_ops_host_check.c -- a stand-alone program with its own main that links the sanitizer runtime itself
# -- against it and runs it: the addressing sweep of tests/test_client_ops.py into buffers of exactly the rows'
# size, the stream accounting, the phases, the refusals.  Nothing is preloaded and no Python runs under this build.
# CPU only: the program makes no GPU call, and this is not for a GPU machine.
# Fails on any sanitizer report or a non-zero exit status of the program.
# Usage: tools/asan_client_ops_host.sh [log]   (default log: profiles/r23/asan_client_ops_host.log)
set -euo pipefail
cd "$(dirname "$0")/.."
LOG=${1:-profiles/r23/asan_client_ops_host.log}
mkdir -p "$(dirname "$LOG")"
CLANG=${CLANG:-/opt/rocm/lib/llvm/bin/clang}
make -C fhe-sign_amd asan -j16 >/dev/null
RTDIR=$(dirname "$("$CLANG" -print-file-name=libclang_rt.asan-x86_64.so)")
EXE=fhe-sign_amd/build_asan/client_ops_host_check
"$CLANG" -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libsan -Iinclude \
  tools/client_ops_host_check.c -Lfhe-sign_amd/lib_asan -lfhe_rocm -Wl,-rpath,"$PWD/fhe-sign_amd/lib_asan" \
  -Wl,-rpath,"$RTDIR" -o "$EXE"
REV=nogit
if git rev-parse --short HEAD >/dev/null 2>&1; then
  REV=$(git rev-parse --short HEAD)
  git diff --quiet HEAD || REV="$REV + uncommitted changes"
fi
{
  echo "# host address + undefined-behaviour sanitizer run: $(date -u +%FT%TZ), $REV"
  echo "# flags: -fsanitize=address,undefined -fno-sanitize-recover=undefined (host code only), detect_leaks=1"
  st=0
  ASAN_OPTIONS=detect_leaks=1:halt_on_error=1:exitcode=66 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 \
    timeout -k 10 900 "$EXE" 2>&1 || st=$?
  echo "# exit status: $st"
} | sed "s#$PWD/##g" > "$LOG"   # paths relative to the checkout: logs of two trees compare
grep "SUMMARY: \|# exit status\|^client ops host check" "$LOG" || true
grep -q "ERROR: AddressSanitizer\|ERROR: LeakSanitizer\|runtime error:" "$LOG" && { echo "sanitizer findings, see $LOG"; exit 1; }
grep -q "# exit status: 0" "$LOG"
