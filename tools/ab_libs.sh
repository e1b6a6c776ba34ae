#!/bin/bash
# on the GPU box: bench.py alternately with the library in the tree and with a variant build named by path
# (KISS_AMD_LIB_PATH, kiss_amd/_lib.py; default kiss_amd/libkiss_old.so.bin), two rounds each, same box.  The shipped
# library file is never overwritten.  usage: [VARIANT=path] tools/ab_libs.sh [bench args...]
cd ${GRAFT_REPO_ROOT:-.}
VARIANT=${VARIANT:-$PWD/kiss_amd/libkiss_old.so.bin}
out=${AB_OUT_DIR:-ab_out}  # the lines of the runs
mkdir -p "$out"
for r in 1 2; do
  for v in new old; do
    if [ $v = old ]; then export KISS_AMD_LIB_PATH=$VARIANT; else unset KISS_AMD_LIB_PATH; fi
    timeout -k 10 200 python bench.py --full --steps 10 --no-e2e --no-fm --cpu-sample 0 --profile-steps 0 "$@" > "$out/ab_${v}_$r.json" 2> "$out/ab_${v}_$r.err" || exit 1
  done
done
