#!/bin/bash
# builds kiss_amd/libkiss_hip.so and phase-profiling variants: of the radix scatter (kiss_amd/libkiss_prof.so.bin,
# -DRX_PROF: per-phase wall-clock ticks of thread 0 of every tile, printed by kiss_radix_check)
# Every variant is the library's own object list (the Makefile's SRCS) with one object compiled anew.
set -e
root=$(cd "$(dirname "$0")/.." && pwd)
cd $root/kiss_amd/csrc
make 2>&1 | grep -E "error|warning" || true
cc="/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -Wno-unused-result"
objs=$(make -s print-objs)
hook_objs=$(make -s print-hook-objs)
# link_with LIST OLD NEW OUT: the objects of LIST, NEW in the place of OLD
link_with() {
    local list=""
    for o in $1; do
        [ "$o" = "$2" ] && o=$3
        list="$list $o"
    done
    echo "$list" | grep -q -- "$3" || { echo "build_prof.sh: $2 is not in the Makefile's object list" >&2; exit 1; }
    /opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o $4 $list
}
$cc -DRX_PROF $EXTRA -c radix.hip -o /tmp/radix_prof.o
link_with "$objs" radix.o /tmp/radix_prof.o ../libkiss_prof.so.bin
# the same from the hooks objects: KISS_HIP_RX_ONE_TILE=1 then profiles k_radix_scatter, nothing set k_radix_scatter_win
# (both phase tables of DESIGN.md 4.0 from one library: KISS_AMD_LIB_PATH=kiss_amd/libkiss_prof_hooks.so.bin)
$cc -DRX_PROF -DKISS_HIP_HOOKS $EXTRA -c radix.hip -o /tmp/radix_prof.hooks.o
link_with "$hook_objs" radix.hooks.o /tmp/radix_prof.hooks.o ../libkiss_prof_hooks.so.bin
# the same for the one-pass flag + compaction of round 0 (-DFC_PROF: flag_compact.hip, the unit of k_fc0_onepass, prints
# "[fc_prof] ..." after the pass)
$cc -DFC_PROF $EXTRA -c flag_compact.hip -o /tmp/fc_fcprof.o
link_with "$objs" flag_compact.o /tmp/fc_fcprof.o ../libkiss_fcprof.so.bin
ls -la ../libkiss_prof.so.bin ../libkiss_fcprof.so.bin ../libkiss_hip.so
