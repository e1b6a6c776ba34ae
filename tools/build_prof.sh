#!/bin/bash
# builds kiss_amd/libkiss_hip.so and phase-profiling variants: of the radix scatter (kiss_amd/libkiss_prof.so.bin,
# -DRX_PROF: per-phase wall-clock ticks of thread 0 of every tile, printed by kiss_radix_check)
set -e
root=$(cd "$(dirname "$0")/.." && pwd)
cd $root/kiss_amd/csrc
make 2>&1 | grep -E "error|warning" || true
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -Wno-unused-result -DRX_PROF $EXTRA -c radix.hip -o /tmp/radix_prof.o
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o ../libkiss_prof.so.bin api.o scan.o classify.o /tmp/radix_prof.o lms_sort.o isa.o place.o induce.o fm.o stages.o multi.o fasta.o general.o verify.o xfer.o lcp.o
# the same from the hooks objects: KISS_HIP_RX_ONE_TILE=1 then profiles k_radix_scatter, nothing set k_radix_scatter_win
# (both phase tables of DESIGN.md 4.0 from one library: KISS_AMD_LIB_PATH=kiss_amd/libkiss_prof_hooks.so.bin)
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -Wno-unused-result -DRX_PROF -DKISS_HIP_HOOKS $EXTRA -c radix.hip -o /tmp/radix_prof.hooks.o
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o ../libkiss_prof_hooks.so.bin api.hooks.o scan.hooks.o classify.hooks.o /tmp/radix_prof.hooks.o lms_sort.hooks.o isa.hooks.o place.hooks.o induce.hooks.o fm.hooks.o stages.hooks.o multi.hooks.o fasta.hooks.o general.hooks.o verify.hooks.o xfer.hooks.o lcp.hooks.o
# the same for the one-pass flag + compaction of round 0 (-DFC_PROF: lms_sort.hip prints "[fc_prof] ..." after the pass)
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -Wno-unused-result -DFC_PROF $EXTRA -c lms_sort.hip -o /tmp/lms_fcprof.o
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o ../libkiss_fcprof.so.bin api.o scan.o classify.o radix.o /tmp/lms_fcprof.o isa.o place.o induce.o fm.o stages.o multi.o fasta.o general.o verify.o xfer.o lcp.o
ls -la ../libkiss_prof.so.bin ../libkiss_fcprof.so.bin ../libkiss_hip.so
