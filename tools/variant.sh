#!/bin/bash
# Kernel A/B experiments: build librescan_hip_<tag>.so with extra -D flags and select it at run time with
# RS_HIP_LIB=<path> (rescan_amd/capi.py).   usage: tools/variant.sh <tag> [-DNAME=VALUE ...]
#   tools/variant.sh dbg -DRS_DBG=1            per-tile timers of the search kernels (RS_HIP_DEBUG_CYCLES)
#   tools/variant.sh taildbg -DRS_TAIL_DBG=1   phase stamps of k_plain_moments / k_icp_update_wide, rs_hip_debug_tail_dump (csrc/rs_tail_dbg.h)
#   tools/variant.sh s0 -DRS_COOP_STREAM=0     the cooperative ICP kernels with sweep_shell instead of the row table and stream (rs_search.h)
#   tools/variant.sh s2 -DRS_COOP_PREFETCH=2 [-DRS_COOP_OCC=5]   chunks of a wave in flight / the kernels' waves-per-SIMD target
#   tools/variant.sh c4 -DRS_XCD_CHUNK_LOG2=4 [-DRS_XCD_CHUNK_WARM_LOG2=4]   phase A's tile map, cold / warm launches: chunks of 2^4 natural blocks; -1: contiguous eighths (rs_xcdmap.h)
set -e
cd "$(dirname "$0")/../rescan_amd"
tag=$1; shift
F="-O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-slp-vectorize -fPIC -Wall -Wno-unused-function"
objs=""
units=$(python -c "import build; print(' '.join(s[:-4] for s in build.SOURCES if s != 'rs_build.hip'))")      # (the library's own list: rescan_amd/build.py)
for tu in $units; do
  /opt/rocm/bin/hipcc $F "$@" -c csrc/$tu.hip -o /tmp/${tu}_$tag.o &
  objs="$objs /tmp/${tu}_$tag.o"
done
wait
[ -f csrc/rs_build.o ] || /opt/rocm/bin/hipcc $F -c csrc/rs_build.hip -o csrc/rs_build.o      # (no experiment flags in the index build; hipCUB: ~20 s)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $objs csrc/rs_build.o -o librescan_hip_$tag.so
echo "$(pwd)/librescan_hip_$tag.so"
