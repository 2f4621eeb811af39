#!/bin/bash
# librsx with the selection kernel's region timers compiled in (RSX_SELECT_PROF, csrc/sc_filter.hip): abtest/librsx_selprof.so
# Use: RSX_LIB_PATH=abtest/librsx_selprof.so python bench.py --gpus 1 --steps 1 --warmup 0 --only-main --no-cpu-baseline
# prints one "[sc_select prof]" line per launch on stderr.  With RSX_SELECT_CAP_ATOMICS=1 every selection is launched twice,
# the second time with its histogram pass limited to the bins the first launch needed: the two alternate in a kernel trace.
# SELECT_PROF=2 tools/build_select_prof.sh <out> builds the capped mode without the timers (for that trace).
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
C=$ROOT/navtech-radar-slam_amd/csrc
OUT=${1:-$ROOT/abtest/librsx_selprof.so}
make -C $C -j8 > /dev/null
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
mkdir -p "$(dirname "$OUT")"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt \
  -I$ROOT/include -I$C -DRSX_SELECT_PROF=${SELECT_PROF:-1} $EXTRA_DEFS -x hip -c $C/sc_filter.hip -o $TMP/sc_filter.hip.o
OBJS=$(ls $C/build/*.o | grep -v sc_filter.hip.o)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $OBJS $TMP/sc_filter.hip.o -ldl -o "$OUT"
echo built "$OUT"
