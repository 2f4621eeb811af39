#!/bin/bash
# librsx with the window kernel's region timers compiled in (RSX_WINDOW_PROF, csrc/sc_window.hip): abtest/librsx_winprof.so
# Use: RSX_LIB_PATH=abtest/librsx_winprof.so python bench.py --gpus 1 --steps 1 --warmup 0 --only-main --no-cpu-baseline
# prints one "[sc_window prof]" line per wave index and launch on stderr.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
C=$ROOT/navtech-radar-slam_amd/csrc
OUT=${1:-$ROOT/abtest/librsx_winprof.so}
make -C $C -j8 > /dev/null
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
mkdir -p "$(dirname "$OUT")"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt \
  -I$ROOT/include -I$C -DRSX_WINDOW_PROF=1 $EXTRA_DEFS -x hip -c $C/sc_window.hip -o $TMP/sc_window.hip.o
OBJS=$(ls $C/build/*.o | grep -v sc_window.hip.o)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $OBJS $TMP/sc_window.hip.o -ldl -o "$OUT"
echo built "$OUT"
