#!/bin/bash
# Profiling build of the library (run here, on the CPU; the .so travels to the GPU box):
#   tools/build_prof.sh ekf   -> ekf.hip with -DEKF_PROFILE   (tools/prof_ekf_phases.py)
#   tools/build_prof.sh fte   -> fte.hip with -DFTE_PROFILE   (tools/prof_fte_phases.py, prof_cr_timeline.py)
#   FTE_PROF_DEFS="-DFTE_PROF_WIDE=1000" tools/build_prof.sh fte: the k_cr_level timeline of the
#   levels with >= 1000 elimination workgroups (-DFTE_PROF_WIDE_MAX=n: and <= n)
#   FTE_PROF_DEFS="-DPIVPRIO=0" OUT=libvar.so tools/build_prof.sh ftevar: fte.hip with other
#   compile-time settings and no profiling (A/B variants, loaded through ACINOSET_HIP_LIB)
# Output: acinoset_amd/csrc/build/libprof.so (the other objects from the normal build);
# OUT=name: acinoset_amd/csrc/build/name instead.
set -euo pipefail
cd "$(dirname "$0")/.."
python -c "from acinoset_amd import build; build.build(verbose=False)"
B=acinoset_amd/csrc/build
F="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -I include -Wno-unused-result"
case "${1:-ekf}" in
  ekf) src=ekf; alt=ekf_prof; defs="-DEKF_PROFILE";;
  fte) src=fte; alt=fte_prof; defs="-DFTE_PROFILE ${FTE_PROF_DEFS:-}";;
  ftevar) src=fte; alt=fte_var; defs="${FTE_PROF_DEFS:-}";;
  *) echo "usage: $0 ekf|fte|ftevar"; exit 2;;
esac
/opt/rocm/bin/hipcc $F $defs -c acinoset_amd/csrc/$src.hip -o $B/$alt.o
# one object per csrc/*.hip, as the normal build links them, with the one above in place of its own
objs=""
for f in acinoset_amd/csrc/*.hip; do
  n=$(basename "$f" .hip)
  if [ "$n" = "$src" ]; then objs="$objs $B/$alt.o"; else objs="$objs $B/$n.o"; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $objs -o $B/${OUT:-libprof.so}
echo "built $B/${OUT:-libprof.so} (${1:-ekf})"
