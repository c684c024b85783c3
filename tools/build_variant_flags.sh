#!/bin/bash
# Build a variant of SEVERAL kernel configurations next to the default library: each listed configuration is compiled with its own CFGnFLAGS plus the extra
# flags, every other object is shared with the default build (run `make` first):
#   tools/build_variant_flags.sh <name> "<extra flags>" <cfg> [<cfg> ...]   ->  robosuite_amd/librsim_hip_<name>.so
#   tools/build_variant_flags.sh nopf -DRSIM_NO_CAND_PREFETCH 0 1           (tests/test_candidate_descriptors.py)
set -eu
name=$1; extra=$2; shift 2
cd "$(dirname "$0")/../robosuite_amd/csrc"
for v in CXXFLAGS CFG0FLAGS CFG1FLAGS CFG2FLAGS CFG3FLAGS TORCH_LIB HIPCC ARCH; do eval "$v=\"$(make -s print-$v)\""; done
CFG4FLAGS=""; CFG5FLAGS=$CFG3FLAGS
D=${TMPDIR:-/tmp}/rsim_variant_$name; mkdir -p $D
pids=""
for c in "$@"; do
  eval "fl=\$CFG${c}FLAGS"
  $HIPCC $CXXFLAGS -I. -I../../include -DRSIM_CFG=$c $fl $extra -x hip -c rsim_step.hip -o $D/cfg$c.o & pids="$pids $!"
done
for p in $pids; do wait $p; done
objs=""
for c in 0 1 2 3 4 5; do
  o=rsim_step_cfg$c.o; [ $c = 0 ] && o=rsim_step.o
  [ -f $D/cfg$c.o ] && [[ " $* " == *" $c "* ]] && o=$D/cfg$c.o
  objs="$objs $o"
done
$HIPCC --offload-arch=$ARCH -shared -fPIC -o ../librsim_hip_$name.so $objs rsim_episode.o rsim_sensors.o rsim_ray.o rsim_ik.o rsim_dist.o rsim_clear.o rsim_sweep.o rsim_api.o rsim_mjcf.o -L$TORCH_LIB -Wl,-rpath,$TORCH_LIB
echo built ../librsim_hip_$name.so
