#!/bin/bash
# Build a variant of SEVERAL kernel configurations next to the default library: each listed configuration is compiled with its own CFGnFLAGS plus the extra
# flags, every other object is shared with the default build (run `make` first):
#   tools/build_variant_flags.sh <name> "<extra flags>" <cfg> [<cfg> ...]   ->  robosuite_amd/librsim_hip_<name>.so
#   tools/build_variant_flags.sh nopf -DRSIM_NO_CAND_PREFETCH 0 1           (tests/test_candidate_descriptors.py)
set -eu
name=$1; extra=$2; shift 2
cd "$(dirname "$0")/../robosuite_amd/csrc"
for v in CXXFLAGS CFG0FLAGS CFG1FLAGS CFG2FLAGS CFG3FLAGS TORCH_LIB HIPCC ARCH STEP_OBJS OTHER_OBJS; do eval "$v=\"$(make -s print-$v)\""; done
CFG4FLAGS=""; CFG5FLAGS=$CFG3FLAGS
D=${TMPDIR:-/tmp}/rsim_variant_$name; mkdir -p $D
so=($STEP_OBJS); pids=""   # the Makefile's link list (STEP_OBJS is in configuration order); the objects built here take their places in it
for c in "$@"; do
  eval "fl=\$CFG${c}FLAGS"
  $HIPCC $CXXFLAGS -I. -I../../include -DRSIM_CFG=$c $fl $extra -x hip -c rsim_step.hip -o $D/cfg$c.o & pids="$pids $!"
  so[$c]=$D/cfg$c.o
done
for p in $pids; do wait $p; done
$HIPCC --offload-arch=$ARCH -shared -fPIC -o ../librsim_hip_$name.so ${so[*]} $OTHER_OBJS -L$TORCH_LIB -Wl,-rpath,$TORCH_LIB
echo built ../librsim_hip_$name.so
