#!/bin/bash
# Build a variant of ONE kernel configuration next to the default library, sharing every other object of the default build (run `make` first):
#   [SRC=/path/to/other_step.hip] tools/build_variant_cfg.sh <name> <cfg 0..5> "<flags that REPLACE the configuration's CFGnFLAGS>" ["<extra APIFLAGS>"]   ->  robosuite_amd/librsim_hip_<name>.so
set -eu
name=$1; cfg=$2; fl=${3:-}; fa=${4:-}
cd "$(dirname "$0")/../robosuite_amd/csrc"
for v in CXXFLAGS TORCH_LIB HIPCC ARCH STEP_OBJS OTHER_OBJS; do eval "$v=\"$(make -s print-$v)\""; done
D=/tmp/rsim_variant_$name; mkdir -p $D
SRC=${SRC:-rsim_step.hip}
$HIPCC $CXXFLAGS -I. -I../../include -DRSIM_CFG=$cfg $fl -x hip -c $SRC -o $D/cfg.o &
if [ -n "$fa" ]; then $HIPCC $CXXFLAGS $fa -x hip -c rsim_api.cpp -o $D/api.o & else cp rsim_api.o $D/api.o; fi
wait
so=($STEP_OBJS); so[$cfg]=$D/cfg.o   # the Makefile's link list (STEP_OBJS is in configuration order) with the objects built here in place
$HIPCC --offload-arch=$ARCH -shared -fPIC -o ../librsim_hip_$name.so ${so[*]} ${OTHER_OBJS/rsim_api.o/$D/api.o} -L$TORCH_LIB -Wl,-rpath,$TORCH_LIB
echo built ../librsim_hip_$name.so
