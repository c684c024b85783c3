#!/bin/bash
# Compare the gfx950 device assembly of every device object of two trees (a refactor that claims "same bits, same registers, same speed" shows it here, without a GPU):
#   [JOBS=16] [OUT=/tmp/rsim_isa] [REUSE_A=1] tools/isa_compare.sh <tree A> <tree B>   ->  one `object: N differing lines of M` row per object
# Each object's command line is the one its Makefile rule would run (`make -n -B <object>`) with `-c` replaced by `-S --cuda-device-only`, so no flag is retyped here.
# Lines with __hip_cuid (a hash of the source text) are left out of the comparison.  REUSE_A=1 keeps the assembly of tree A from an earlier call.
set -eu
a=$(cd "$1" && pwd); b=$(cd "$2" && pwd)
OUT=${OUT:-${TMPDIR:-/tmp}/rsim_isa}; JOBS=${JOBS:-16}
objs="rsim_step rsim_step_cfg1 rsim_step_cfg2 rsim_step_cfg3 rsim_step_cfg4 rsim_step_cfg5 rsim_episode rsim_sensors rsim_ray rsim_ik rsim_dist rsim_clear rsim_sweep"
mkdir -p $OUT/a $OUT/b
emit() {  # <tree> <out dir>: the commands, one per line, then run JOBS at a time
  for o in $objs; do
    make -s -n -B -C "$1/robosuite_amd/csrc" $o.o | sed -e "s| -c | -S --cuda-device-only |" -e "s| -o $o\.o| -o $2/$o.s|" -e "s|^|cd $1/robosuite_amd/csrc \&\& |"
  done | xargs -P $JOBS -d '\n' -n 1 bash -c
}
[ "${REUSE_A:-0}" = 1 ] || emit "$a" $OUT/a
emit "$b" $OUT/b
for o in $objs; do
  grep -v __hip_cuid $OUT/a/$o.s > $OUT/a/$o.cmp; grep -v __hip_cuid $OUT/b/$o.s > $OUT/b/$o.cmp
  n=$(diff $OUT/a/$o.cmp $OUT/b/$o.cmp | grep -c '^[<>]' || true)
  echo "$o: $n differing lines of $(wc -l < $OUT/b/$o.cmp)"
done
