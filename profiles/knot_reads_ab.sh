#!/bin/bash
# Builds the A/B variant of round 5 beside the product library (here, no GPU needed):
#   bash profiles/knot_reads_ab.sh         summersph_amd/libsummersph_hip_read2.so      -DSPH_KNOTS_READ2: the two table knots as one
#                                          ds_read2_b64 again, in every kernel that keeps its table in LDS (pair_common.hpp)
# then on the GPU box:  SUMMERSPH_LIB=summersph_amd/libsummersph_hip_read2.so python bench.py --gpus 1 --steps 20 --warmup 5
set -e -o pipefail
cd "$(dirname "$0")/../summersph_amd/csrc"
make -j8 >/dev/null
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -fno-gpu-rdc -Wall -Wno-unused-result"
OBJS="api grid pairs integrate varh tiled gravity accrete domain render profile energy groups gradients sample gravity_at bound cube terms binned trace"
variant() {      # <suffix> <macro> <sources that see the macro>
  local list=""
  for s in $3; do /opt/rocm/bin/hipcc $FLAGS -D$2 -c $s.hip -o $tmp/$1_$s.o & done
  wait
  for o in $OBJS; do
    if [[ " $3 " == *" $o "* ]]; then list="$list $tmp/$1_$o.o"; else list="$list $o.o"; fi
  done
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -fno-gpu-rdc -shared -o ../libsummersph_hip_$1.so $list
  echo built summersph_amd/libsummersph_hip_$1.so
}
variant read2 SPH_KNOTS_READ2 "pairs varh tiled terms"
