#!/bin/bash
# builds the diagnostic (stamped) binary of the fused-tap conv kernel into tools/_bin/conv3_stamp (git-ignored; travels with gpurun)
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
O=$R/tools/_bin
mkdir -p $O
F="--offload-arch=gfx950 -O3 -std=c++17 -DLO_STAMPS"
OBJS=
for f in lo_conv3 lo_conv_geom lo_igemm lo_conv_f8 lo_conv_select lo_wgrad lo_wgrad3 lo_wgrad2 lo_norm; do
  hipcc $F -x hip -c $R/lunaris_orion_amd/csrc/$f.hip -o /tmp/s_$f.o
  OBJS="$OBJS /tmp/s_$f.o"
done
hipcc $F -x hip -c $R/lunaris_orion_amd/csrc/lo_util.cpp -o /tmp/s_util.o
hipcc $F -x hip -c $R/tools/conv3_stamp.cpp -o /tmp/s_main.o
hipcc --offload-arch=gfx950 $OBJS /tmp/s_util.o /tmp/s_main.o -o $O/conv3_stamp
