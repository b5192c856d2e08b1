#!/bin/bash
# usage (on the GPU box): tools/ab.sh <kbench args...>   -- runs kbench once per lib/libttemb_*.so, alternating twice
R=$(cd "$(dirname "$0")/.." && pwd)
cd $R
for rep in 1 2; do
  for lib in falcon-ttdforgnns_amd/lib/libttemb_*.so; do
    echo -n "$(basename $lib) : "
    TTEMB_LIB=$PWD/$lib python3 tools/kbench.py "$@" | tail -1
  done
done
