#!/bin/bash
# builds libclh_dbg.so with the K3 phase clocks compiled in, then prints the breakdown
set -e
cd "$(dirname "$0")/../ciri_long_amd/csrc"
SRCS="$(sed -n 's/^SRCS *:= *//p' Makefile | sed 's/\$(HERE)//g; s/\.hip//g') ssw_wavefront"      # the Makefile's sources, K1 as one object
for f in $SRCS; do
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -DCLH_DEBUG_POA -DCLH_PROBE_BUILD -c $f.hip -o /tmp/$f.dbg.o &
done
wait
hipcc --offload-arch=gfx950 -shared -fPIC -o ../libclh_dbg.so $(for f in $SRCS; do echo /tmp/$f.dbg.o; done) -lz -lpthread
cd ../..
[ -n "$BUILD_ONLY" ] && exit 0
python tools/k3_phases.py "$@"
rm -f ciri_long_amd/libclh_dbg.so
