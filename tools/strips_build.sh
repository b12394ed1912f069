#!/bin/bash
# libclh_dbg.so with only the RV=1 and row-strip classes of K1 (fast to build); extra -D flags may be passed
set -e
cd "$(dirname "$0")/../ciri_long_amd/csrc"
SRCS="$(sed -n 's/^SRCS *:= *//p' Makefile | sed 's/\$(HERE)//g; s/\.hip//g') ssw_wavefront"      # the Makefile's sources, K1 as one object
for f in $SRCS; do
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -DCLH_STRIPS_BUILD "$@" -c $f.hip -o /tmp/$f.dbg.o &
done
wait
hipcc --offload-arch=gfx950 -shared -fPIC -o ../libclh_dbg.so $(for f in $SRCS; do echo /tmp/$f.dbg.o; done) -lz -lpthread
