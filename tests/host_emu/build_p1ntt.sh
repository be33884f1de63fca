#!/bin/bash
# Builds the CPU execution of the transforms over G1 (csrc/p1ntt.hpp, bounds tracked) and the numbers of csrc/plan.hpp p1ntt_sizes_for, as
# host libraries of their own (tests only): tests/test_p1ntt_emu.py, tests/test_p1ntt_plan.py.
set -e
cd "$(dirname "$0")"
mkdir -p _build
for name in p1ntt plan_p1ntt; do
  if [ ! -f _build/lib$name.so ] || [ $name.cpp -nt _build/lib$name.so ] || [ -n "$(find ../../nim-blscurve_amd/csrc -name '*.hpp' -newer _build/lib$name.so)" ]; then
    hipcc -O2 -std=c++17 -x hip --offload-host-only -DBLS_TRACK_BOUNDS -g -rdynamic -fPIC -shared -I ../../nim-blscurve_amd/csrc $name.cpp -o _build/lib$name.so.$$
    mv _build/lib$name.so.$$ _build/lib$name.so
  fi
done
