#!/bin/bash
# Builds the CPU execution of the cell-proof call (csrc/fk20cells.hpp, bounds tracked) and the numbers of csrc/plan.hpp fk20_cells_sizes_for,
# as host libraries of their own (tests only): tests/test_fk20_cells_emu.py, tests/test_fk20_cells_plan.py.
set -e
cd "$(dirname "$0")"
mkdir -p _build
for name in fk20cells plan_fk20cells; do
  if [ ! -f _build/lib$name.so ] || [ $name.cpp -nt _build/lib$name.so ] || [ -n "$(find ../../nim-blscurve_amd/csrc -name '*.hpp' -newer _build/lib$name.so)" ]; then
    hipcc -O2 -std=c++17 -x hip --offload-host-only -DBLS_TRACK_BOUNDS -g -rdynamic -fPIC -shared -I ../../nim-blscurve_amd/csrc $name.cpp -o _build/lib$name.so.$$
    mv _build/lib$name.so.$$ _build/lib$name.so
  fi
done
