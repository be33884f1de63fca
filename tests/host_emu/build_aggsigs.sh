#!/bin/bash
# Builds the CPU execution of the per-group signature aggregation's item bodies, of the signature compression and of the signature-only
# decoder (csrc/aggsigs.hpp, csrc/deser.hpp, bounds tracked), with the workspace sizes of csrc/plan.hpp aggsigs_sizes_for, as a host library of
# its own (tests only): tests/test_aggsigs_emu.py, tests/test_aggsigs_plan.py.
set -e
cd "$(dirname "$0")"
mkdir -p _build
if [ ! -f _build/libaggsigs.so ] || [ aggsigs.cpp -nt _build/libaggsigs.so ] || [ -n "$(find ../../nim-blscurve_amd/csrc -name '*.hpp' -newer _build/libaggsigs.so)" ]; then
  hipcc -O2 -std=c++17 -x hip --offload-host-only -DBLS_TRACK_BOUNDS -g -rdynamic -fPIC -shared -I ../../nim-blscurve_amd/csrc aggsigs.cpp -o _build/libaggsigs.so.$$
  mv _build/libaggsigs.so.$$ _build/libaggsigs.so
fi
