#!/bin/bash
# Builds the CPU execution of the short linear combinations (csrc/lincomb.hpp, bounds tracked) with the numbers of csrc/plan.hpp
# lincomb_measure / lincomb_sizes_for, as a host library of its own (tests only): tests/test_lincomb_emu.py, tests/test_lincomb_plan.py.
set -e
cd "$(dirname "$0")"
mkdir -p _build
if [ ! -f _build/liblincomb.so ] || [ lincomb.cpp -nt _build/liblincomb.so ] || [ -n "$(find ../../nim-blscurve_amd/csrc -name '*.hpp' -newer _build/liblincomb.so)" ]; then
  hipcc -O2 -std=c++17 -x hip --offload-host-only -DBLS_TRACK_BOUNDS -g -rdynamic -fPIC -shared -I ../../nim-blscurve_amd/csrc lincomb.cpp -o _build/liblincomb.so.$$
  mv _build/liblincomb.so.$$ _build/liblincomb.so
fi
