#!/bin/bash
# Builds the CPU execution of the transforms over Fr (csrc/frntt.hpp, 256 emulated lanes) with the numbers of csrc/plan.hpp frntt_sizes_for,
# as a host library of its own (tests only): tests/test_frntt_emu.py, tests/test_frntt_plan.py.
set -e
cd "$(dirname "$0")"
mkdir -p _build
if [ ! -f _build/libfrntt.so ] || [ frntt.cpp -nt _build/libfrntt.so ] || [ -n "$(find ../../nim-blscurve_amd/csrc -name '*.hpp' -newer _build/libfrntt.so)" ]; then
  hipcc -O2 -std=c++17 -x hip --offload-host-only -g -rdynamic -fPIC -shared -I ../../nim-blscurve_amd/csrc frntt.cpp -o _build/libfrntt.so.$$
  mv _build/libfrntt.so.$$ _build/libfrntt.so
fi
