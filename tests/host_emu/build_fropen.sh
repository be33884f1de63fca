#!/bin/bash
# Builds the CPU execution of the openings over Fr (csrc/fropen.hpp, 256 emulated lanes) with the numbers of csrc/plan.hpp fropen_sizes_for,
# as a host library of its own (tests only): tests/test_fropen_emu.py, tests/test_fropen_plan.py.
set -e
cd "$(dirname "$0")"
mkdir -p _build
if [ ! -f _build/libfropen.so ] || [ fropen.cpp -nt _build/libfropen.so ] || [ plan_fropen.cpp -nt _build/libfropen.so ] || [ -n "$(find ../../nim-blscurve_amd/csrc -name '*.hpp' -newer _build/libfropen.so)" ]; then
  hipcc -O2 -std=c++17 -x hip --offload-host-only -g -rdynamic -fPIC -shared -I ../../nim-blscurve_amd/csrc fropen.cpp plan_fropen.cpp -o _build/libfropen.so.$$
  mv _build/libfropen.so.$$ _build/libfropen.so
fi
