#!/bin/bash
# Builds the launch plan of the key aggregation by participation bits (csrc/plan.hpp aggbits_measure / aggbits_fill) and the CPU execution of
# its item bodies (csrc/aggbits.hpp, bounds tracked) as two host libraries of their own (tests only): tests/test_aggbits_plan.py,
# tests/test_aggbits_emu.py.
set -e
cd "$(dirname "$0")"
mkdir -p _build
if [ "$1" != "emu" ]; then
  if [ ! -f _build/libplan_aggbits.so ] || [ plan_aggbits.cpp -nt _build/libplan_aggbits.so ] || [ ../../nim-blscurve_amd/csrc/plan.hpp -nt _build/libplan_aggbits.so ]; then
    ${CXX:-c++} -O1 -std=c++17 -Wall -Wextra -Werror -fPIC -shared -I ../../nim-blscurve_amd/csrc plan_aggbits.cpp -o _build/libplan_aggbits.so.$$
    mv _build/libplan_aggbits.so.$$ _build/libplan_aggbits.so
  fi
fi
if [ "$1" != "plan" ]; then
  if [ ! -f _build/libaggbits.so ] || [ aggbits.cpp -nt _build/libaggbits.so ] || [ -n "$(find ../../nim-blscurve_amd/csrc -name '*.hpp' -newer _build/libaggbits.so)" ]; then
    hipcc -O2 -std=c++17 -x hip --offload-host-only -DBLS_TRACK_BOUNDS -g -rdynamic -fPIC -shared -I ../../nim-blscurve_amd/csrc aggbits.cpp -o _build/libaggbits.so.$$
    mv _build/libaggbits.so.$$ _build/libaggbits.so
  fi
fi
