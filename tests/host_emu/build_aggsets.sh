#!/bin/bash
# Builds the launch plan of the per-set key aggregation (csrc/plan.hpp aggsets_measure / aggsets_fill) and the CPU execution of its item
# bodies (csrc/aggsets.hpp, bounds tracked) as two host libraries of their own (tests only): tests/test_aggsets_plan.py, tests/test_aggsets_emu.py.
set -e
cd "$(dirname "$0")"
mkdir -p _build
if [ "$1" != "emu" ]; then
  if [ ! -f _build/libplan_aggsets.so ] || [ plan_aggsets.cpp -nt _build/libplan_aggsets.so ] || [ ../../nim-blscurve_amd/csrc/plan.hpp -nt _build/libplan_aggsets.so ]; then
    ${CXX:-c++} -O1 -std=c++17 -Wall -Wextra -Werror -fPIC -shared -I ../../nim-blscurve_amd/csrc plan_aggsets.cpp -o _build/libplan_aggsets.so.$$
    mv _build/libplan_aggsets.so.$$ _build/libplan_aggsets.so
  fi
fi
if [ "$1" != "plan" ]; then
  if [ ! -f _build/libaggsets.so ] || [ aggsets.cpp -nt _build/libaggsets.so ] || [ -n "$(find ../../nim-blscurve_amd/csrc -name '*.hpp' -newer _build/libaggsets.so)" ]; then
    hipcc -O2 -std=c++17 -x hip --offload-host-only -DBLS_TRACK_BOUNDS -g -rdynamic -fPIC -shared -I ../../nim-blscurve_amd/csrc aggsets.cpp -o _build/libaggsets.so.$$
    mv _build/libaggsets.so.$$ _build/libaggsets.so
  fi
fi
