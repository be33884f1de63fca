#!/bin/bash
# Builds the CPU execution of the per-group aggregateVerify bodies (csrc/aggveach.hpp, bounds tracked) and its plan (csrc/plan.hpp
# aggveach_*) as two host libraries of their own (tests only): tests/test_aggveach_emu.py, tests/test_aggveach_plan.py.
set -e
cd "$(dirname "$0")"
mkdir -p _build
if [ "$1" != "emu" ]; then
  if [ ! -f _build/libplan_aggveach.so ] || [ plan_aggveach.cpp -nt _build/libplan_aggveach.so ] || [ ../../nim-blscurve_amd/csrc/plan.hpp -nt _build/libplan_aggveach.so ]; then
    ${CXX:-c++} -O1 -std=c++17 -Wall -Wextra -Werror -fPIC -shared -I ../../nim-blscurve_amd/csrc plan_aggveach.cpp -o _build/libplan_aggveach.so.$$
    mv _build/libplan_aggveach.so.$$ _build/libplan_aggveach.so
  fi
fi
if [ "$1" != "plan" ]; then
  if [ ! -f _build/libaggveach.so ] || [ aggveach.cpp -nt _build/libaggveach.so ] || [ -n "$(find ../../nim-blscurve_amd/csrc -name '*.hpp' -newer _build/libaggveach.so)" ]; then
    hipcc -O2 -std=c++17 -x hip --offload-host-only -DBLS_TRACK_BOUNDS -g -rdynamic -fPIC -shared -I ../../nim-blscurve_amd/csrc aggveach.cpp -o _build/libaggveach.so.$$
    mv _build/libaggveach.so.$$ _build/libaggveach.so
  fi
fi
