#!/bin/bash
# Builds the launch plan of the same-message pre-aggregation (csrc/plan.hpp combsets_measure) and the CPU execution of its bodies
# (csrc/combsets.hpp, bounds tracked) as two host libraries of their own (tests only): tests/test_combsets_plan.py, tests/test_combsets_emu.py.
set -e
cd "$(dirname "$0")"
mkdir -p _build
if [ "$1" != "emu" ]; then
  if [ ! -f _build/libplan_combsets.so ] || [ plan_combsets.cpp -nt _build/libplan_combsets.so ] || [ ../../nim-blscurve_amd/csrc/plan.hpp -nt _build/libplan_combsets.so ]; then
    ${CXX:-c++} -O1 -std=c++17 -Wall -Wextra -Werror -fPIC -shared -I ../../nim-blscurve_amd/csrc plan_combsets.cpp -o _build/libplan_combsets.so.$$
    mv _build/libplan_combsets.so.$$ _build/libplan_combsets.so
  fi
fi
if [ "$1" != "plan" ]; then
  if [ ! -f _build/libcombsets.so ] || [ combsets.cpp -nt _build/libcombsets.so ] || [ -n "$(find ../../nim-blscurve_amd/csrc -name '*.hpp' -newer _build/libcombsets.so)" ]; then
    hipcc -O2 -std=c++17 -x hip --offload-host-only -DBLS_TRACK_BOUNDS -g -rdynamic -fPIC -shared -I ../../nim-blscurve_amd/csrc combsets.cpp -o _build/libcombsets.so.$$
    mv _build/libcombsets.so.$$ _build/libcombsets.so
  fi
fi
