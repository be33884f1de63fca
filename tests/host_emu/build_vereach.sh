#!/bin/bash
# Builds the CPU execution of the per-set verification body (csrc/vereach.hpp, bounds tracked) and its launch plan (csrc/plan.hpp each_for)
# as two host libraries of their own (tests only): tests/test_vereach_emu.py, tests/test_vereach_plan.py.
set -e
cd "$(dirname "$0")"
mkdir -p _build
if [ "$1" != "emu" ]; then
  if [ ! -f _build/libplan_each.so ] || [ plan_each.cpp -nt _build/libplan_each.so ] || [ ../../nim-blscurve_amd/csrc/plan.hpp -nt _build/libplan_each.so ]; then
    ${CXX:-c++} -O1 -std=c++17 -Wall -Wextra -Werror -fPIC -shared -I ../../nim-blscurve_amd/csrc plan_each.cpp -o _build/libplan_each.so.$$
    mv _build/libplan_each.so.$$ _build/libplan_each.so
  fi
fi
if [ "$1" != "plan" ]; then
  if [ ! -f _build/libvereach.so ] || [ vereach.cpp -nt _build/libvereach.so ] || [ -n "$(find ../../nim-blscurve_amd/csrc -name '*.hpp' -newer _build/libvereach.so)" ]; then
    hipcc -O2 -std=c++17 -x hip --offload-host-only -DBLS_TRACK_BOUNDS -g -rdynamic -fPIC -shared -I ../../nim-blscurve_amd/csrc vereach.cpp -o _build/libvereach.so.$$
    mv _build/libvereach.so.$$ _build/libvereach.so
  fi
fi
