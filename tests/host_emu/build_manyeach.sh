#!/bin/bash
# Builds the CPU execution of the per-batch pass (csrc/manyeach.hpp with the combsets / aggveach bodies it joins, bounds tracked) and its plan
# (csrc/plan.hpp manyeach_*) as two host libraries of their own (tests only): tests/test_manyeach_emu.py, tests/test_manyeach_plan.py.
set -e
cd "$(dirname "$0")"
mkdir -p _build
if [ "$1" != "emu" ]; then
  if [ ! -f _build/libplan_manyeach.so ] || [ plan_manyeach.cpp -nt _build/libplan_manyeach.so ] || [ ../../nim-blscurve_amd/csrc/plan.hpp -nt _build/libplan_manyeach.so ]; then
    ${CXX:-c++} -O1 -std=c++17 -Wall -Wextra -Werror -fPIC -shared -I ../../nim-blscurve_amd/csrc plan_manyeach.cpp -o _build/libplan_manyeach.so.$$
    mv _build/libplan_manyeach.so.$$ _build/libplan_manyeach.so
  fi
fi
if [ "$1" != "plan" ]; then
  if [ ! -f _build/libmanyeach.so ] || [ manyeach.cpp -nt _build/libmanyeach.so ] || [ -n "$(find ../../nim-blscurve_amd/csrc -name '*.hpp' -newer _build/libmanyeach.so)" ]; then
    hipcc -O2 -std=c++17 -x hip --offload-host-only -DBLS_TRACK_BOUNDS -g -rdynamic -fPIC -shared -I ../../nim-blscurve_amd/csrc manyeach.cpp -o _build/libmanyeach.so.$$
    mv _build/libmanyeach.so.$$ _build/libmanyeach.so
  fi
fi
