#!/bin/bash
# Builds the launch plan of batchVerify by message (csrc/plan.hpp slice_for_grouped) and the CPU execution of its device grouping
# (csrc/bymsg.hpp) as two host libraries of their own (tests only): tests/test_bymsg_plan.py, tests/test_bymsg_emu.py.
set -e
cd "$(dirname "$0")"
mkdir -p _build
if [ "$1" != "emu" ]; then
  if [ ! -f _build/libplan_bymsg.so ] || [ plan_bymsg.cpp -nt _build/libplan_bymsg.so ] || [ ../../nim-blscurve_amd/csrc/plan.hpp -nt _build/libplan_bymsg.so ]; then
    ${CXX:-c++} -O1 -std=c++17 -Wall -Wextra -Werror -fPIC -shared -I ../../nim-blscurve_amd/csrc plan_bymsg.cpp -o _build/libplan_bymsg.so.$$
    mv _build/libplan_bymsg.so.$$ _build/libplan_bymsg.so
  fi
fi
if [ "$1" != "plan" ]; then
  if [ ! -f _build/libbymsg.so ] || [ bymsg.cpp -nt _build/libbymsg.so ] || [ -n "$(find ../../nim-blscurve_amd/csrc -name '*.hpp' -newer _build/libbymsg.so)" ]; then
    hipcc -O2 -std=c++17 -x hip --offload-host-only -DBLS_TRACK_BOUNDS -g -rdynamic -fPIC -shared -I ../../nim-blscurve_amd/csrc bymsg.cpp -o _build/libbymsg.so.$$
    mv _build/libbymsg.so.$$ _build/libbymsg.so
  fi
fi
