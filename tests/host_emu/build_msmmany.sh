#!/bin/bash
# Builds the launch plan of k MSMs in one pass (csrc/plan.hpp msm_many_for and friends) and the CPU execution of its counting sort
# (csrc/msmmany.hpp) as two host libraries of their own (tests only): tests/test_msm_many_plan.py, tests/test_msm_many_emu.py,
# tests/test_gpu_msm_many.py.
set -e
cd "$(dirname "$0")"
mkdir -p _build
if [ "$1" != "emu" ]; then
  if [ ! -f _build/libplan_msmmany.so ] || [ plan_msmmany.cpp -nt _build/libplan_msmmany.so ] || [ ../../nim-blscurve_amd/csrc/plan.hpp -nt _build/libplan_msmmany.so ]; then
    ${CXX:-c++} -O1 -std=c++17 -Wall -Wextra -Werror -fPIC -shared -I ../../nim-blscurve_amd/csrc plan_msmmany.cpp -o _build/libplan_msmmany.so.$$
    mv _build/libplan_msmmany.so.$$ _build/libplan_msmmany.so
  fi
fi
if [ "$1" != "plan" ]; then
  if [ ! -f _build/libmsmmany.so ] || [ msmmany.cpp -nt _build/libmsmmany.so ] || [ -n "$(find ../../nim-blscurve_amd/csrc -name '*.hpp' -newer _build/libmsmmany.so)" ]; then
    hipcc -O2 -std=c++17 -x hip --offload-host-only -DBLS_TRACK_BOUNDS -g -rdynamic -fPIC -shared -I ../../nim-blscurve_amd/csrc msmmany.cpp -o _build/libmsmmany.so.$$
    mv _build/libmsmmany.so.$$ _build/libmsmmany.so
  fi
fi
