#!/bin/bash
# Builds the launch plan of the fixed-base table MSM (csrc/plan.hpp fixed_for and friends) as a host library and as a sanitized program of its
# own, and the CPU execution of its counting sort (csrc/msmtable.hpp) as a second host library (tests only): tests/test_msm_table_plan.py,
# tests/test_msm_table_emu.py, tests/test_gpu_msm_table.py.
set -e
cd "$(dirname "$0")"
mkdir -p _build
CSRC=../../nim-blscurve_amd/csrc
if [ "$1" = "plan" ] || [ -z "$1" ]; then
  if [ ! -f _build/libplan_msmtable.so ] || [ plan_msmtable.cpp -nt _build/libplan_msmtable.so ] || [ $CSRC/plan.hpp -nt _build/libplan_msmtable.so ]; then
    ${CXX:-c++} -O1 -std=c++17 -Wall -Wextra -Werror -fPIC -shared -I $CSRC plan_msmtable.cpp -o _build/libplan_msmtable.so.$$
    mv _build/libplan_msmtable.so.$$ _build/libplan_msmtable.so
  fi
fi
if [ "$1" = "san" ]; then
  if [ ! -f _build/plan_msmtable_san ] || [ plan_msmtable.cpp -nt _build/plan_msmtable_san ] || [ $CSRC/plan.hpp -nt _build/plan_msmtable_san ]; then
    ${CXX:-c++} -O1 -g -std=c++17 -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -DPLAN_MSMTABLE_MAIN -I $CSRC plan_msmtable.cpp \
      -o _build/plan_msmtable_san.$$
    mv _build/plan_msmtable_san.$$ _build/plan_msmtable_san
  fi
fi
if [ "$1" = "emu" ] || [ -z "$1" ]; then
  if [ ! -f _build/libmsmtable.so ] || [ msmtable.cpp -nt _build/libmsmtable.so ] || [ -n "$(find $CSRC -name '*.hpp' -newer _build/libmsmtable.so)" ]; then
    hipcc -O2 -std=c++17 -x hip --offload-host-only -DBLS_TRACK_BOUNDS -g -rdynamic -fPIC -shared -I $CSRC msmtable.cpp -o _build/libmsmtable.so.$$
    mv _build/libmsmtable.so.$$ _build/libmsmtable.so
  fi
fi
