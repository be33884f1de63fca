#!/bin/bash
# Builds the plan of the pairing-product calls (csrc/plan.hpp pairprod_* and the sig-less aggveach_fill) as a host library and as a sanitized
# program of its own, and the CPU execution of the pair-slot bodies (csrc/pairprod.hpp, bounds tracked) as a second host library (tests only):
# tests/test_pairprod_plan.py, tests/test_pairprod_emu.py.
set -e
cd "$(dirname "$0")"
mkdir -p _build
CSRC=../../nim-blscurve_amd/csrc
if [ "$1" = "plan" ]; then
  if [ ! -f _build/libplan_pairprod.so ] || [ plan_pairprod.cpp -nt _build/libplan_pairprod.so ] || [ $CSRC/plan.hpp -nt _build/libplan_pairprod.so ]; then
    ${CXX:-c++} -O1 -std=c++17 -Wall -Wextra -Werror -fPIC -shared -I $CSRC plan_pairprod.cpp -o _build/libplan_pairprod.so.$$
    mv _build/libplan_pairprod.so.$$ _build/libplan_pairprod.so
  fi
fi
if [ "$1" = "san" ]; then
  if [ ! -f _build/plan_pairprod_san ] || [ plan_pairprod.cpp -nt _build/plan_pairprod_san ] || [ $CSRC/plan.hpp -nt _build/plan_pairprod_san ]; then
    ${CXX:-c++} -O1 -g -std=c++17 -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -DPLAN_PAIRPROD_MAIN -I $CSRC plan_pairprod.cpp \
      -o _build/plan_pairprod_san.$$
    mv _build/plan_pairprod_san.$$ _build/plan_pairprod_san
  fi
fi
if [ "$1" = "emu" ]; then
  if [ ! -f _build/libpairprod.so ] || [ pairprod.cpp -nt _build/libpairprod.so ] || [ -n "$(find $CSRC -name '*.hpp' -newer _build/libpairprod.so)" ]; then
    hipcc -O2 -std=c++17 -x hip --offload-host-only -DBLS_TRACK_BOUNDS -g -rdynamic -fPIC -shared -I $CSRC pairprod.cpp -o _build/libpairprod.so.$$
    mv _build/libpairprod.so.$$ _build/libpairprod.so
  fi
fi
