#!/bin/bash
# Builds the staging layout of the grouped calls' host inputs (csrc/plan.hpp pack_for) as a host library of its own (tests only):
# tests/test_pack_plan.py.
set -e
cd "$(dirname "$0")"
mkdir -p _build
if [ ! -f _build/libplan_pack.so ] || [ plan_pack.cpp -nt _build/libplan_pack.so ] || [ ../../nim-blscurve_amd/csrc/plan.hpp -nt _build/libplan_pack.so ]; then
  ${CXX:-c++} -O1 -std=c++17 -Wall -Wextra -Werror -fPIC -shared -I ../../nim-blscurve_amd/csrc plan_pack.cpp -o _build/libplan_pack.so.$$
  mv _build/libplan_pack.so.$$ _build/libplan_pack.so
fi
