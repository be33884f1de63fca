#!/bin/bash
# Builds the product's launch plans (csrc/plan.hpp) as a host library of their own (tests only): a second's work, so that the GPU tests,
# which ask tests/util.py for the plan, do not wait for the emulation build of build.sh.
set -e
cd "$(dirname "$0")"
mkdir -p _build
if [ ! -f _build/libplan.so ] || [ plan.cpp -nt _build/libplan.so ] || [ ../../nim-blscurve_amd/csrc/plan.hpp -nt _build/libplan.so ]; then
  ${CXX:-c++} -O1 -std=c++17 -Wall -Wextra -Werror -fPIC -shared -I ../../nim-blscurve_amd/csrc plan.cpp -o _build/libplan.so.$$
  mv _build/libplan.so.$$ _build/libplan.so
fi
