#!/bin/bash
# Builds the CPU execution of the threshold-signature recovery (csrc/fr.hpp, csrc/curve.hpp jac_mul_256_w4, csrc/recover.hpp, bounds tracked)
# with the numbers of csrc/plan.hpp recover_measure / recover_sizes_for, as a host library of its own (tests only):
# tests/test_recover_emu.py, tests/test_recover_plan.py.
set -e
cd "$(dirname "$0")"
mkdir -p _build
if [ ! -f _build/librecover.so ] || [ recover.cpp -nt _build/librecover.so ] || [ -n "$(find ../../nim-blscurve_amd/csrc -name '*.hpp' -newer _build/librecover.so)" ]; then
  hipcc -O2 -std=c++17 -x hip --offload-host-only -DBLS_TRACK_BOUNDS -g -rdynamic -fPIC -shared -I ../../nim-blscurve_amd/csrc recover.cpp -o _build/librecover.so.$$
  mv _build/librecover.so.$$ _build/librecover.so
fi
