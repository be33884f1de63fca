#!/bin/bash
# Builds the CPU execution of popVerify's arithmetic (csrc/deser.hpp g1_compress, csrc/h2c.hpp's 48-byte prepared hash_to_field, the PoP
# hash-map body; bounds tracked) as a host library of its own (tests only): tests/test_pop_emu.py.
set -e
cd "$(dirname "$0")"
mkdir -p _build
if [ ! -f _build/libpop.so ] || [ pop.cpp -nt _build/libpop.so ] || [ -n "$(find ../../nim-blscurve_amd/csrc -name '*.hpp' -newer _build/libpop.so)" ]; then
  hipcc -O2 -std=c++17 -x hip --offload-host-only -DBLS_TRACK_BOUNDS -g -rdynamic -fPIC -shared -I ../../nim-blscurve_amd/csrc pop.cpp -o _build/libpop.so.$$
  mv _build/libpop.so.$$ _build/libpop.so
fi
