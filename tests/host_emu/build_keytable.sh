#!/bin/bash
# Builds the launch decisions of key admission (csrc/plan.hpp admit_survivors / admit_merge) and the CPU execution of the key-table decoder
# and of the record gather (csrc/deser.hpp deserialize_public_key, csrc/keytable.hpp, bounds tracked) as two host libraries of their own (tests
# only): tests/test_key_table_plan.py, tests/test_key_table_emu.py.  "main": plan_keytable.cpp as a stand-alone program with its own main
# (-DPLAN_KEYTABLE_MAIN) under the address and undefined-behaviour sanitizers, _build/plan_keytable_san - host code only, run on its own.
set -e
cd "$(dirname "$0")"
mkdir -p _build
if [ "$1" = "main" ]; then
  ${CXX:-c++} -O1 -g -std=c++17 -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=undefined -DPLAN_KEYTABLE_MAIN \
      -I ../../nim-blscurve_amd/csrc plan_keytable.cpp -o _build/plan_keytable_san
  exit 0
fi
if [ "$1" != "emu" ]; then
  if [ ! -f _build/libplan_keytable.so ] || [ plan_keytable.cpp -nt _build/libplan_keytable.so ] || [ ../../nim-blscurve_amd/csrc/plan.hpp -nt _build/libplan_keytable.so ]; then
    ${CXX:-c++} -O1 -std=c++17 -Wall -Wextra -Werror -fPIC -shared -I ../../nim-blscurve_amd/csrc plan_keytable.cpp -o _build/libplan_keytable.so.$$
    mv _build/libplan_keytable.so.$$ _build/libplan_keytable.so
  fi
fi
if [ "$1" != "plan" ]; then
  if [ ! -f _build/libkeytable.so ] || [ keytable.cpp -nt _build/libkeytable.so ] || [ -n "$(find ../../nim-blscurve_amd/csrc -name '*.hpp' -newer _build/libkeytable.so)" ]; then
    hipcc -O2 -std=c++17 -x hip --offload-host-only -DBLS_TRACK_BOUNDS -g -rdynamic -fPIC -shared -I ../../nim-blscurve_amd/csrc keytable.cpp -o _build/libkeytable.so.$$
    mv _build/libkeytable.so.$$ _build/libkeytable.so
  fi
fi
