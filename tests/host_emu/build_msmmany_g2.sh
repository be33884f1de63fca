#!/bin/bash
# Builds, for the G2 many-MSM call and the Jacobian-to-affine calls (tests only): the launch plan (csrc/plan.hpp msm_many_for with its G2 flag,
# to_affine_for) as a host library and as a sanitized program of its own; the CPU execution of the G2 tail's Horner walk (csrc/msmmany.hpp) and
# of the shared-inversion body (csrc/toaffine.hpp) as two more host libraries.  tests/test_msm_many_g2_plan.py, tests/test_msm_many_g2_emu.py,
# tests/test_to_affine_emu.py, tests/test_gpu_msm_many_g2.py, tests/test_gpu_to_affine.py.
set -e
cd "$(dirname "$0")"
mkdir -p _build
CSRC=../../nim-blscurve_amd/csrc
if [ "$1" = "plan" ] || [ -z "$1" ]; then
  if [ ! -f _build/libplan_msmmany_g2.so ] || [ plan_msmmany_g2.cpp -nt _build/libplan_msmmany_g2.so ] || [ $CSRC/plan.hpp -nt _build/libplan_msmmany_g2.so ]; then
    ${CXX:-c++} -O1 -std=c++17 -Wall -Wextra -Werror -fPIC -shared -I $CSRC plan_msmmany_g2.cpp -o _build/libplan_msmmany_g2.so.$$
    mv _build/libplan_msmmany_g2.so.$$ _build/libplan_msmmany_g2.so
  fi
fi
if [ "$1" = "san" ]; then
  if [ ! -f _build/plan_msmmany_g2_san ] || [ plan_msmmany_g2.cpp -nt _build/plan_msmmany_g2_san ] || [ $CSRC/plan.hpp -nt _build/plan_msmmany_g2_san ]; then
    ${CXX:-c++} -O1 -g -std=c++17 -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -DPLAN_MSMMANY_G2_MAIN -I $CSRC plan_msmmany_g2.cpp \
      -o _build/plan_msmmany_g2_san.$$
    mv _build/plan_msmmany_g2_san.$$ _build/plan_msmmany_g2_san
  fi
fi
for lib in msmmany_g2 toaffine; do
  if [ "$1" = "$lib" ] || [ -z "$1" ]; then
    if [ ! -f _build/lib$lib.so ] || [ $lib.cpp -nt _build/lib$lib.so ] || [ -n "$(find $CSRC -name '*.hpp' -newer _build/lib$lib.so)" ]; then
      hipcc -O2 -std=c++17 -x hip --offload-host-only -DBLS_TRACK_BOUNDS -g -rdynamic -fPIC -shared -I $CSRC $lib.cpp -o _build/lib$lib.so.$$
      mv _build/lib$lib.so.$$ _build/lib$lib.so
    fi
  fi
done
