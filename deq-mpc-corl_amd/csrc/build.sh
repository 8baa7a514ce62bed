#!/bin/bash
# Builds libmi_alqp.so for gfx950 (MI355X). hipcc cross-compiles without a GPU. One translation unit per kernel family,
# all compiled in parallel; arguments go to every compile.
#   ALQP_ONLY="obj ..."   recompile only these objects of the list below and relink (the others must exist from a full
#                         build), e.g. ALQP_ONLY="alqp_ipm_g4_f64 alqp_ipm_g4_f32" ./build.sh
#   ALQP_OBJ_SUFFIX=_x    with ALQP_ONLY: write those objects as build/<obj>_x.o, so that a debug compile leaves the
#                         product objects alone
#   ALQP_OUT=path         the library to link (default libmi_alqp.so)
set -euo pipefail
cd "$(dirname "$0")"
# -pragma-unroll-threshold: the panel loops of alqp_quad.hpp must be fully unrolled (register
# arrays need static indices); the default threshold silently leaves them rolled.
# -O2, not -O3: these kernels run one wavefront per SIMD and are bound by instruction count; -O3's extra transformations
# add instructions (A/B on one box: headline fp32 quad kernel 5.165 -> 5.269 M solves/s, resident interior-point fp64
# 372 k -> 382 k QP/s; nothing measured got slower)
FLAGS="--offload-arch=gfx950 -O2 -std=c++17 -fPIC -I../../include -mllvm -pragma-unroll-threshold=1000000"
# object, source, defines of that object: what libmi_alqp.so is made of
UNITS="
alqp_abi         alqp_abi.hip
alqp_team        alqp_team.hip
alqp_aux         alqp_aux.hip
alqp_quad_f32    alqp_quad.hip        -DALQP_QUAD_F32
alqp_quad_f64    alqp_quad.hip        -DALQP_QUAD_F64
alqp_team_dyn      alqp_team.hip      -DALQP_BWD_DYN_UNIT
alqp_team_xbox_step  alqp_team.hip    -DALQP_XBOX_STEP_UNIT
alqp_team_shdyn    alqp_team.hip      -DALQP_SHDYN_UNIT
alqp_team_gen_d    alqp_team.hip      -DALQP_GEN_UNIT=1
alqp_team_gen_x    alqp_team.hip      -DALQP_GEN_UNIT=2
alqp_team_gen_p    alqp_team.hip      -DALQP_GEN_UNIT=4
alqp_team_gen_dx   alqp_team.hip      -DALQP_GEN_UNIT=3
alqp_team_gen_dp   alqp_team.hip      -DALQP_GEN_UNIT=5
alqp_team_gen_xp   alqp_team.hip      -DALQP_GEN_UNIT=6
alqp_team_gen_dxp  alqp_team.hip      -DALQP_GEN_UNIT=7
alqp_team_rows_step  alqp_team.hip    -DALQP_ROWS_STEP_UNIT
alqp_team_dense_step       alqp_team.hip  -DALQP_DENSE_STEP_UNIT=0
alqp_team_dense_step_rows  alqp_team.hip  -DALQP_DENSE_STEP_UNIT=1
alqp_team_nl_x     alqp_team_nl.hip   -DALQP_NL_UNIT=2
alqp_team_nl_p     alqp_team_nl.hip   -DALQP_NL_UNIT=4
alqp_team_nl_xp    alqp_team_nl.hip   -DALQP_NL_UNIT=6
alqp_quad_dyn_f32  alqp_quad.hip      -DALQP_QUAD_F32 -DALQP_BWD_DYN_UNIT
alqp_quad_dyn_f64  alqp_quad.hip      -DALQP_QUAD_F64 -DALQP_BWD_DYN_UNIT
alqp_quad_shdyn_f32  alqp_quad.hip    -DALQP_QUAD_F32 -DALQP_SHDYN_UNIT
alqp_quad_shdyn_f64  alqp_quad.hip    -DALQP_QUAD_F64 -DALQP_SHDYN_UNIT
alqp_dyn_casadi  alqp_dyn_casadi.hip
alqp_ipm         alqp_ipm.hip
alqp_ipm_g4_f64  alqp_ipm_g4.hip      -DALQP_G4_F64
alqp_ipm_g4_f32  alqp_ipm_g4.hip      -DALQP_G4_F32
alqp_dyn_rigid   alqp_dyn_rigid.hip
"
ONLY="${ALQP_ONLY:-}"
for name in $ONLY; do
  grep -q "^$name " <<< "$UNITS" || { echo "build.sh: ALQP_ONLY names no object of the library: $name" >&2; exit 2; }
done
mkdir -p build
pids=()
objs=()
while read -r obj src defs; do
  [ -n "$obj" ] || continue
  o=build/$obj.o
  if [ -z "$ONLY" ] || [[ " $ONLY " == *" $obj "* ]]; then
    [ -z "$ONLY" ] || o=build/$obj${ALQP_OBJ_SUFFIX:-}.o
    hipcc $FLAGS $defs -c "$src" -o "$o" "$@" &
    pids+=($!)
  fi
  objs+=("$o")
done <<< "$UNITS"
for p in "${pids[@]}"; do wait "$p"; done
hipcc --offload-arch=gfx950 -shared -fPIC "${objs[@]}" -o "${ALQP_OUT:-libmi_alqp.so}"
