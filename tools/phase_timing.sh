#!/bin/bash
# Debug build of the (13,4) team and fp32 quad kernels with per-phase cycle counters (-DALQP_PHASE_TIMING) into
# deq-mpc-corl_amd/csrc/build/libmi_alqp_timing.so; tools/phase_timing.py (quad) and tools/team_timing.py (team) run
# it on the GPU. Not part of the product build: the counters serialise loads and compute. Every other object comes
# from a product build (csrc/build.sh).
set -euo pipefail
DIMS="${1:-X(13, 4)}"
ALQP_ONLY="alqp_team alqp_quad_f32" ALQP_OBJ_SUFFIX=_timing ALQP_OUT=build/libmi_alqp_timing.so \
  bash "$(dirname "$0")/../deq-mpc-corl_amd/csrc/build.sh" -DALQP_PHASE_TIMING "-DALQP_FOR_EACH_DIMS(X)=$DIMS" ${EXTRA_FLAGS:-}
