#!/bin/bash
# Debug build of the register-resident interior-point kernel with per-phase cycle counters (-DALQP_G4_TIMING, fp64,
# (13,4) only) linked with the product objects into deq-mpc-corl_amd/csrc/build/libmi_alqp_g4timing.so;
# tools/g4_timing.py runs it on the GPU. Not part of the product build (the other objects come from csrc/build.sh).
set -euo pipefail
ALQP_ONLY=alqp_ipm_g4_f64 ALQP_OBJ_SUFFIX=_timing ALQP_OUT=build/libmi_alqp_g4timing.so \
  bash "$(dirname "$0")/../deq-mpc-corl_amd/csrc/build.sh" -DALQP_G4_TIMING '-DALQP_FOR_EACH_DIMS(X)=X(13,4)'
