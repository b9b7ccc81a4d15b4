#!/bin/bash
# builds the product library and the stamped diagnostic one (build/diag/libagbnp_hip_pstamps.so)
set -e
cd "$(dirname "$0")/.."
make -C openmm_agbnp_plugin_amd/csrc 2>&1 | grep -E "error|Error" && exit 1
mkdir -p build/diag
# (the same sources and flags as the product: csrc/Makefile holds the one list)
make -C openmm_agbnp_plugin_amd/csrc OUT=../../build/diag/libagbnp_hip_pstamps.so EXTRA_HIPFLAGS=-DAGBNP_PAIR_STAMPS BUILD_TAG=+pstamps lib 2>&1 | grep -E "error" && exit 1
echo built
