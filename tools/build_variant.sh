#!/bin/bash
# A second build of the library with extra compiler flags, for A/B runs in one call on one device (tools/abn.sh):
#   bash tools/build_variant.sh NAME "-DFLAG=1 ..."   ->  experiments/lib_NAME.so   (objects under /tmp/fthmc_NAME)
# The sources and the flags of each are the Makefile's own (fthmc_amd/csrc/Makefile: SRCS and the per-file rules).
#   PRELOAD= (empty) builds without kernel-argument preload, NOLICM= (empty) builds flow_small with MachineLICM
ROOT=$(cd "$(dirname "$0")/.." && pwd); NAME=$1; EXTRA=$2; D=/tmp/fthmc_$NAME; mkdir -p $D
OUT="$ROOT/experiments/lib_$NAME.so"
make -C "$ROOT/fthmc_amd/csrc" -j16 O="$D/" OUT="$OUT" EXTRA="$EXTRA" ${PRELOAD+PRELOAD="$PRELOAD"} ${NOLICM+NOLICM="$NOLICM"} "$OUT" && ls -la "$OUT"
