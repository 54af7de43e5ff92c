#!/bin/bash
# build a variant of libpwpp_hip.so for an A/B run: tools/ab_build.sh <name> [-DFLAG=...]  ->  ab/<name>.so  (PWPP_LIB_PATH selects it)
# The sources are the Makefile's (SRCS), taken from PWPP_AB_CSRC instead of csrc/ when that is set: a checkout of another commit's
# csrc directory, e.g. the parent's.  Any compiler failure fails the script.
set -euo pipefail
name=$1; shift
cd "$(dirname "$0")/../patchwork-plusplus_amd"
csrc=${PWPP_AB_CSRC:-csrc}
srcs=$(make -s print-srcs | sed "s#csrc/#$csrc/#g")
mkdir -p ../ab
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -fvisibility=hidden -Wall -Wno-unused-function "$@" -shared -Wl,--version-script=$csrc/pwpp.map -o ../ab/$name.so $srcs
ls -la ../ab/$name.so
