#!/bin/bash
# Build experimental variants of libldpc_mi355x.so into build_variants/<name>.so
# (every translation unit of csrc/Makefile's SRCS compiled with the variant's flags)
set -e
cd "$(dirname "$0")/.."
mkdir -p build_variants
build() {
  name=$1; shift
  rm -rf "build_variants/obj_$name"  # make tracks timestamps, not flags
  make -s -j4 -C iib_project_ldpc_codes_amd/csrc OBJDIR="$PWD/build_variants/obj_$name" OUT="$PWD/build_variants/$name.so" \
    EXTRA="$*" &
}
build v0
for spec in ${VARIANTS:-}; do name=${spec%%:*}; flags=${spec#*:}; build $name ${flags//,/ }; done
wait
ls -la build_variants
