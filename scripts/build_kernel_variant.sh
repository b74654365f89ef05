#!/bin/bash
# A variant library that differs from the product build only in the flags of the decoder kernels'
# files (KERNEL_SRCS in csrc/Makefile: the kernels and the launch plans that select among them):
#   scripts/build_kernel_variant.sh <name> [-DFLAG=...]  -> build_variants/<name>.so
# (links the product objects of the other translation units: run `make` first)
set -e
cd "$(dirname "$0")/.."
name=$1; shift
rm -rf "build_variants/obj_$name"  # make tracks timestamps, not flags: always recompile the variant objects
make -s -j8 -C iib_project_ldpc_codes_amd/csrc VARIANT_SRCS='$(KERNEL_SRCS)' VARIANT_OBJDIR="$PWD/build_variants/obj_$name" \
  OUT="$PWD/build_variants/$name.so" EXTRA="$*"
ls -la build_variants/$name.so
