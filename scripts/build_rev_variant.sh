#!/bin/bash
# A variant library whose csrc/sampler.hip is taken from git revision REV (the other translation
# units are this tree's product objects: run `make` first):
#   scripts/build_rev_variant.sh <rev> <name> [-DFLAG=...]  -> build_variants/<name>.so
set -e
cd "$(dirname "$0")/.."
rev=$1; name=$2; shift 2
mkdir -p build_variants/src_$name
git show "$rev:iib_project_ldpc_codes_amd/csrc/sampler.hip" > build_variants/src_$name/sampler.hip
rm -rf "build_variants/obj_$name"  # make tracks timestamps, not flags: always recompile the variant objects
make -s -C iib_project_ldpc_codes_amd/csrc VARIANT_SRCS=sampler.hip VARIANT_SRCDIR="$PWD/build_variants/src_$name/" \
  VARIANT_OBJDIR="$PWD/build_variants/obj_$name" OUT="$PWD/build_variants/$name.so" EXTRA="$*"
ls -la build_variants/$name.so
