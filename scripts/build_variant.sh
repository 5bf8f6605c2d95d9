#!/bin/bash
# Build a variant of liber_hip.so for A/B measurements:  scripts/build_variant.sh NAME [-DFLAG ...]
# -> elasticreconstruction_amd/_ab/liber_hip_NAME.so  (select with ER_HIP_LIB=<path>)
# The csrc Makefile builds it (its source list, its flags, EXTRA = the flags given here) into a directory of its own.
# FLAGS_PRE / FLAGS_INT (environment): extra flags for er_tsdf_pre.hip (k_reproject_scatter, k_prepare) / er_tsdf_int.hip (k_integrate) only;
# unset = the Makefile's defaults for those two files, "none" = no extra flags.
set -e
R="$(cd "$(dirname "$0")/.." && pwd)"; name=$1; shift
AB="$R/elasticreconstruction_amd/_ab"
per_file=()
[ -n "${FLAGS_PRE+x}" ] && { [ "$FLAGS_PRE" = none ] && FLAGS_PRE=""; per_file+=("FLAGS_er_tsdf_pre.hip=$FLAGS_PRE"); }
[ -n "${FLAGS_INT+x}" ] && { [ "$FLAGS_INT" = none ] && FLAGS_INT=""; per_file+=("FLAGS_er_tsdf_int.hip=$FLAGS_INT"); }
make -C "$R/elasticreconstruction_amd/csrc" -j16 lib BUILD="$AB/_build_$name" LIB="$AB/liber_hip_$name.so" EXTRA="$*" "${per_file[@]}"
rm -rf "$AB/_build_$name"
echo "built $AB/liber_hip_$name.so"
