#!/bin/bash
# Build liber_hip.so of a git revision as an A/B variant:  scripts/build_rev_variant.sh NAME REV [-DFLAG ...]
# The revision's own Makefile builds it, in a temporary copy of that revision: its source list and flags are whatever they were then.
set -e
R="$(cd "$(dirname "$0")/.." && pwd)"; name=$1; rev=$2; shift; shift
T=$(mktemp -d); trap 'rm -rf "$T"' EXIT
git -C "$R" archive "$rev" elasticreconstruction_amd/csrc include | tar -x -C "$T"
M="$T/elasticreconstruction_amd/csrc"
if [ $# -gt 0 ] && ! grep -q '^EXTRA' "$M/Makefile"; then
  echo "the Makefile of $rev has no EXTRA: it cannot take $*" >&2; exit 1
fi
# OUT= on the command line moves the library of every revision's Makefile; the objects stay in the temporary tree
mkdir -p "$T/out" "$R/elasticreconstruction_amd/_ab"
make -C "$M" -j16 lib OUT="$T/out" ${1:+EXTRA="$*"}
cp "$T/out/liber_hip.so" "$R/elasticreconstruction_amd/_ab/liber_hip_$name.so"
echo "built _ab/liber_hip_$name.so from $rev"
