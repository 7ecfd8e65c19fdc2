#!/bin/bash
# Is the DEVICE code of the working tree the one of <commit>?  Compiles every .hip source of both trees to gfx950 assembly (device only) and
# diffs them ignoring comments, debug directives and the per-compilation cuid symbol.  Used to show that the kernels shipped at the end of a round
# are the ones its profiles were collected on (round 6: profiles of 6f0e33e).      usage: scripts/isa_same_as.sh <commit>
# The ordinal of a function within its file is dropped from the local labels (.LBB<n>_<m>, whose trailing loop comment goes as well, .Lfunc_begin<n>, .Lfunc_end<n>): removing a kernel
# renumbers every kernel behind it.  For a file that differs, the lines only one side has are counted and the symbols they define are named,
# so that "kernel X is gone, nothing else" can be read off the output.
C=${1:?commit}; T=$(mktemp -d)
mkdir -p $T/old $T/new
git archive $C cdmft-lanc-ed_amd/csrc include | tar -x -C $T/old
f() { grep -v "^\s*;\|\.file\|\.ident\|^\s*\.loc\|debug\|__hip_cuid" $1 | sed -E 's/BB[0-9]+_/BB_/g; s/^(\.LBB_[0-9]+:)\s*;.*/\1/; s/\.Lfunc_(begin|end)[0-9]+/.Lfunc_\1/g'; }
rc=0
for S in cdmft-lanc-ed_amd/csrc/*.hip; do
  B=$(basename $S .hip)
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC --cuda-device-only -S -o $T/new/$B.s $S 2>/dev/null
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC --cuda-device-only -S -o $T/old/$B.s $T/old/$S 2>/dev/null
  D=$(diff <(f $T/old/$B.s) <(f $T/new/$B.s))
  n=$(printf '%s' "$D" | grep -c '^[<>]')
  echo "$B: $n differing lines"
  if [ "$n" != "0" ]; then
    rc=1
    echo "  only in $C: $(printf '%s' "$D" | grep -c '^<') lines, defining: $(printf '%s' "$D" | sed -nE 's/^< ([A-Za-z_][A-Za-z0-9_$.]*):.*/\1/p' | grep -v '^\.L' | tr '\n' ' ')"
    echo "  only in the working tree: $(printf '%s' "$D" | grep -c '^>') lines, defining: $(printf '%s' "$D" | sed -nE 's/^> ([A-Za-z_][A-Za-z0-9_$.]*):.*/\1/p' | grep -v '^\.L' | tr '\n' ' ')"
  fi
done
rm -rf $T
exit $rc
