#!/bin/bash
# Development: build librsx_hip from the sources of a git ref -> tools/_dev/librsx_<name>.so (A/B against the working tree)
#   tools/build_ref.sh <name> <git-ref> [-DFOO ...]
set -e
cd "$(dirname "$0")/.."
name=$1; ref=$2; shift 2
src=tools/_dev/src_$name
rm -rf $src; mkdir -p $src/csrc $src/include
for f in $(git ls-tree --name-only $ref rsoccer_amd/csrc/); do git show $ref:$f > $src/csrc/$(basename $f); done
git show $ref:include/rsx.h > $src/include/rsx.h
C="--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -Wno-unused-value -mllvm -amdgpu-kernarg-preload-count=12 -I$src/include -I$src/csrc $* -c"
# the units of the ref and their flags: the ref's own __graft_entry__.HIP_UNITS (no second copy of that table here)
git show $ref:__graft_entry__.py > $src/units_of_ref.py
objs=
while read -r unit flags; do
    hipcc $C $flags -o /tmp/_rsx_${name}_${unit%.hip}.o $src/csrc/$unit &
    objs="$objs /tmp/_rsx_${name}_${unit%.hip}.o"
done < <(python -c "import sys; sys.path.insert(0, '$src'); import units_of_ref as g; [print(u, *f) for u, f in g.HIP_UNITS]")
wait
hipcc --offload-arch=gfx950 -fPIC -shared -o tools/_dev/librsx_${name}.so $objs
echo built tools/_dev/librsx_${name}.so
