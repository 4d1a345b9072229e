#!/bin/bash
# Build a variant of libmarlnav.so into marl-nav_amd/lib/<name>.so, from the
# working tree with extra -D flags (the diagnostic macros of marlnav_debug.h),
# or from a git revision (HISTORY.md: where each removed A/B variant's code is):
#   scripts/build_variant.sh ref HEAD        # the committed kernels
#   scripts/build_variant.sh observed "" -DMARLNAV_AB=16384
# then: LIBS=marl-nav_amd/lib/ref.so bash scripts/cmd_ab.sh (on the GPU box)
set -eu
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
name=$1 rev=${2:-}
shift $(( $# >= 2 ? 2 : 1 ))
src="$ROOT"
tmp=""
if [ -n "$rev" ]; then
    tmp=$(mktemp -d)
    git -C "$ROOT" archive "$rev" marl-nav_amd/csrc include | tar -x -C "$tmp"
    src="$tmp"
fi
cd "$src/marl-nav_amd/csrc"
# every translation unit of the library (the rollout's needs the policy's)
/opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -std=c++17 -fPIC -shared -ffp-contract=off \
    -fno-slp-vectorize -mllvm -amdgpu-sched-strategy=max-ilp -mllvm -amdgpu-kernarg-preload-count=14 -Wno-pass-failed "$@" marlnav_*.hip -o "$ROOT/marl-nav_amd/lib/$name.so"
[ -n "$tmp" ] && rm -rf "$tmp"
echo "built marl-nav_amd/lib/$name.so"
