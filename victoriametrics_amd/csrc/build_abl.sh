#!/bin/sh
# build_abl.sh — phase-probe builds of the pipe kernel (perf work): each
# variant drops or pins one phase to measure its floor.
# Produces ../libvmgpu_<name>.so variants selectable via VMGPU_LIB.
# The merged cuts of the pipe kernel (sentinel slab, accumulated hint, fast
# dt/1e3, clamp shortcut, scalar descriptors, uncounted staged loads, count
# probe, once-per-wave window/step) are no longer switchable here; to A/B one,
# build commit 248705b, where all eight of their gates exist.
set -e
cd "$(dirname "$0")"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC"
mkdir -p .abl

# the same sources as build.sh: the library exports entry points from every
# one of them, and all but binop, transform and aggrcol use vmgpu.hip's
# context
build_one() {
  name=$1
  shift
  hipcc $FLAGS "$@" -shared vmgpu.hip decode.hip binop.hip transform.hip aggrcol.hip hot.hip cvot.hip \
    topk.hip hstat.hip aggrhist.hip aggrcv.hip aggrtopk.hip -o ../libvmgpu_$name.so
}

build_one pipe_stage -DVMGPU_PIPE_ABL_STAGE &
build_one pipe_copy -DVMGPU_PIPE_ABL_STAGE -DVMGPU_PIPE_ABL_NO_SCAN &
build_one pipe_noeval -DVMGPU_PIPE_ABL_NO_EVAL &
build_one pipe_noscrape -DVMGPU_ABL_NO_SCRAPE &
wait
build_one pipe_mw8 -DVMGPU_PIPE_MINWAVES=8 &
build_one pipe_mw5 -DVMGPU_PIPE_MINWAVES=5 &
build_one pipe_mw6 -DVMGPU_PIPE_MINWAVES=6 &
wait
echo "ablation libs built"
