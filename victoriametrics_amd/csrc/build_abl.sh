#!/bin/sh
# build_abl.sh — A/B ablation builds of the pipe kernel (perf work).
# Produces ../libvmgpu_<name>.so variants selectable via VMGPU_LIB.
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
    topk.hip hstat.hip aggrhist.hip aggrcv.hip -o ../libvmgpu_$name.so
}

build_one pipe_stage -DVMGPU_PIPE_ABL_STAGE &
build_one pipe_copy -DVMGPU_PIPE_ABL_STAGE -DVMGPU_PIPE_ABL_NO_SCAN &
build_one pipe_noeval -DVMGPU_PIPE_ABL_NO_EVAL &
build_one pipe_noscrape -DVMGPU_ABL_NO_SCRAPE &
wait
build_one pipe_mw8 -DVMGPU_PIPE_MINWAVES=8 &
build_one pipe_mw5 -DVMGPU_PIPE_MINWAVES=5 &
build_one pipe_mw6 -DVMGPU_PIPE_MINWAVES=6 &
build_one pipe_u2 -DVMGPU_PIPE_UNROLL=2 &
wait
# instruction-count cuts, one off at a time (all four are on by default),
# and all four off (the kernel before them, plus the ungated scalar
# bookkeeping and the NaN-value fixes described at the gates in vmgpu.hip)
build_one pipe_nosent -DVMGPU_PIPE_SENTINEL=0 &
build_one pipe_nohacc -DVMGPU_PIPE_HINT_ACC=0 &
build_one pipe_nodtfast -DVMGPU_PIPE_DT_FAST=0 &
build_one pipe_nopmaxskip -DVMGPU_PIPE_SKIP_PMAX=0 &
build_one pipe_nocuts -DVMGPU_PIPE_SENTINEL=0 -DVMGPU_PIPE_HINT_ACC=0 \
  -DVMGPU_PIPE_DT_FAST=0 -DVMGPU_PIPE_SKIP_PMAX=0 &
wait
# latency cuts of the series loop, one off at a time (both on by default),
# and both off
build_one pipe_nosdesc -DVMGPU_PIPE_SDESC=0 &
build_one pipe_noasmload -DVMGPU_PIPE_ASMLOAD=0 &
build_one pipe_noprefetch -DVMGPU_PIPE_SDESC=0 -DVMGPU_PIPE_ASMLOAD=0 &
wait
# cuts found by the instruction account (profiles/pipe_probe_time.md), one
# off at a time (all on by default)
build_one pipe_noprobe1 -DVMGPU_PIPE_PROBE1=0 &
build_one pipe_nodgonce -DVMGPU_PIPE_DG_ONCE=0 &
wait
echo "ablation libs built"
