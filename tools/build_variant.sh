#!/bin/bash
# Build an experimental copy of the product library with extra compile flags:
#   tools/build_variant.sh <suffix> [flags...]   -> ray_tracer_2_amd/librt2_mi355x_<suffix>.so
set -e
cd "$(dirname "$0")/.."
SUF=$1; shift
C=ray_tracer_2_amd/csrc
/opt/rocm/bin/hipcc -std=c++17 -O3 --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fno-slp-vectorize -fPIC -shared \
  -I include "$@" $C/rt_kernel.hip $C/rt_api.hip $C/rt_api_queries.hip $C/rt_api_frames.hip $C/rt_api_test.hip $C/rt_bvh_search.hip $C/rt_refit.hip $C/rt_denoise.hip $C/rt_temporal.hip $C/rt_vdenoise.hip $C/rt_adaptive.hip $C/rt_upsample.hip $C/rt_display.hip \
  $C/host/obj_loader.cpp $C/host/bvh.cpp $C/host/scene.cpp $C/host/scene_pack.cpp $C/host/launch_options.cpp $C/host/launch_state_entries.cpp $C/host/png_decode.cpp $C/host/scene_capi.cpp \
  $C/host/denoise.cpp $C/host/temporal.cpp $C/host/object_motions.cpp $C/host/vdenoise.cpp $C/host/adaptive.cpp $C/host/upsample.cpp $C/host/display.cpp $C/host/ray_tracer.cpp \
  -lz -ldl -o ray_tracer_2_amd/librt2_mi355x_$SUF.so   # (the sources: PRODUCT_SOURCES of ray_tracer_2_amd/build.py)
