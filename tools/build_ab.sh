#!/bin/bash
# Builds a variant of the product library for tools/ab_libs.sh: build/ab/lib<NAME>.so = the kernels compiled with extra
# flags + the objects of the Makefile's librmgr-ssim-hip.so but ssim_kernels.o (make lib first).   usage: tools/build_ab.sh NAME [extra hipcc flags...]
set -e
cd "$(dirname "$0")/.."
NAME=$1; shift
mkdir -p build/ab
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Iinclude -Issim_amd/csrc -Wall -Wno-unused-function "$@" -c ssim_amd/csrc/ssim_kernels.hip -o build/ab/k_$NAME.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -Wl,--version-script=ssim_amd/csrc/exports.map -o build/ab/lib$NAME.so build/ab/k_$NAME.o \
    build/obj/ssim_probe.o build/obj/msssim_kernels.o build/obj/ssim16_kernels.o build/obj/ssimf_kernels.o build/obj/msssimf_kernels.o build/obj/ssimh_kernels.o build/obj/ssimw_kernels.o build/obj/ssim_hip_abi.o build/obj/ssim_samples_abi.o build/obj/ssim_comm.o build/obj/ssim_tune.o build/obj/ssim_dropin.o build/obj/ssim_context.o build/obj/ssim_openmp.o
echo "build/ab/lib$NAME.so"
