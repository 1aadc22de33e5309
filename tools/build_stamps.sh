#!/bin/bash
# Diagnostic library with per-tick stamps in the persistent sweeps (-DARCVAE_PS_STAMPS): ab_libs/libarcvae_stamps.so
# (ab_libs/ is git-ignored and travels to the GPU box); used by tools/tick_stamps.py and tools/tick_stamps_layers.py
# through ARCVAE_HIP_LIB.  The object list is the Makefile's (make builds the other units), lstm.o replaced by the stamped one.
set -e
cd "$(dirname "$0")/../mlx-vae_amd/csrc"
mkdir -p ../../ab_libs build
make -s -j"${JOBS:-8}"
OBJS=$(make -s objs)
[ -n "$OBJS" ] || { echo "no OBJS in the Makefile" >&2; exit 1; }
/opt/rocm/bin/hipcc -I../../include -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -Wno-unused-function -DARCVAE_PS_STAMPS -c lstm.hip -o build/lstm_stamps.o
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o ../../ab_libs/libarcvae_stamps.so ${OBJS/build\/lstm.o/build\/lstm_stamps.o}
ls -la ../../ab_libs/libarcvae_stamps.so
