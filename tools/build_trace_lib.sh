#!/bin/bash
# Diagnostic library: attn.hip with -DVBX_ATTN_TRACE and gemm.hip / gemm3.hip / gemm4.hip with -DVBX_GEMM_TRACE (per-workgroup start /
# prologue-end / loop-end / end timestamps), linked with the product's other objects -> voicebox-pytorch_amd/lib/libvbx_hip_trace.so.
# The object list is build.py's SOURCES, so the library has every symbol _lib.lib() binds.
# Used by tools/attn_timeline.py (VBX_LIB_PATH) and tools/native/gemm_trace.cpp.
set -e
cd "$(dirname "$0")/.."
L=voicebox-pytorch_amd/lib; C=voicebox-pytorch_amd/csrc
python voicebox-pytorch_amd/build.py > /dev/null  # the product's objects, current
F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-value"
declare -A TRACE=([attn.hip]=-DVBX_ATTN_TRACE [gemm.hip]=-DVBX_GEMM_TRACE [gemm3.hip]=-DVBX_GEMM_TRACE [gemm4.hip]=-DVBX_GEMM_TRACE)
OBJS=""
for s in $(python -c "import sys; sys.path.insert(0, 'voicebox-pytorch_amd'); import build; print(' '.join(build.SOURCES))"); do
  o=$L/${s%.hip}.o
  if [ -n "${TRACE[$s]}" ]; then
    o=$L/${s%.hip}_trace.o
    /opt/rocm/bin/hipcc $F ${TRACE[$s]} -c $C/$s -o $o &
  fi
  OBJS="$OBJS $o"
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $L/libvbx_hip_trace.so $OBJS
echo built $L/libvbx_hip_trace.so
