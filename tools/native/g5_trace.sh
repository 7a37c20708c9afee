#!/bin/bash
# here: tools/native/g5_trace.sh build    on the GPU: tools/native/g5_trace.sh run [train 0|1] [geglu 0|1]
# build: gemm5.hip with -DVBX_G5_TRACE beside the product's other objects (build.py's SOURCES) -> lib/g5trace/libvbx_hip.so
cd "$(dirname "$0")/../.."
L=voicebox-pytorch_amd/lib; C=voicebox-pytorch_amd/csrc
if [ "$1" = build ]; then
  mkdir -p $L/g5trace
  python voicebox-pytorch_amd/build.py > /dev/null || exit 1  # the product's objects, current
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-value -fno-slp-vectorize -DVBX_G5_TRACE -c $C/gemm5.hip -o $L/g5trace/gemm5.o || exit 1
  OBJS=$(python -c "import sys; sys.path.insert(0, 'voicebox-pytorch_amd'); import build; print(' '.join('$L/' + ('g5trace/' if s == 'gemm5.hip' else '') + s[:-4] + '.o' for s in build.SOURCES))") || exit 1
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $L/g5trace/libvbx_hip.so $OBJS || exit 1
  /opt/rocm/bin/hipcc -O1 -std=c++17 tools/native/g5_trace.cpp -o tools/native/g5_trace -L$L/g5trace -lvbx_hip -Wl,-rpath,'$ORIGIN/../../voicebox-pytorch_amd/lib/g5trace' || exit 1
  echo built
else
  shift; tools/native/g5_trace "$@"
fi
