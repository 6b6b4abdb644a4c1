#!/bin/bash
# Compile the C++ drop-in check of the pseudo-spherical ray radiances (harp_amd::DisortImpl::
# forward_rays / forward_rays_band with zd) against the container's libtorch (ROCm build)
# and the in-tree libhdisort.so, as tests/cpp/build_flx.sh does for the flux record.
# Output: tests/cpp/disort_rays_spher_dropin
set -euo pipefail
HERE=$(cd "$(dirname "$0")" && pwd)
ROOT=$(cd "$HERE/../.." && pwd)
TORCH=$(python -c "import torch, os; print(os.path.dirname(torch.__file__))")
ABI=$(python -c "import torch; print(int(torch._C._GLIBCXX_USE_CXX11_ABI))")
/opt/rocm/bin/hipcc -O2 -std=c++17 -D_GLIBCXX_USE_CXX11_ABI=$ABI -D__HIP_PLATFORM_AMD__ -DUSE_ROCM \
  -I"$ROOT/include" -I"$TORCH/include" -I"$TORCH/include/torch/csrc/api/include" \
  "$HERE/disort_rays_spher_dropin.cpp" -o "$HERE/disort_rays_spher_dropin" \
  -L"$TORCH/lib" -Wl,-rpath,"$TORCH/lib" -ltorch -ltorch_cpu -lc10 -ltorch_hip -lc10_hip \
  -L"$ROOT/pyharp_amd" -Wl,-rpath,'$ORIGIN/../../pyharp_amd' -lhdisort -lz
