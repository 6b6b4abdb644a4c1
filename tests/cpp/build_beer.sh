#!/bin/bash
# Compile the C++ drop-in check of the Beer-Lambert solver (harp_amd::BeerLambert,
# include/harp_amd/beer_lambert.hpp) against the container's libtorch (ROCm build) and
# the in-tree libhdisort.so, as tests/cpp/build_rays.sh does for the ray radiances.
# Output: tests/cpp/beer_dropin
set -euo pipefail
HERE=$(cd "$(dirname "$0")" && pwd)
ROOT=$(cd "$HERE/../.." && pwd)
TORCH=$(python -c "import torch, os; print(os.path.dirname(torch.__file__))")
ABI=$(python -c "import torch; print(int(torch._C._GLIBCXX_USE_CXX11_ABI))")
/opt/rocm/bin/hipcc -O2 -std=c++17 -D_GLIBCXX_USE_CXX11_ABI=$ABI -D__HIP_PLATFORM_AMD__ -DUSE_ROCM \
  -I"$ROOT/include" -I"$TORCH/include" -I"$TORCH/include/torch/csrc/api/include" \
  "$HERE/beer_dropin.cpp" -o "$HERE/beer_dropin" \
  -L"$TORCH/lib" -Wl,-rpath,"$TORCH/lib" -ltorch -ltorch_cpu -lc10 -ltorch_hip -lc10_hip \
  -L"$ROOT/pyharp_amd" -Wl,-rpath,'$ORIGIN/../../pyharp_amd' -lhdisort -lz
