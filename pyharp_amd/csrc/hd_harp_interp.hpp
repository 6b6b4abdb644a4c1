// hd_harp_interp.hpp -- the table lookup shared by the optics forwards (hd_harp.hip)
// and their adjoints (hd_harp_grad.hip): Numerical Recipes locate, interpn.h's index
// pair on one axis and its two-point formula.  lerp_ref keeps contraction off in its
// own body, so it rounds the same in whichever file includes it.
#pragma once
#include <hip/hip_runtime.h>

namespace hd {

// zero-offset j with xx[j] <= x < xx[j+1] for ascending or descending xx,
// -1 below / n-1 above the range (Numerical Recipes locate, as locate.h)
__device__ inline int locate_dev(const double* xx, double x, int n) {
  int jl = 0, ju = n + 1;  // unit offsets
  const bool ascnd = xx[n - 1] >= xx[0];
  while (ju - jl > 1) {
    const int jm = (ju + jl) >> 1;
    if ((x >= xx[jm - 1]) == ascnd) jl = jm;
    else ju = jm;
  }
  int j;
  if (x == xx[0]) j = 1;
  else if (x == xx[n - 1]) j = n;
  else j = jl;
  return j - 1;
}

// interpn.h's index pair and arithmetic on one axis
__device__ __forceinline__ void bracket(const double* ax, int n, double x, int& i1, int& i2) {
  i1 = locate_dev(ax, x, n);
  if (i1 == -1) {
    i1 = 0;
    i2 = 0;
  } else if (i1 == n - 1) {
    i2 = n - 1;
  } else {
    i2 = i1 + 1;
  }
}
__device__ __forceinline__ double lerp_ref(const double* ax, int i1, int i2, double x, double v1,
                                           double v2) {
#pragma clang fp contract(off)
  const double x1 = ax[i1], x2 = ax[i2];
  return x2 != x1 ? ((x - x1) * v2 + (x2 - x) * v1) / (x2 - x1) : (v1 + v2) / 2.;
}

}  // namespace hd
