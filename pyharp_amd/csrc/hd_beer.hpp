// hd_beer.hpp -- argument blocks and launchers of the Beer-Lambert solver
// (hd_beer.hip; C-ABI: include/hdbeer.h, entry points in hd_api.cpp).
#pragma once

#include <hip/hip_runtime.h>

namespace hd {

constexpr int kBeerMaxNN = 16;  // nstr <= 32

// One chunk of consecutive solves s0 .. s0+nsc-1 (s = wave * ncol + col).
struct BeerArgs {
  const double* prop;     // [nsolve][nlyr][nprop], slot 0 = layer thickness, layer 0 = bottom
  const double* fbeam;    // [nsolve] or null
  const double* umu0;
  const double* albedo;
  const double* fisot;
  const double* planckv;  // [nlyr+3][nsc] of hd_planck_kernel, or null (no emission)
  double* flux;           // the chunk's fluxes [nsc][nlyr+1][2] (flux kernel)
  double* xsurf;          // [nsc] upward intensity leaving the surface (surface kernel)
  int* status;            // [nsolve]
  int* anyerr;
  long s0;
  int nsc;
  int nlyr;
  int nprop;
  double rmu[kBeerMaxNN];  // 1 / mu_i of the double-Gauss nodes
  double wmu[kBeerMaxNN];  // w_i mu_i
};

struct BeerRayArgs {
  const double* prop;
  const double* albedo;   // alpha term: (1 - albedo) B(btemp)
  const double* fisot;
  const double* planckv;  // [nlyr+3][nsc] or null
  const double* xsurf;    // [nsc] of the surface kernel
  const double* umu;      // [nray] or [ncol][nray]
  double* rad;            // the chunk's radiances [nsc][nray]
  int* status;
  int* anyerr;
  long s0;
  int nsc;
  int ncol;
  int nlyr;
  int nprop;
  int nray;
  int per_column;
  double alpha;
};

// fluxes of a chunk at every level (down pass, surface, up pass)
hipError_t launch_beer_flux(int nn, const BeerArgs& a, hipStream_t stream);
// the down pass alone: the upward intensity leaving the surface into a.xsurf
hipError_t launch_beer_surface(int nn, const BeerArgs& a, hipStream_t stream);
hipError_t launch_beer_rays(const BeerRayArgs& a, hipStream_t stream);
// out[c][e] = fma(weight[w], x[(w * ncol + c - s0)][e], out[c][e]) for the waves w of the
// chunk in ascending order, e < m: hd_band_sum's sequence continued chunk by chunk
hipError_t launch_beer_band_acc(const double* x, const double* weight, double* out, long s0,
                                int nsc, int ncol, long m, hipStream_t stream);

}  // namespace hd
