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

// ---- gradients (hd_beer_flux_bwd, hd_beer_rays_bwd) ------------------------------------

// The cotangent of a chunk's results, m values per solve: per wave, or the band's with
// the weights (the kernels form weight[w] * gband themselves).
struct BeerCot {
  const double* per_wave;  // [nsolve][m] or null
  const double* band;      // [ncol][m]
  const double* weight;    // [nwave]
};

// One chunk of the adjoint.  Gradient outputs are null where not wanted.
struct BeerBwdArgs {
  const double* prop;
  const double* fbeam;
  const double* umu0;
  const double* albedo;
  const double* fisot;
  const double* planckv;  // [nlyr+3][nsc] or null
  BeerCot cot;            // of the fluxes, m = 2 (nlyr+1) (flux form)
  const double* seed;     // [nsc] dL/d(surface intensity) of the upward rays (surface form)
  double* sweep;          // [nlyr][2 NN][nsc] scratch between the two sweeps
  double* gb;             // [nlyr+3][nsc] dL/dB, planckv's layout; null without emission
  double* gtau;           // [nsolve][nlyr]
  double* g_albedo;       // [nsolve] each
  double* g_fbeam;
  double* g_umu0;
  double* g_fisot;
  int* status;
  int* anyerr;
  long s0;
  int nsc;
  int ncol;
  int nlyr;
  int nprop;
  double rmu[kBeerMaxNN];
  double wmu[kBeerMaxNN];
};

struct BeerRayBwdArgs {
  const double* prop;
  const double* albedo;
  const double* fisot;
  const double* planckv;
  const double* xsurf;  // [nsc] of the surface kernel
  const double* umu;
  BeerCot cot;          // of the radiances, m = nray
  double* seed;         // [nsc] out: sum of the upward rays' adjoints at the surface
  double* gb;
  double* gtau;
  double* g_albedo;
  double* g_fbeam;      // zeroed here; the surface form of the flux adjoint adds to them
  double* g_umu0;
  double* g_fisot;
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

// dL/dB of a chunk into the temperature gradients
struct BeerPlanckBwdArgs {
  const double* temf;
  const double* btemp;
  const double* ttemp;
  const double* temis;
  const double* wlo;
  const double* whi;
  const double* planckv;  // [nlyr+3][nsc]
  double* gb;             // [nlyr+3][nsc]: levels 0..nlyr become dL/dB dB/dT in place
  double* gtemf;          // [ncol][nlyr+1], carried from chunk to chunk
  double* g_btemp;        // [nsolve] each
  double* g_ttemp;
  double* g_temis;
  long s0;
  int nsc;
  int ncol;
  int nlyr;
};

// the adjoint of launch_beer_flux: every gradient written
hipError_t launch_beer_flux_bwd(int nn, const BeerBwdArgs& a, hipStream_t stream);
// the adjoint of launch_beer_surface from a.seed: added to what launch_beer_rays_bwd wrote
hipError_t launch_beer_surface_bwd(int nn, const BeerBwdArgs& a, hipStream_t stream);
hipError_t launch_beer_rays_bwd(const BeerRayBwdArgs& a, hipStream_t stream);
hipError_t launch_beer_planck_bwd(const BeerPlanckBwdArgs& a, hipStream_t stream);

}  // namespace hd
