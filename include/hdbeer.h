/*
 * hdbeer.h -- C-ABI of the Beer-Lambert solver of libhdisort.so: the fluxes and the
 * emergent ray radiances of a purely absorbing, emitting atmosphere (HIP kernels for
 * gfx950, pyharp_amd/csrc/hd_beer.hip).
 *
 * The reference declares two solvers behind RTSolverImpl::forward(prop, bc, temf)
 * (src/rtsolver/rtsolver.hpp:34-64): Disort and BeerLambert, the latter with one option,
 * alpha, and the disabled body src/rtsolver/beer_lambert.cpp_ (TOA radiances `toa` along
 * the outgoing rays and their band sum `btoa`).  This header is that second solver.
 *
 * Same library, contexts (hd_context_create ...), return codes, status bits, hd_inputs
 * and hd_config as hdisort.h.  In hd_config, nstr is the order of the double-Gauss
 * quadrature the fluxes are summed with (even, 2..32), nmom is unused, nprop >= 1 (a
 * table of extinction alone, as hd_rfm_attenuate writes, goes straight in) and flags
 * may carry HD_FLAG_PLANCK.
 *
 * Physics.  Only prop[..][l][0], the layer's optical thickness, is read: EXTINCTION IS
 * TREATED AS ABSORPTION, whatever slot 1 (the single-scattering albedo) and the phase
 * moments hold.  At ssa = 0 the results are those of hd_solve / hd_solve_rays (the
 * discrete-ordinate equations decouple there); with ssa > 0 they are not.  The level
 * Planck values B come from temf and the wave bounds as in hd_solve (0 without
 * HD_FLAG_PLANCK), and the source is linear in optical depth inside a layer.  At slant
 * thickness x = dtau / |mu|, with E = 1 - exp(-x) and w1 = 1 - E / x:
 *   I_out = I_in (1 - E) + B_out w1 + B_in (E - w1)
 * (B_in on the side the ray enters).  Boundaries as hd_solve:
 *   top      I_down = fisot + temis B(ttemp)
 *   surface  I_up   = (1 - albedo) B(btemp) + albedo (F_down_diffuse + mu0 F0 e^(-tau/mu0)) / pi
 *   F_down_diffuse = 2 pi sum_i w_i mu_i I_down_i over the nstr/2 nodes of hd_quadrature.
 *
 * Status (int32 per solve, bits of hdisort.h): HD_STATUS_BAD_INPUT for a negative or
 * non-finite thickness, albedo outside [0,1], a beam (fbeam > 0) with umu0 outside
 * (0,1]; HD_STATUS_NONFINITE for a non-finite result.  status / stream / return codes /
 * ordering on the context / device restore as hd_solve: with status NULL the call is
 * synchronous and returns HD_ENUMERIC if any solve set an error bit.  Under stream
 * capture the calls never allocate: they return HD_EINVAL unless an identical call
 * outside capture sized the context's scratch first (hd_context_reserve does not).
 * hd_context_set_chunk bounds the solves per internal chunk (0: 262 144); scratch is one
 * chunk's Planck levels and, for a band sum without stored per-wave results, one chunk's
 * per-wave values.
 */
#ifndef HDBEER_H_
#define HDBEER_H_

#include "hdisort.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * flux [nwave][ncol][nlyr+1][2] f64 DEVICE, level 0 = surface (hd_solve's layout):
 *   [..][0] = 2 pi sum_i w_i mu_i I_up_i      [..][1] = direct + diffuse downward flux
 */
int hd_beer_flux(hd_context *ctx, const hd_config *cfg, const hd_inputs *in, double *flux,
                 int *status, void *stream);

/*
 * The fluxes and their weighted sum over the wave axis,
 *   band->bflux[c][lev][dir] = sum_w band->weight[w] flux[w][c][lev][dir],
 * formed as out = 0; out = fma(weight[w], flux[w], out) for w = 0, 1, ...: bitwise equal
 * to hd_band_sum (hdharp.h) of the stored fluxes at every chunk size, no atomics.  flux
 * may be NULL: per-wave fluxes are then not stored.
 */
int hd_beer_flux_band(hd_context *ctx, const hd_config *cfg, const hd_inputs *in,
                      const hd_band *band, double *flux, int *status, void *stream);

/*
 * Emergent radiance along nray directions: at the top level for umu > 0, at the
 * surface for umu < 0 (no azimuth dependence without scattering; the direct beam is not
 * part of a radiance).  Upward rays start from the surface expression above.
 *
 * alpha (the reference's one option, rays only): with alpha > 0, an upward ray whose
 * slant depth of the whole column x_s = sum(dtau) / umu lies in (0, 1000) gains
 *   (1 - albedo) B(btemp) alpha Gamma(alpha, x_s) x_s^(-alpha)
 * at the top: the emission from below the lower boundary when the source grows as
 * (tau / tau_s)^alpha there, int_{x_s}^inf (t/x_s)^alpha e^(-t) dt - e^(-x_s).  alpha > 0
 * with x_s = 0 sets HD_STATUS_BAD_INPUT.  alpha < 0 or non-finite is HD_EINVAL.
 *
 * A ray whose umu is 0, non-finite or above 1 in magnitude is NaN and sets
 * HD_STATUS_BAD_INPUT on the solves of its column (every solve for shared rays); the
 * column's other rays are unaffected.
 *
 * Band sum: with brad (and weight), brad[c][r] = sum_w weight[w] rad[w][c][r] in
 * hd_band_sum's sequence, as hd_beer_flux_band; rad may then be NULL.
 *
 * The struct shares its name with the function: refer to it as `struct hd_beer_rays`.
 */
struct hd_beer_rays {
  int nray;             /* rays per column, >= 1                               */
  int per_column;       /* 0: umu is [nray], shared; 1: [ncol][nray]           */
  const double *umu;    /* DEVICE polar cosines, nonzero, > 0 upward, |umu| <= 1 */
  double alpha;         /* >= 0; 0: off                                        */
  const double *weight; /* DEVICE [nwave] or NULL                              */
  double *brad;         /* DEVICE [ncol][nray], overwritten; needs weight      */
};

/* rad: DEVICE [nwave][ncol][nray], or NULL when rays->brad is given */
int hd_beer_rays(hd_context *ctx, const hd_config *cfg, const hd_inputs *in,
                 const struct hd_beer_rays *rays, double *rad, int *status, void *stream);

/*
 * Gradients: the exact adjoint of the three calls above (DESIGN.md section 3d,
 * "Gradients").  Given the cotangent of a call's result -- dL/d(result) for some scalar
 * L -- the _bwd calls return dL/d(input) for prop[..][l][0], temf and the boundary
 * conditions.  cfg and in are those of the forward call.  Not differentiated: the other
 * slots of prop (never read), umu, the band weights, alpha.
 *
 * The cotangent comes in one of two forms; exactly one of per_wave and band + weight is
 * set, anything else is HD_EINVAL.  m = 2 (nlyr+1) for the fluxes, nray for the rays.
 */
typedef struct hd_beer_cot {
  const double *per_wave; /* DEVICE [nwave][ncol][m]: of flux / rad                   */
  const double *band;     /* DEVICE [ncol][m]: of bflux / brad; the per-wave          */
  const double *weight;   /* DEVICE [nwave]     cotangent weight[w] band is not stored */
} hd_beer_cot;

/*
 * Optional DEVICE outputs, overwritten; NULL: not wanted.  gtau is dense (no nprop
 * stride).  gtemf sums over the waves of a column in ascending wave order, carried
 * through memory from chunk to chunk: bitwise the same at every chunk size, no atomics.
 * g_x needs in->x; gtemf, g_btemp and g_ttemp need HD_FLAG_PLANCK (HD_EINVAL otherwise;
 * g_temis is zero without it).  The temperature gradients use
 *   dB/dT = (4 B - K T^4 (g(v2) - g(v1))) / T,  g(v) = v^4 / (e^v - 1),  v_i = c2 nu_i / T
 * with the solver's own B: the derivative of the exact band integral, not of the PLKAVG
 * approximation.
 */
typedef struct hd_beer_grads {
  double *gtau;     /* [nwave][ncol][nlyr]  dL/d prop[..][l][0] */
  double *gtemf;    /* [ncol][nlyr+1]                           */
  double *g_albedo; /* [nwave][ncol] each                       */
  double *g_fbeam;
  double *g_umu0;
  double *g_btemp;
  double *g_ttemp;
  double *g_temis;
  double *g_fisot;
} hd_beer_grads;

/*
 * Status as the forward calls: a solve they flag HD_STATUS_BAD_INPUT gets the same bit
 * and NaN gradients (gtemf: NaN in that solve's column), a non-finite gradient sets
 * HD_STATUS_NONFINITE.  Context, stream, status and capture rules as hd_beer_flux;
 * scratch is one chunk's Planck levels, dL/dB per level and 2 (nstr/2) nlyr doubles per
 * solve between the adjoint's two sweeps (16 GB at most).
 */
int hd_beer_flux_bwd(hd_context *ctx, const hd_config *cfg, const hd_inputs *in,
                     const hd_beer_cot *cot, const hd_beer_grads *g, int *status, void *stream);

/* rays: nray, per_column, umu and alpha of the forward call (weight and brad are unused) */
int hd_beer_rays_bwd(hd_context *ctx, const hd_config *cfg, const hd_inputs *in,
                     const struct hd_beer_rays *rays, const hd_beer_cot *cot,
                     const hd_beer_grads *g, int *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HDBEER_H_ */
