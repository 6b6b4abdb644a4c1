// hd_beer.hip -- gfx950 kernels of the Beer-Lambert solver (include/hdbeer.h): the
// radiative transfer of a purely absorbing, emitting atmosphere.  Without scattering the
// discrete-ordinate equations decouple: every stream, and every outgoing ray, is one
// integral along its own path with a thermal source linear in optical depth per layer.
// No eigenproblem, no boundary system, FP64 throughout.
//
//   hd_beer_flux_kernel<NN, false>  one lane per solve: the nstr/2 downward intensities
//                        from the top boundary to the surface (each level's downward flux
//                        as it is passed), the Lambertian surface, the nstr/2 upward
//                        intensities back to the top (each level's upward flux)
//   hd_beer_flux_team_kernel<T>     the same fluxes, to the bit, for a small batch: the
//                        streams of a solve in T neighbouring lanes
//   hd_beer_flux_kernel<NN, true>   the down pass alone: the upward intensity leaving
//                        the surface, which every upward ray starts from
//   hd_beer_ray_kernel   one lane per (solve, ray): the emergent radiance at the top
//                        (umu > 0) or at the surface (umu < 0)
//   hd_beer_band_acc_kernel  out = fma(weight[w], x[w], out) over a chunk's waves, a lane
//                        per output; hd_beer_band_acc_staged_kernel: the same chains out
//                        of LDS for one column with many waves
//   hd_beer_flux_bwd_kernel<NN, SURF>, hd_beer_ray_bwd_kernel, hd_beer_planck_bwd_kernel,
//   hd_beer_temf_acc_kernel  the gradients: the exact adjoint of the kernels above
//                        (hd_beer_flux_bwd / hd_beer_rays_bwd), described where they stand
//
// Layer transfer at slant thickness x = dtau / |mu|, with E = 1 - exp(-x) and
// w1 = 1 - E / x (B_in on the side the ray enters, B_out where it leaves):
//   I_out = I_in (1 - E) + B_out w1 + B_in (E - w1)
//
// Memory.  prop is [solve][layer][nprop] and only slot 0 is
// read.  In the flux kernel a lane owns a solve, so a lane-per-solve read would stride
// nlyr * nprop * 8 bytes: instead a wave stages a [64 solves][16 layers] tile through
// LDS with consecutive lanes along the layer axis (stride nprop * 8 bytes: every byte of
// a fetched line that holds a thickness is used; at nprop = 1 the read is contiguous),
// and writes the tile's level fluxes back the same way (stride 16 bytes, the other
// direction's slot in between).  Rows are padded to 17 doubles: a lane reading its own
// row with ds_read_b64 then hits a different bank pair in each half-wave.
// In the ray kernel the lanes of a solve's rays read the same address (one fetch,
// broadcast) and walk the layers together.
#include <hip/hip_runtime.h>

#include <cmath>

#include "hd_beer.hpp"
#include "hd_device.hpp"
#include "hd_kernels.hpp"  // dispatch_nn

#pragma clang fp contract(off)

namespace hd {

namespace {

constexpr int kTL = 16;  // layers per staged tile

// Transfer coefficients of one layer at slant thickness x >= 0:
//   t = exp(-x),  w1 = 1 - E / x,  cin = E - w1,  E = 1 - t   (all three >= 0).
// 1 - E / x cancels for small x (relative error eps / (x / 2)), so below x = 1/8 the
// series w1 = sum_{k >= 1} (-1)^(k+1) x^k / (k+1)! is summed instead and E = x (1 - w1)
// follows exactly from the definition: no transcendental call there, and x = 0 gives
// t = 1, w1 = cin = 0 exactly.  Eleven terms: the first one dropped is x^12 / 13! <
// 1.2e-21 at x = 1/8, below 2^-53 of the leading term x / 2.  At and above 1/8
// E = 1 - exp(-x) >= 0.117 carries an absolute error of 1.6e-16 and w1 >= 0.06 a
// relative one below 3e-14.
__device__ __forceinline__ void beer_coef(double x, double& t, double& cin, double& w1) {
  double e;
  if (x < 0.125) {
    double p = 1.0 / 479001600.0;
    p = fma(-x, p, 1.0 / 39916800.0);
    p = fma(-x, p, 1.0 / 3628800.0);
    p = fma(-x, p, 1.0 / 362880.0);
    p = fma(-x, p, 1.0 / 40320.0);
    p = fma(-x, p, 1.0 / 5040.0);
    p = fma(-x, p, 1.0 / 720.0);
    p = fma(-x, p, 1.0 / 120.0);
    p = fma(-x, p, 1.0 / 24.0);
    p = fma(-x, p, 1.0 / 6.0);
    p = fma(-x, p, 0.5);
    w1 = x * p;
    e = fma(-x, w1, x);
    t = 1.0 - e;
  } else {
    t = exp(-x);
    e = 1.0 - t;
    w1 = 1.0 - e / x;
  }
  cin = e - w1;
}

__device__ __forceinline__ double beer_step(double i_in, double x, double b_in, double b_out) {
  double t, cin, w1;
  beer_coef(x, t, cin, w1);
  return fma(i_in, t, fma(b_out, w1, b_in * cin));
}

__device__ __forceinline__ bool bad_tau(double d) { return !(d >= 0.0) || !(d <= 1.7e308); }

// beer_coef and w1p = dw1/dx = ((1 - w1) - t) / x, which cancels at small x as w1 does:
// below the same x = 1/8 the series w1p = sum_{k >= 1} (-1)^(k+1) k x^(k-1) / (k+1)! is
// summed (x = 0 gives 1/2 exactly).  Eleven terms: the first one dropped is
// 12 x^11 / 13! < 2.3e-19 at x = 1/8, below 2^-53 of the leading term 1/2.  At and above
// 1/8 the difference (1 - w1) - t >= 0.057 carries an absolute error of 3e-16.
__device__ __forceinline__ void beer_coef_d(double x, double& t, double& cin, double& w1,
                                            double& w1p) {
  beer_coef(x, t, cin, w1);
  if (x < 0.125) {
    double p = 1.0 / 43545600.0;  // k / (k+1)!, k = 11 .. 1
    p = fma(-x, p, 1.0 / 3991680.0);
    p = fma(-x, p, 1.0 / 403200.0);
    p = fma(-x, p, 1.0 / 45360.0);
    p = fma(-x, p, 1.0 / 5760.0);
    p = fma(-x, p, 1.0 / 840.0);
    p = fma(-x, p, 1.0 / 144.0);
    p = fma(-x, p, 1.0 / 30.0);
    p = fma(-x, p, 0.125);
    p = fma(-x, p, 1.0 / 3.0);
    w1p = fma(-x, p, 0.5);
  } else {
    w1p = ((1.0 - w1) - t) / x;
  }
}

// d I_out / d dtau of one layer step at slant thickness x = dtau rmu
__device__ __forceinline__ double beer_dstep(double i_in, double rmu, double b_in, double b_out,
                                             double t, double w1p) {
  return rmu * (fma(b_out, w1p, (t - w1p) * b_in) - t * i_in);
}

// The temperature derivative of hd_planck_kernel's band value b = plkavg(wlo, whi, t), by
// Leibniz' rule on the exact band integral:
//   dB/dT = (4 B - K T^4 (g(v2) - g(v1))) / T,   g(v) = v^4 / (e^v - 1),  v_i = c2 nu_i / T
// (plkavg's constants).  Not the derivative of the PLKAVG approximation, whose branches
// and Simpson stop are not smooth in T (Gradients).
__device__ __forceinline__ double planck_g(double v) {
  return v > 0.0 ? v * v * v * v / expm1(v) : 0.0;
}
__device__ double beer_dplanck(double wlo, double whi, double t, double b) {
  if (!(t >= 0.0)) return __builtin_nan("");
  if (t < 1.0e-4) return 0.0;
  const double k = 5.67032e-8 / kPi * (15.0 / (kPi * kPi * kPi * kPi));
  const double c2 = 1.438786;
  const double t4 = t * t * t * t;
  return (4.0 * b - k * t4 * (planck_g(c2 * whi / t) - planck_g(c2 * wlo / t))) / t;
}

// alpha Gamma(alpha, x) x^-alpha for alpha > 0, 0 < x < 1000: the emission from below
// the lower boundary when the source grows as (tau / tau_s)^alpha there,
//   int_x^inf (t / x)^alpha e^-t dt - e^-x.
// The usual split of the incomplete gamma function: the series of the lower function
// below x = alpha + 1, the continued fraction of the upper one (modified Lentz) above;
// x^-alpha is taken into both so that neither form overflows.
__device__ double beer_alpha_term(double a, double x) {
  if (x < a + 1.0) {
    double ap = a, del = 1.0 / a, sum = del;
    for (int n = 0; n < 500; ++n) {
      ap += 1.0;
      del *= x / ap;
      sum += del;
      if (fabs(del) < fabs(sum) * 1.0e-17) break;
    }
    return a * (tgamma(a) * pow(x, -a) - exp(-x) * sum);
  }
  const double tiny = 1.0e-300;
  double b = x + 1.0 - a, c = 1.0 / tiny, d = 1.0 / b, h = d;
  for (int i = 1; i <= 500; ++i) {
    const double an = -(double)i * ((double)i - a);
    b += 2.0;
    d = an * d + b;
    if (fabs(d) < tiny) d = tiny;
    c = b + an / c;
    if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = d * c;
    h *= del;
    if (fabs(del - 1.0) < 1.0e-16) break;
  }
  return a * exp(-x) * h;
}

__device__ __forceinline__ void beer_flag(int* status, int* anyerr, long s, int st) {
  if (st) {
    atomicOr(&status[s], st);
    if (st & 0x0F) atomicOr(anyerr, 1);
  }
}

}  // namespace

// ============================================================================
// fluxes (SURF = false) / the surface's upward intensity (SURF = true)
// ============================================================================
template <int NN, bool SURF>
__global__ __launch_bounds__(64) void hd_beer_flux_kernel(BeerArgs A) {
  __shared__ double tile[64][kTL + 1];
  // above nstr 16 the flux weights come through LDS (every lane reads one address): in
  // SGPRs beside the 2 NN of rmu and the constants of exp() they overflow the scalar file
  __shared__ double q_wmu[NN];
  const int lane = threadIdx.x;
  if constexpr (NN > 8) {
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < NN; ++i) q_wmu[i] = A.wmu[i];
    }
    __syncthreads();
  }
  const long sb = (long)blockIdx.x * 64;  // the block's first solve within the chunk
  const int nv = (int)(A.nsc - sb < 64 ? A.nsc - sb : 64);
  const bool live = lane < nv;
  const long sl = sb + (live ? lane : 0);  // lanes past the chunk shadow the first one
  const long s = A.s0 + sl;
  const int L = A.nlyr, nlev = L + 1;
  const size_t nsc = (size_t)A.nsc;
  const bool planck = A.planckv != nullptr;
  const double bsurf = planck ? A.planckv[(size_t)(L + 1) * nsc + sl] : 0.0;
  if (SURF && !A.albedo) {  // a black surface: nothing comes back from the down pass
    if (live) A.xsurf[sl] = bsurf;
    return;
  }
  int st = 0;
  const double fb = A.fbeam ? A.fbeam[s] : 0.0;
  const double mu0 = A.umu0 ? A.umu0[s] : 1.0;
  bool beam = fb > 0.0;
  if (beam && !(mu0 > 0.0 && mu0 <= 1.0)) {
    st |= kStBadInput;
    beam = false;
  }
  const double alb = A.albedo ? A.albedo[s] : 0.0;
  if (!(alb >= 0.0 && alb <= 1.0)) st |= kStBadInput;
  const double f0 = beam ? mu0 * fb : 0.0;

  // [64 solves][nl layers] of prop slot 0 from layer t0 on: lanes along the layer axis
  auto stage_in = [&](int t0, int nl) {
#pragma unroll 2
    for (int idx = lane; idx < 64 * kTL; idx += 64) {
      const int r = idx / kTL, l = idx % kTL;
      if (r < nv && l < nl)
        tile[r][l] = A.prop[((size_t)(A.s0 + sb + r) * L + t0 + l) * A.nprop];
    }
  };
  // the tile's level fluxes: level = t0 + l + off, slot dir
  auto stage_out = [&](int t0, int nl, int off, int dir) {
#pragma unroll 2
    for (int idx = lane; idx < 64 * kTL; idx += 64) {
      const int r = idx / kTL, l = idx % kTL;
      if (r < nv && l < nl)
        A.flux[((size_t)(sb + r) * nlev + t0 + l + off) * 2 + dir] = tile[r][l];
    }
  };
  auto hemi_flux = [&](const double (&I)[NN]) {
    double f = 0.0;
#pragma unroll
    for (int i = 0; i < NN; ++i) {
      if constexpr (NN > 8) f = fma(q_wmu[i], I[i], f);
      else f = fma(A.wmu[i], I[i], f);
    }
    return 2.0 * kPi * f;
  };

  // ---- down: top boundary -> surface ----------------------------------------------
  double I[NN];
  {
    const double top = (A.fisot ? A.fisot[s] : 0.0) + (planck ? A.planckv[(size_t)(L + 2) * nsc + sl] : 0.0);
#pragma unroll
    for (int i = 0; i < NN; ++i) I[i] = top;
  }
  double fdn = hemi_flux(I) + f0;
  double chk = fdn;
  if (!SURF && live) A.flux[((size_t)sl * nlev + L) * 2 + 1] = fdn;
  double tauc = 0.0;
  double bin = planck ? A.planckv[(size_t)L * nsc + sl] : 0.0;  // the side the rays enter
  for (int t0 = (L - 1) / kTL * kTL; t0 >= 0; t0 -= kTL) {
    const int nl = L - t0 < kTL ? L - t0 : kTL;
    __syncthreads();
    stage_in(t0, nl);
    __syncthreads();
    for (int l = nl - 1; l >= 0; --l) {
      const double d = tile[lane][l];
      if (bad_tau(d)) st |= kStBadInput;
      const double bout = planck ? A.planckv[(size_t)(t0 + l) * nsc + sl] : 0.0;
#pragma unroll
      for (int i = 0; i < NN; ++i) I[i] = beer_step(I[i], d * A.rmu[i], bin, bout);
      bin = bout;
      tauc += d;
      fdn = hemi_flux(I) + (beam ? f0 * exp(-tauc / mu0) : 0.0);
      chk += fdn;
      if (!SURF) tile[lane][l] = fdn;
    }
    if (!SURF) {
      __syncthreads();
      stage_out(t0, nl, 0, 1);
    }
  }
  // ---- Lambertian surface ---------------------------------------------------------
  const double isurf = (1.0 - alb) * bsurf + alb * fdn / kPi;
  if (SURF) {
    if (!isfinite(isurf)) st |= kStNonFinite;
    if (live) {
      A.xsurf[sl] = isurf;
      beer_flag(A.status, A.anyerr, s, st);
    }
    return;
  }
  // ---- up: surface -> top ---------------------------------------------------------
#pragma unroll
  for (int i = 0; i < NN; ++i) I[i] = isurf;
  double fup = hemi_flux(I);
  chk += fup;
  if (live) A.flux[(size_t)sl * nlev * 2] = fup;
  bin = planck ? A.planckv[sl] : 0.0;
  for (int t0 = 0; t0 < L; t0 += kTL) {
    const int nl = L - t0 < kTL ? L - t0 : kTL;
    __syncthreads();
    stage_in(t0, nl);
    __syncthreads();
    for (int l = 0; l < nl; ++l) {
      const double d = tile[lane][l];
      const double bout = planck ? A.planckv[(size_t)(t0 + l + 1) * nsc + sl] : 0.0;
#pragma unroll
      for (int i = 0; i < NN; ++i) I[i] = beer_step(I[i], d * A.rmu[i], bin, bout);
      bin = bout;
      fup = hemi_flux(I);
      chk += fup;
      tile[lane][l] = fup;
    }
    __syncthreads();
    stage_out(t0, nl, 1, 0);
  }
  if (!isfinite(chk)) st |= kStNonFinite;
  if (live) beer_flag(A.status, A.anyerr, s, st);
}

// ============================================================================
// fluxes of a small batch: T lanes per solve, one stream each
// ============================================================================
// A batch that leaves most of the chip idle (C1: 16 solves) is one wave walking every
// layer's NN streams in turn: 97 us at nstr 8, nlyr 40.  Here the streams of a solve sit in
// T = 2, 4, 8 or 16 >= NN neighbouring lanes; every lane gathers the team's intensities by
// shuffles and forms the level flux with the one-lane kernel's fma sequence, so the two
// kernels return the same bits.
template <int T>
__global__ __launch_bounds__(64) void hd_beer_flux_team_kernel(BeerArgs A, int nn) {
  constexpr int R = 64 / T;  // solves per block
  __shared__ double tile[R][kTL + 1];
  __shared__ double q_rmu[kBeerMaxNN], q_wmu[kBeerMaxNN];
  const int lane = threadIdx.x;
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < kBeerMaxNN; ++i) {
      q_rmu[i] = A.rmu[i];
      q_wmu[i] = A.wmu[i];
    }
  }
  __syncthreads();
  const int i = lane % T, r = lane / T;
  const long sb = (long)blockIdx.x * R;
  const int nv = (int)(A.nsc - sb < R ? A.nsc - sb : R);
  const bool live = r < nv;
  const bool lead = live && i == 0;        // the team's lane that stores
  const long sl = sb + (live ? r : 0);
  const long s = A.s0 + sl;
  const int L = A.nlyr, nlev = L + 1;
  const size_t nsc = (size_t)A.nsc;
  const bool planck = A.planckv != nullptr;
  const double rmu = q_rmu[i < nn ? i : 0];  // lanes past nn shadow stream 0, never summed
  const double bsurf = planck ? A.planckv[(size_t)(L + 1) * nsc + sl] : 0.0;
  int st = 0;
  const double fb = A.fbeam ? A.fbeam[s] : 0.0;
  const double mu0 = A.umu0 ? A.umu0[s] : 1.0;
  bool beam = fb > 0.0;
  if (beam && !(mu0 > 0.0 && mu0 <= 1.0)) {
    st |= kStBadInput;
    beam = false;
  }
  const double alb = A.albedo ? A.albedo[s] : 0.0;
  if (!(alb >= 0.0 && alb <= 1.0)) st |= kStBadInput;
  const double f0 = beam ? mu0 * fb : 0.0;

  auto stage_in = [&](int t0, int nl) {
    for (int idx = lane; idx < R * kTL; idx += 64) {
      const int rr = idx / kTL, l = idx % kTL;
      if (rr < nv && l < nl)
        tile[rr][l] = A.prop[((size_t)(A.s0 + sb + rr) * L + t0 + l) * A.nprop];
    }
  };
  auto stage_out = [&](int t0, int nl, int off, int dir) {
    for (int idx = lane; idx < R * kTL; idx += 64) {
      const int rr = idx / kTL, l = idx % kTL;
      if (rr < nv && l < nl)
        A.flux[((size_t)(sb + rr) * nlev + t0 + l + off) * 2 + dir] = tile[rr][l];
    }
  };
  auto hemi_flux = [&](double v) {  // hd_beer_flux_kernel's sum, stream 0 first
    double f = 0.0;
    for (int j = 0; j < nn; ++j) f = fma(q_wmu[j], __shfl(v, r * T + j), f);
    return 2.0 * kPi * f;
  };

  double I = (A.fisot ? A.fisot[s] : 0.0) + (planck ? A.planckv[(size_t)(L + 2) * nsc + sl] : 0.0);
  double fdn = hemi_flux(I) + f0;
  double chk = fdn;
  if (lead) A.flux[((size_t)sl * nlev + L) * 2 + 1] = fdn;
  double tauc = 0.0;
  double bin = planck ? A.planckv[(size_t)L * nsc + sl] : 0.0;
  for (int t0 = (L - 1) / kTL * kTL; t0 >= 0; t0 -= kTL) {
    const int nl = L - t0 < kTL ? L - t0 : kTL;
    __syncthreads();
    stage_in(t0, nl);
    __syncthreads();
    for (int l = nl - 1; l >= 0; --l) {
      const double d = tile[r][l];
      if (bad_tau(d)) st |= kStBadInput;
      const double bout = planck ? A.planckv[(size_t)(t0 + l) * nsc + sl] : 0.0;
      I = beer_step(I, d * rmu, bin, bout);
      bin = bout;
      tauc += d;
      fdn = hemi_flux(I) + (beam ? f0 * exp(-tauc / mu0) : 0.0);
      chk += fdn;
      if (i == 0) tile[r][l] = fdn;  // (the block is one wave: its lanes' reads came first)
    }
    __syncthreads();
    stage_out(t0, nl, 0, 1);
  }
  const double isurf = (1.0 - alb) * bsurf + alb * fdn / kPi;
  I = isurf;
  double fup = hemi_flux(I);
  chk += fup;
  if (lead) A.flux[(size_t)sl * nlev * 2] = fup;
  bin = planck ? A.planckv[sl] : 0.0;
  for (int t0 = 0; t0 < L; t0 += kTL) {
    const int nl = L - t0 < kTL ? L - t0 : kTL;
    __syncthreads();
    stage_in(t0, nl);
    __syncthreads();
    for (int l = 0; l < nl; ++l) {
      const double d = tile[r][l];
      const double bout = planck ? A.planckv[(size_t)(t0 + l + 1) * nsc + sl] : 0.0;
      I = beer_step(I, d * rmu, bin, bout);
      bin = bout;
      fup = hemi_flux(I);
      chk += fup;
      if (i == 0) tile[r][l] = fup;
    }
    __syncthreads();
    stage_out(t0, nl, 1, 0);
  }
  if (!isfinite(chk)) st |= kStNonFinite;
  if (lead) beer_flag(A.status, A.anyerr, s, st);
}

// ============================================================================
// rays: one lane per (solve, ray), the ray index fastest
// ============================================================================
__global__ __launch_bounds__(256) void hd_beer_ray_kernel(BeerRayArgs A) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= (long)A.nsc * A.nray) return;
  const long sl = tid / A.nray;
  const int r = (int)(tid - sl * A.nray);
  const long s = A.s0 + sl;
  const int L = A.nlyr;
  const size_t nsc = (size_t)A.nsc;
  const int c = (int)(s % A.ncol);
  const double mu = A.umu[A.per_column ? (size_t)c * A.nray + r : (size_t)r];
  double* out = A.rad + (size_t)sl * A.nray + r;
  if (!(mu != 0.0 && fabs(mu) <= 1.0)) {  // also a NaN
    *out = __builtin_nan("");
    beer_flag(A.status, A.anyerr, s, kStBadInput);
    return;
  }
  const bool planck = A.planckv != nullptr;
  const double rmu = 1.0 / fabs(mu);
  const double* p = A.prop + (size_t)s * L * A.nprop;
  int st = 0;
  double v, tsum = 0.0;
  if (mu > 0.0) {  // from the surface to the top
    v = A.xsurf[sl];
    double bin = planck ? A.planckv[sl] : 0.0;
    for (int l = 0; l < L; ++l) {
      const double d = p[(size_t)l * A.nprop];
      if (bad_tau(d)) st |= kStBadInput;
      const double bout = planck ? A.planckv[(size_t)(l + 1) * nsc + sl] : 0.0;
      v = beer_step(v, d * rmu, bin, bout);
      bin = bout;
      tsum += d;
    }
    if (A.alpha > 0.0) {
      const double xs = tsum * rmu;
      if (xs == 0.0) {
        st |= kStBadInput;
      } else if (xs < 1000.0) {
        const double alb = A.albedo ? A.albedo[s] : 0.0;
        const double bs = planck ? A.planckv[(size_t)(L + 1) * nsc + sl] : 0.0;
        v += (1.0 - alb) * bs * beer_alpha_term(A.alpha, xs);
      }
    }
  } else {  // from the top boundary to the surface
    v = (A.fisot ? A.fisot[s] : 0.0) + (planck ? A.planckv[(size_t)(L + 2) * nsc + sl] : 0.0);
    double bin = planck ? A.planckv[(size_t)L * nsc + sl] : 0.0;
    for (int l = L - 1; l >= 0; --l) {
      const double d = p[(size_t)l * A.nprop];
      if (bad_tau(d)) st |= kStBadInput;
      const double bout = planck ? A.planckv[(size_t)l * nsc + sl] : 0.0;
      v = beer_step(v, d * rmu, bin, bout);
      bin = bout;
    }
  }
  *out = v;
  if (!isfinite(v)) st |= kStNonFinite;
  beer_flag(A.status, A.anyerr, s, st);
}

// ============================================================================
// band sum of a chunk: one lane per output (column, element), the chunk's waves of that
// column in ascending order, one fma each -- hd_band_flux_kernel's sequence
// ============================================================================
__global__ __launch_bounds__(256) void hd_beer_band_acc_kernel(const double* x,
                                                               const double* weight,
                                                               double* out, long s0, int nsc,
                                                               int ncol, long m) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)ncol * m) return;
  const long c = t / m, e = t - c * m;
  const long last = s0 + nsc - 1;
  if (last < c) return;
  long w = s0 > c ? (s0 - c + ncol - 1) / ncol : 0;
  const long wend = (last - c) / ncol + 1;  // one past the chunk's last wave of column c
  double acc = out[t];
  const long base = (c - s0) * m + e;  // wave w at x[base + w * ncol * m]
  const long stride = (long)ncol * m;
  for (; w + 8 <= wend; w += 8) {  // the loads of eight waves in flight, the fmas in order
    double v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = x[base + (w + k) * stride];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc = fma(weight[w + k], v[k], acc);
  }
  for (; w < wend; ++w) acc = fma(weight[w], x[base + w * stride], acc);
  out[t] = acc;
}

// One column and many waves (line-by-line: ~80 outputs, 2e4 waves): the lane-per-output
// kernel above runs two waves whose every fma waits for its own load.  Here a block owns
// kAccE outputs; its first wave carries the fma chains, in the same order, out of LDS,
// while the other waves fetch the next kAccW waves' values into the second buffer
// (coalesced: kAccE consecutive doubles per wave), so a batch costs one memory round
// trip or its kAccW dependent fmas, whichever is longer, instead of both per wave.
constexpr int kAccE = 16, kAccW = 240, kAccThreads = 1024;
__global__ __launch_bounds__(kAccThreads) void hd_beer_band_acc_staged_kernel(
    const double* x, const double* weight, double* out, long s0, int nsc, long m) {
  __shared__ double buf[2][kAccW][kAccE];  // 60 KB
  __shared__ double wbuf[2][kAccW];
  const int tid = threadIdx.x;
  const long e0 = (long)blockIdx.x * kAccE;
  const int ne = (int)(m - e0 < kAccE ? m - e0 : kAccE);
  // waves w0 .. w0 + kAccW - 1 of the chunk, by the 960 lanes of waves 1..15: four values
  // each, the loads issued together before the first LDS store waits for them
  static_assert(kAccW * kAccE == 4 * (kAccThreads - 64), "four values per fetching lane");
  auto fetch = [&](int b, int w0) {
    double v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int idx = tid - 64 + j * (kAccThreads - 64);
      const int k = idx / kAccE, e = idx % kAccE;
      v[j] = (w0 + k < nsc && e < ne) ? x[(size_t)(w0 + k) * m + e0 + e] : 0.0;
    }
    const int kw = tid - 64;
    const double wv = (kw < kAccW && w0 + kw < nsc) ? weight[s0 + w0 + kw] : 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int idx = tid - 64 + j * (kAccThreads - 64);
      buf[b][idx / kAccE][idx % kAccE] = v[j];
    }
    if (kw < kAccW) wbuf[b][kw] = wv;
  };
  if (tid >= 64) fetch(0, 0);
  __syncthreads();
  double acc = (tid < ne) ? out[e0 + tid] : 0.0;
  int b = 0;
  for (int w0 = 0; w0 < nsc; w0 += kAccW, b ^= 1) {
    if (tid >= 64) {
      if (w0 + kAccW < nsc) fetch(b ^ 1, w0 + kAccW);
    } else if (tid < ne) {
      const int nw = nsc - w0 < kAccW ? nsc - w0 : kAccW;
      if (nw == kAccW) {  // a full batch: the next eight waves' LDS reads beside eight fmas
        double xa[8], wa[8], xb[8], wb[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          xa[j] = buf[b][j][tid];
          wa[j] = wbuf[b][j];
        }
        for (int k0 = 8; k0 <= kAccW; k0 += 8) {
          if (k0 < kAccW) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              xb[j] = buf[b][k0 + j][tid];
              wb[j] = wbuf[b][k0 + j];
            }
          }
#pragma unroll
          for (int j = 0; j < 8; ++j) acc = fma(wa[j], xa[j], acc);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            xa[j] = xb[j];
            wa[j] = wb[j];
          }
        }
      } else {
        for (int k = 0; k < nw; ++k) acc = fma(wbuf[b][k], buf[b][k][tid], acc);
      }
    }
    __syncthreads();
  }
  if (tid < ne) out[e0 + tid] = acc;
}

// ============================================================================
// gradients (Gradients): the exact adjoint of the kernels above
// ============================================================================
// The adjoint of hd_beer_flux_kernel, one lane per solve, tau through the same LDS tile.
// With the cotangent g on flux[lev][dir], the adjoints of the intensities obey
//   up    lam_up[l]  = 2 pi w mu g_up[l]  + t[l]   lam_up[l+1]   (top -> bottom)
//   down  lam_dn[l]  = 2 pi w mu g_dn'[l] + t[l-1] lam_dn[l-1]   (bottom -> top)
// with g_dn'[0] = g_dn[0] + albedo / pi * sum_i lam_up[0] (the Lambertian surface), and a
// layer's d/dtau pairs the adjoint leaving it with the intensity entering it.  So
//   sweep 1 (top -> bottom) recomputes I_down and runs lam_up, storing both as they enter
//           each layer from above: sweep[layer][2 NN][nsc];
//   sweep 2 (bottom -> top) recomputes I_up against the stored lam_up and runs lam_dn
//           against the stored I_down: dL/dtau per layer, dL/dB per level, the boundary
//           gradients in registers.
// SURF: the adjoint of the down pass alone from A.seed = dL/d(surface intensity), added to
// what hd_beer_ray_bwd_kernel wrote.
// A solve the forward flags BAD_INPUT gets NaN gradients and the same bit.
template <int NN, bool SURF>
__global__ __launch_bounds__(64) void hd_beer_flux_bwd_kernel(BeerBwdArgs A) {
  __shared__ double tile[64][kTL + 1];
  __shared__ double q_wmu[NN];
  const int lane = threadIdx.x;
  if constexpr (NN > 8) {
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < NN; ++i) q_wmu[i] = A.wmu[i];
    }
    __syncthreads();
  }
  const long sb = (long)blockIdx.x * 64;
  const int nv = (int)(A.nsc - sb < 64 ? A.nsc - sb : 64);
  const bool live = lane < nv;
  const long sl = sb + (live ? lane : 0);
  const long s = A.s0 + sl;
  const int L = A.nlyr, nlev = L + 1;
  const size_t nsc = (size_t)A.nsc;
  const bool planck = A.planckv != nullptr;
  const double bsurf = planck ? A.planckv[(size_t)(L + 1) * nsc + sl] : 0.0;
  if (SURF && !A.albedo) {  // a black surface: the seed reaches B(btemp) alone
    if (live && planck) A.gb[(size_t)(L + 1) * nsc + sl] += A.seed[sl];
    return;
  }
  int st = 0;
  const double fb = A.fbeam ? A.fbeam[s] : 0.0;
  const double mu0 = A.umu0 ? A.umu0[s] : 1.0;
  bool beam = fb > 0.0;
  if (beam && !(mu0 > 0.0 && mu0 <= 1.0)) {
    st |= kStBadInput;
    beam = false;
  }
  const double alb = A.albedo ? A.albedo[s] : 0.0;
  if (!(alb >= 0.0 && alb <= 1.0)) st |= kStBadInput;
  const double f0 = beam ? mu0 * fb : 0.0;

  auto wm = [&](int i) {
    if constexpr (NN > 8) return q_wmu[i];
    else return A.wmu[i];
  };
  // the cotangent of flux[lev][dir]
  const double* gp = nullptr;
  double wgt = 1.0;
  if constexpr (!SURF) {
    if (A.cot.per_wave) {
      gp = A.cot.per_wave + (size_t)s * nlev * 2;
    } else {
      gp = A.cot.band + (size_t)(s % A.ncol) * nlev * 2;
      wgt = A.cot.weight[s / A.ncol];
    }
  }
  auto cot = [&](int lev, int dir) {
    if constexpr (SURF) return 0.0;
    else return A.cot.per_wave ? gp[lev * 2 + dir] : wgt * gp[lev * 2 + dir];
  };
  auto stage_in = [&](int t0, int nl) {
#pragma unroll 2
    for (int idx = lane; idx < 64 * kTL; idx += 64) {
      const int r = idx / kTL, l = idx % kTL;
      if (r < nv && l < nl)
        tile[r][l] = A.prop[((size_t)(A.s0 + sb + r) * L + t0 + l) * A.nprop];
    }
  };
  auto stage_gtau = [&](int t0, int nl) {
#pragma unroll 2
    for (int idx = lane; idx < 64 * kTL; idx += 64) {
      const int r = idx / kTL, l = idx % kTL;
      if (r < nv && l < nl) {
        double* q = A.gtau + (size_t)(A.s0 + sb + r) * L + t0 + l;
        *q = SURF ? *q + tile[r][l] : tile[r][l];
      }
    }
  };

  // ---- sweep 1: top boundary -> surface ---------------------------------------------
  double I[NN], lam[NN];
  {
    const double top = (A.fisot ? A.fisot[s] : 0.0) + (planck ? A.planckv[(size_t)(L + 2) * nsc + sl] : 0.0);
    const double g2 = 2.0 * kPi * cot(L, 0);
#pragma unroll
    for (int i = 0; i < NN; ++i) {
      I[i] = top;
      lam[i] = g2 * wm(i);
    }
  }
  double tauc = 0.0;
  double bin = planck ? A.planckv[(size_t)L * nsc + sl] : 0.0;
  for (int t0 = (L - 1) / kTL * kTL; t0 >= 0; t0 -= kTL) {
    const int nl = L - t0 < kTL ? L - t0 : kTL;
    __syncthreads();
    stage_in(t0, nl);
    __syncthreads();
    for (int l = nl - 1; l >= 0; --l) {
      const int ly = t0 + l;
      if (live) {
        double* q = A.sweep + (size_t)ly * 2 * NN * nsc + sl;
#pragma unroll
        for (int i = 0; i < NN; ++i) {
          q[(size_t)i * nsc] = I[i];
          if constexpr (!SURF) q[(size_t)(NN + i) * nsc] = lam[i];
        }
      }
      const double d = tile[lane][l];
      if (bad_tau(d)) st |= kStBadInput;
      const double bout = planck ? A.planckv[(size_t)ly * nsc + sl] : 0.0;
      const double g2 = 2.0 * kPi * cot(ly, 0);
#pragma unroll
      for (int i = 0; i < NN; ++i) {
        double t, cin, w1;
        beer_coef(d * A.rmu[i], t, cin, w1);
        I[i] = fma(I[i], t, fma(bout, w1, bin * cin));
        lam[i] = fma(t, lam[i], g2 * wm(i));
      }
      bin = bout;
      tauc += d;
    }
  }
  // ---- Lambertian surface -----------------------------------------------------------
  const double ttot = tauc;
  double fdn = 0.0, sup = SURF ? A.seed[sl] : 0.0;
#pragma unroll
  for (int i = 0; i < NN; ++i) {
    fdn = fma(wm(i), I[i], fdn);
    if constexpr (!SURF) sup += lam[i];
  }
  const double e0 = beam ? exp(-ttot / mu0) : 0.0;
  fdn = 2.0 * kPi * fdn + f0 * e0;
  const double isurf = (1.0 - alb) * bsurf + alb * fdn / kPi;
  const bool bad = (st & kStBadInput) != 0;
  const double poison = bad ? __builtin_nan("") : 0.0;  // added to everything written
  const double g_alb = sup * (fdn / kPi - bsurf);
  const double g_bsurf = sup * (1.0 - alb);
  double gd = cot(0, 1) + sup * alb / kPi;  // dL/d(total downward flux) at the level
  // ---- sweep 2: surface -> top ------------------------------------------------------
  double gbeam = gd * e0;             // sum over the levels passed of gd e^(-tauc / mu0)
  double g_fb = gd * mu0 * e0;
  double g_mu0 = gd * fb * e0 * (1.0 + ttot / mu0);
  {
    const double g2 = 2.0 * kPi * gd;
#pragma unroll
    for (int i = 0; i < NN; ++i) {
      I[i] = isurf;
      lam[i] = g2 * wm(i);
    }
  }
  double chk = g_alb + g_bsurf;
  double tsum = 0.0, carry = 0.0;  // carry: dL/dB of the level below the layer, so far
  bin = planck ? A.planckv[sl] : 0.0;
  for (int t0 = 0; t0 < L; t0 += kTL) {
    const int nl = L - t0 < kTL ? L - t0 : kTL;
    __syncthreads();
    stage_in(t0, nl);
    __syncthreads();
    for (int l = 0; l < nl; ++l) {
      const int ly = t0 + l;
      const double d = tile[lane][l];
      const double bout = planck ? A.planckv[(size_t)(ly + 1) * nsc + sl] : 0.0;
      gd = cot(ly + 1, 1);
      const double g2 = 2.0 * kPi * gd;
      const double* q = A.sweep + (size_t)ly * 2 * NN * nsc + sl;
      double gt = 0.0, gbl = carry, gbu = 0.0;
#pragma unroll
      for (int i = 0; i < NN; ++i) {
        double t, cin, w1, w1p;
        beer_coef_d(d * A.rmu[i], t, cin, w1, w1p);
        const double idn = q[(size_t)i * nsc];
        if constexpr (!SURF) {  // up: enters at the level below with I[i], leaves with lup
          const double lup = q[(size_t)(NN + i) * nsc];
          gt = fma(lup, beer_dstep(I[i], A.rmu[i], bin, bout, t, w1p), gt);
          gbu = fma(lup, w1, gbu);
          gbl = fma(lup, cin, gbl);
          I[i] = fma(I[i], t, fma(bout, w1, bin * cin));
        }
        // down: enters at the level above with idn, leaves with lam[i]
        gt = fma(lam[i], beer_dstep(idn, A.rmu[i], bout, bin, t, w1p), gt);
        gbl = fma(lam[i], w1, gbl);
        gbu = fma(lam[i], cin, gbu);
        lam[i] = fma(t, lam[i], g2 * wm(i));
      }
      if (beam) {
        gt -= fb * gbeam;  // every level at or below the layer sees its thickness
        tsum += d;
        const double tc = ttot - tsum;  // the depth of the layer's upper level
        const double e = exp(-tc / mu0);
        gbeam = fma(gd, e, gbeam);
        g_fb = fma(gd * mu0, e, g_fb);
        g_mu0 = fma(gd * fb * e, 1.0 + tc / mu0, g_mu0);
      }
      chk += gt + gbl;
      tile[lane][l] = gt + poison;  // (the lane's own slot: its thickness has been read)
      if (planck && live) {
        double* b = A.gb + (size_t)ly * nsc + sl;
        *b = (SURF ? *b + gbl : gbl) + poison;
      }
      carry = gbu;
      bin = bout;
    }
    if (A.gtau) {
      __syncthreads();
      stage_gtau(t0, nl);
    }
  }
  double g_top = 0.0;
#pragma unroll
  for (int i = 0; i < NN; ++i) g_top += lam[i];
  chk += carry + g_top + g_fb + g_mu0;
  if (!bad && !isfinite(chk)) st |= kStNonFinite;
  if (live) {
    auto put = [&](double* p, size_t k, double v) {
      if (p) p[k] = (SURF ? p[k] + v : v) + poison;
    };
    if (planck) {
      put(A.gb, (size_t)L * nsc + sl, carry);
      put(A.gb, (size_t)(L + 1) * nsc + sl, g_bsurf);
      put(A.gb, (size_t)(L + 2) * nsc + sl, g_top);
    }
    put(A.g_albedo, s, g_alb);
    put(A.g_fbeam, s, beam ? g_fb : 0.0);
    put(A.g_umu0, s, beam ? g_mu0 : 0.0);
    put(A.g_fisot, s, g_top);
    beer_flag(A.status, A.anyerr, s, st);
  }
}

// ============================================================================
// the adjoint along the rays: one lane per solve, walking its rays in order
// ============================================================================
// A ray's adjoint is g times the transmission from the layer to where the ray emerges,
// formed as exp(-(x_total - x_passed)) beside the recomputed intensity (both sums in the
// walk's own order, so the last layer's is exp(0)): no per-ray scratch.  The tau and B
// gradients of a solve's rays add up in ray order in the lane; upward rays leave the sum
// of their adjoints at the surface in A.seed for hd_beer_flux_bwd_kernel<NN, true>.
__global__ __launch_bounds__(64) void hd_beer_ray_bwd_kernel(BeerRayBwdArgs A) {
  const long sl = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (sl >= A.nsc) return;
  const long s = A.s0 + sl;
  const int L = A.nlyr;
  const size_t nsc = (size_t)A.nsc;
  const int c = (int)(s % A.ncol);
  const bool planck = A.planckv != nullptr;
  const double* p = A.prop + (size_t)s * L * A.nprop;
  double* gtau = A.gtau ? A.gtau + (size_t)s * L : nullptr;
  const double wgt = A.cot.per_wave ? 1.0 : A.cot.weight[s / A.ncol];
  const double* gp = A.cot.per_wave ? A.cot.per_wave + (size_t)s * A.nray
                                    : A.cot.band + (size_t)c * A.nray;
  const double alb = A.albedo ? A.albedo[s] : 0.0;
  const double bs = planck ? A.planckv[(size_t)(L + 1) * nsc + sl] : 0.0;
  const double top = (A.fisot ? A.fisot[s] : 0.0) + (planck ? A.planckv[(size_t)(L + 2) * nsc + sl] : 0.0);
  auto blev = [&](int lev) { return planck ? A.planckv[(size_t)lev * nsc + sl] : 0.0; };
  int st = 0;
  if (gtau)
    for (int l = 0; l < L; ++l) gtau[l] = 0.0;
  if (planck)
    for (int l = 0; l <= L; ++l) A.gb[(size_t)l * nsc + sl] = 0.0;
  double seed = 0.0, g_top = 0.0, g_alb = 0.0, g_bs = 0.0, chk = 0.0;
  for (int r = 0; r < A.nray; ++r) {
    const double mu = A.umu[A.per_column ? (size_t)c * A.nray + r : (size_t)r];
    if (!(mu != 0.0 && fabs(mu) <= 1.0)) {
      st |= kStBadInput;
      continue;
    }
    const bool up = mu > 0.0;
    const double rmu = 1.0 / fabs(mu);
    const double g = A.cot.per_wave ? gp[r] : wgt * gp[r];
    double xtot = 0.0, dsum = 0.0;  // in the walk's order: from the side the ray enters
    for (int k = 0; k < L; ++k) {
      const double d = p[(size_t)(up ? k : L - 1 - k) * A.nprop];
      if (bad_tau(d)) st |= kStBadInput;
      xtot += d * rmu;
      dsum += d;
    }
    double ga = 0.0;  // the alpha term's dL/dtau, the same for every layer
    if (up && A.alpha > 0.0) {
      const double xs = dsum * rmu;
      if (xs == 0.0) {
        st |= kStBadInput;
      } else if (xs < 1000.0) {
        const double a = beer_alpha_term(A.alpha, xs);
        const double da = -A.alpha * exp(-xs) / xs - A.alpha / xs * a;
        g_alb -= g * bs * a;
        g_bs = fma(g * (1.0 - alb), a, g_bs);
        ga = g * (1.0 - alb) * bs * da * rmu;
      }
    }
    double v = up ? A.xsurf[sl] : top;
    double bin = blev(up ? 0 : L), xpass = 0.0, carry = 0.0;
    for (int k = 0; k < L; ++k) {
      const int ly = up ? k : L - 1 - k;
      const int lin = up ? ly : ly + 1, lout = up ? ly + 1 : ly;
      const double d = p[(size_t)ly * A.nprop];
      const double x = d * rmu;
      const double bout = blev(lout);
      double t, cin, w1, w1p;
      beer_coef_d(x, t, cin, w1, w1p);
      xpass += x;
      const double rem = xtot - xpass;
      const double lam = rem > 0.0 ? g * exp(-rem) : g;  // the adjoint leaving the layer
      const double gt = fma(lam, beer_dstep(v, rmu, bin, bout, t, w1p), ga);
      chk += gt;
      if (gtau) gtau[ly] += gt;
      if (planck) {
        A.gb[(size_t)lin * nsc + sl] += fma(lam, cin, carry);
        carry = lam * w1;
      }
      v = fma(v, t, fma(bout, w1, bin * cin));
      bin = bout;
    }
    if (planck) A.gb[(size_t)(up ? L : 0) * nsc + sl] += carry;
    const double lam0 = g * exp(-xtot);  // at the side the ray enters
    if (up) seed += lam0;
    else g_top += lam0;
  }
  chk += seed + g_top + g_alb + g_bs;
  const bool bad = (st & kStBadInput) != 0;
  if (!bad && !isfinite(chk)) st |= kStNonFinite;
  if (bad) {
    const double nan = __builtin_nan("");
    seed = g_top = g_alb = g_bs = nan;
    if (gtau)
      for (int l = 0; l < L; ++l) gtau[l] = nan;
    if (planck)
      for (int l = 0; l <= L; ++l) A.gb[(size_t)l * nsc + sl] = nan;
  }
  A.seed[sl] = seed;
  if (planck) {
    A.gb[(size_t)(L + 1) * nsc + sl] = g_bs;
    A.gb[(size_t)(L + 2) * nsc + sl] = g_top;
  }
  if (A.g_albedo) A.g_albedo[s] = g_alb;
  if (A.g_fisot) A.g_fisot[s] = g_top;
  if (A.g_fbeam) A.g_fbeam[s] = bad ? seed : 0.0;
  if (A.g_umu0) A.g_umu0[s] = bad ? seed : 0.0;
  beer_flag(A.status, A.anyerr, s, st);
}

// ============================================================================
// dL/dB -> dL/dT
// ============================================================================
// One lane per (level, solve) of a chunk's gb: the levels 0..nlyr become dL/dB dB/dT in
// place; the two boundary rows go to g_btemp and to g_ttemp / g_temis per solve.
__global__ __launch_bounds__(256) void hd_beer_planck_bwd_kernel(BeerPlanckBwdArgs A) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int nl = A.nlyr + 3;
  if (tid >= (long)A.nsc * nl) return;
  const int lev = (int)(tid / A.nsc);
  const int sl = (int)(tid - (long)lev * A.nsc);
  const long s = A.s0 + sl;
  const int w = (int)(s / A.ncol);
  const int c = (int)(s - (long)w * A.ncol);
  const size_t k = (size_t)lev * A.nsc + sl;
  const double g = A.gb[k], wlo = A.wlo[w], whi = A.whi[w];
  if (lev <= A.nlyr) {
    A.gb[k] = g * beer_dplanck(wlo, whi, A.temf[(size_t)c * (A.nlyr + 1) + lev], A.planckv[k]);
  } else if (lev == A.nlyr + 1) {
    if (A.g_btemp) A.g_btemp[s] = g * beer_dplanck(wlo, whi, A.btemp ? A.btemp[s] : 0.0, A.planckv[k]);
  } else if (A.g_ttemp || A.g_temis) {
    const double te = A.temis ? A.temis[s] : 0.0, tt = A.ttemp ? A.ttemp[s] : 0.0;
    const double b = plkavg(wlo, whi, tt);
    if (A.g_ttemp) A.g_ttemp[s] = g * te * beer_dplanck(wlo, whi, tt, b);
    if (A.g_temis) A.g_temis[s] = g * b;
  }
}

// gtemf[c][lev] += the chunk's waves of column c in ascending order, one add each, carried
// through memory from chunk to chunk: the same chain at every chunk size, no atomics
__global__ __launch_bounds__(256) void hd_beer_temf_acc_kernel(const double* gb, double* gtemf,
                                                               long s0, int nsc, int ncol,
                                                               int nlev) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)ncol * nlev) return;
  const long c = t / nlev, lev = t - c * nlev;
  const long last = s0 + nsc - 1;
  if (last < c) return;
  long w = s0 > c ? (s0 - c + ncol - 1) / ncol : 0;
  const long wend = (last - c) / ncol + 1;
  const long base = lev * nsc + (c - s0);  // wave w at gb[base + w * ncol]
  double acc = gtemf[t];
  for (; w + 8 <= wend; w += 8) {
    double v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = gb[base + (w + k) * ncol];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc += v[k];
  }
  for (; w < wend; ++w) acc += gb[base + w * ncol];
  gtemf[t] = acc;
}

// ============================================================================
// launchers
// ============================================================================
template <bool SURF>
static hipError_t launch_beer_nn(int nn, const BeerArgs& a, hipStream_t stream) {
  const dim3 grid((unsigned)((a.nsc + 63) / 64)), block(64);
  return dispatch_nn<1, kBeerMaxNN>(nn, [&](auto NN) {
    hipLaunchKernelGGL((hd_beer_flux_kernel<NN, SURF>), grid, block, 0, stream, a);
    return hipGetLastError();
  });
}

// chunks of at most this many solves (under two one-lane waves per CU) take the team kernel
constexpr int kBeerTeamMaxSolves = 2048;

hipError_t launch_beer_flux(int nn, const BeerArgs& a, hipStream_t stream) {
  if (nn >= 2 && a.nsc <= kBeerTeamMaxSolves) {
    const int t = nn <= 2 ? 2 : nn <= 4 ? 4 : nn <= 8 ? 8 : 16;
    const dim3 grid((unsigned)(((long)a.nsc * t + 63) / 64)), block(64);
    if (t == 2) hipLaunchKernelGGL(hd_beer_flux_team_kernel<2>, grid, block, 0, stream, a, nn);
    else if (t == 4) hipLaunchKernelGGL(hd_beer_flux_team_kernel<4>, grid, block, 0, stream, a, nn);
    else if (t == 8) hipLaunchKernelGGL(hd_beer_flux_team_kernel<8>, grid, block, 0, stream, a, nn);
    else hipLaunchKernelGGL(hd_beer_flux_team_kernel<16>, grid, block, 0, stream, a, nn);
    return hipGetLastError();
  }
  return launch_beer_nn<false>(nn, a, stream);
}

hipError_t launch_beer_surface(int nn, const BeerArgs& a, hipStream_t stream) {
  return launch_beer_nn<true>(nn, a, stream);
}

hipError_t launch_beer_rays(const BeerRayArgs& a, hipStream_t stream) {
  const long n = (long)a.nsc * a.nray;
  hipLaunchKernelGGL(hd_beer_ray_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                     a);
  return hipGetLastError();
}

template <bool SURF>
static hipError_t launch_beer_bwd_nn(int nn, const BeerBwdArgs& a, hipStream_t stream) {
  const dim3 grid((unsigned)((a.nsc + 63) / 64)), block(64);
  return dispatch_nn<1, kBeerMaxNN>(nn, [&](auto NN) {
    hipLaunchKernelGGL((hd_beer_flux_bwd_kernel<NN, SURF>), grid, block, 0, stream, a);
    return hipGetLastError();
  });
}

hipError_t launch_beer_flux_bwd(int nn, const BeerBwdArgs& a, hipStream_t stream) {
  return launch_beer_bwd_nn<false>(nn, a, stream);
}

hipError_t launch_beer_surface_bwd(int nn, const BeerBwdArgs& a, hipStream_t stream) {
  return launch_beer_bwd_nn<true>(nn, a, stream);
}

hipError_t launch_beer_rays_bwd(const BeerRayBwdArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(hd_beer_ray_bwd_kernel, dim3((unsigned)((a.nsc + 63) / 64)), dim3(64), 0,
                     stream, a);
  return hipGetLastError();
}

hipError_t launch_beer_planck_bwd(const BeerPlanckBwdArgs& a, hipStream_t stream) {
  const long n = (long)a.nsc * (a.nlyr + 3);
  hipLaunchKernelGGL(hd_beer_planck_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !a.gtemf) return e;
  const long m = (long)a.ncol * (a.nlyr + 1);
  hipLaunchKernelGGL(hd_beer_temf_acc_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0,
                     stream, a.gb, a.gtemf, a.s0, a.nsc, a.ncol, a.nlyr + 1);
  return hipGetLastError();
}

hipError_t launch_beer_band_acc(const double* x, const double* weight, double* out, long s0,
                                int nsc, int ncol, long m, hipStream_t stream) {
  const long n = (long)ncol * m;
  if (ncol == 1 && nsc >= 128 && m <= 4096) {  // (then wave w of the chunk is solve s0 + w)
    hipLaunchKernelGGL(hd_beer_band_acc_staged_kernel, dim3((unsigned)((m + kAccE - 1) / kAccE)),
                       dim3(kAccThreads), 0, stream, x, weight, out, s0, nsc, m);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(hd_beer_band_acc_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     stream, x, weight, out, s0, nsc, ncol, m);
  return hipGetLastError();
}

}  // namespace hd
