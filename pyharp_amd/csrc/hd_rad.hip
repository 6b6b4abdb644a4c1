// hd_rad.hip -- gfx950 kernels of the intensity path: every azimuthal mode,
// fluxes at user optical depths (usrtau) and radiances at user angles
// (usrang), nstr <= 32.  One lane owns one (solve, mode m) problem ("unit");
// units are mode-major inside a chunk (u = m*ns + sl), so a wave's lanes share
// m and the mode-m Legendre tables are uniform loads.
//
//   hd_rad_taus_kernel       unscaled depth of every level (cumsum from the top)
//   hd_rad_layer_kernel<NN>  per (unit, layer): the flux kernel's layer setup
//                            with the mode-m table Y_l^m(mu_i), parity split by
//                            (l+m), beam source x (2 - delta_m0), thermal only at
//                            m = 0; also keeps L, V, k and the particular
//                            solution for the radiance kernels  [c_soleig,
//                            c_upbeam, c_upisot per mode]
//   hd_rad_sweep_kernel<NN>  per unit: adding sweep (Lambert surface and top
//                            emission only at m = 0) and back-substitution that
//                            keeps I+ and I- at every level   [c_setmtx, c_solve0]
//   hd_rad_const_kernel<NN>  per (unit, layer): the layer's homogeneous
//                            constants from its level intensities, pivot-free;
//                            with radiances also the user-angle maps (hd_rad_lane.hpp)
//   hd_rad_flux_kernel<NN>   per (solve, user depth): fluxes from the m = 0
//                            field inside the layer   [c_fluxes] (hd_rad_lane.hpp)
//   hd_rad_user_map_kernel<NN>  per (unit, user angle): source-function integration
//                            along the ray through every layer, from the maps [c_usrint]
//   hd_rad_azimuth_kernel    uu = sum_m I_m cos(m (phi - phi0))
//   hd_rad_ray_kernel        paired rays (hd_solve_rays): azimuth sum and TMS/IMS per
//                            (solve, depth, ray), optional band sum over the waves
//
// The layer, sweep and user_map kernels here run at nstr <= 16 only (NN <= 8: every
// NN-loop unrolled, the matrices in registers); nstr 18..32 takes the team kernels
// of hd_team_mfma.hip and the rolled one-lane kernels of hd_rad_wide.hip, launched
// from the one sequence at the end of this file.  Record layouts: hd_rad_layout.hpp.
// hd_rad_spher.hip compiles this file a second time for the pseudo-spherical beam (kSpher).
//
// Formulation: DESIGN.md section 3b, mirrored in numpy by
// tests/kernel_model_rad.py; oracle: oracle/disort_rad_np.py.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "hd_rad.hpp"

// This source is compiled in two forms, as hd_rad_lane.hpp is: as it stands, and from
// hd_rad_spher.hip with HD_RAD_SPHER defined -- the beam-using one-lane kernels (layer,
// sweep, const, flux, user_map, ray) with the pseudo-spherical beam of DESIGN.md section 3e
// in namespace hd::spher, without the kernels that use no beam and without the launch
// sequence.  kSpher is a constant of the translation unit, not a template parameter: the
// plain kernels keep their names and their code.
#ifndef HD_RAD_SPHER
#define HD_RAD_SPHER 0
#endif

namespace hd {
#if HD_RAD_SPHER
namespace spher {
#endif

namespace {

constexpr bool kSpher = HD_RAD_SPHER != 0;
constexpr int kLayerBlockR = 256;
// the layer kernel's records (operators for the sweep, radiance records for the const,
// flux and user kernels): whole-line stores, read a kernel later -- nontemporal
#ifndef HD_RAD_NT
#define HD_RAD_NT 1
#endif
constexpr bool kRadNt = HD_RAD_NT != 0;
constexpr int kLayersPerBlockR = kLayerBlockR / 64;

__constant__ RadTabs<1, kMaxRegNN> c_rad;  // quadrature and Y_l^m table of NN 1..8
__constant__ RadCoef c_rcoef;             // the Y_l^m recurrence coefficients

}  // namespace

// quad_r / tab_r / ylm_row / flag, hd_rad_const_kernel and hd_rad_flux_kernel, unrolled
#include "hd_rad_lane.hpp"

#if !HD_RAD_SPHER
// ============================================================================
// unscaled depth of every level, solver order (0 = top)
// ============================================================================
__global__ __launch_bounds__(256) void hd_rad_taus_kernel(RadArgs A) {
  const int sl = blockIdx.x * blockDim.x + threadIdx.x;
  if (sl >= A.ns) return;
  const long s = A.s0 + sl;
  const int L = A.nlyr, np = A.nprop;
  const double* p = A.prop + (size_t)s * L * np;
  double t = 0.0;
  A.taus[sl] = 0.0;
  for (int lc = 0; lc < L; ++lc) {
    t += p[(size_t)(L - 1 - lc) * np];
    A.taus[(size_t)(lc + 1) * A.ns + sl] = t;
  }
  if (A.utau && A.ntau > 0 && A.utau[A.ntau - 1] > t * (1.0 + 1e-12) + 1e-300)
    flag(A, s, kStBadInput);  // user depth below the bottom
}
#endif  // !HD_RAD_SPHER

// ============================================================================
// per-(unit, layer) setup (hd_layer_kernel generalised to mode m)
// ============================================================================
// kSpher (pseudo-spherical beam): the beam's rate in this layer is
// sph_beam's secant (any sign, or zero) in place of 1/mu0 and its amplitude at the layer
// top exp(-ch'_top); Y_l^m(mu0) keeps the true mu0.
template <int NN>
__global__ __launch_bounds__(kLayerBlockR) void hd_rad_layer_kernel(RadArgs A) {
  constexpr int N = 2 * NN;
  using R = RadRec<NN>;
  using O = RadOps<NN>;
  __shared__ double psi_lds[NN * NN * kLayerBlockR];
  auto psi_at = [&](int e) -> double& { return psi_lds[e * kLayerBlockR + threadIdx.x]; };
  const Quad<NN>& Qc = quad_r<NN>();
  const int lt = threadIdx.x;
  const int ntile = (A.nu + 63) / 64;
  const int ts = blockIdx.x % ntile;
  const int tl = blockIdx.x / ntile;
  const int u = ts * 64 + (lt & 63);
  const int lc = tl * kLayersPerBlockR + (lt >> 6);
  const int L = A.nlyr;
  if (u >= A.nu || lc >= L) return;
  const int m = u / A.ns;
  const int sl = u - m * A.ns;
  const long s = A.s0 + sl;
  const size_t nu = A.nu;
  const int nm = A.nmom;
  const int np = A.nprop;
  int st = 0;

  const double* q = A.prop + ((size_t)s * L + (L - 1 - lc)) * np;
  const double tau = q[0];
  double ssa = np > 1 ? q[1] : 0.0;
  if (!(tau >= 0.0) || !(ssa >= 0.0) || !(ssa <= 1.0)) st |= kStBadInput;
  if (ssa == 1.0) ssa = 1.0 - kDither;
  const double f = nm >= N ? q[1 + N] : 0.0;
  if (!(f < 1.0)) st |= kStBadInput;
  const double taup = (1.0 - ssa * f) * tau;
  const double om = ssa * (1.0 - f) / (1.0 - ssa * f);
  const double rf = om / (1.0 - f);

  const double mu0 = A.umu0 ? A.umu0[s] : 1.0;
  const double fb = A.fbeam ? A.fbeam[s] : 0.0;
  bool beam = fb > 0.0 && mu0 > 0.0;
  if (fb > 0.0 && !(mu0 > 0.0 && mu0 <= 1.0)) st |= kStBadInput;  // cdisort c_chekin
  double rmu0 = beam ? 1.0 / mu0 : 0.0;
  double chtop = 0.0;  // kSpher: slant depth of the beam at the layer top
  if constexpr (kSpher) {
    beam = beam && sph_beam_on(A, sl);
    const SphBeam sb = sph_beam(A, lc, sl, taup);
    rmu0 = beam ? sb.lam : 0.0;
    chtop = sb.top;
  }
  const double mub = beam ? mu0 : 0.0;
  const bool therm = A.planck && m == 0;

  // ---- mode-m phase matrix even/odd parts (parity of l+m) + beam vectors ----
  double lch[NN][NN], ap[NN][NN], xs[NN], xd[NN];
#pragma unroll
  for (int i = 0; i < NN; ++i) {
    xs[i] = xd[i] = 0.0;
#pragma unroll
    for (int j = i; j < NN; ++j) lch[i][j] = ap[i][j] = 0.0;
  }
  {
    const int mp = m & 1;
    const double* lam = &tab_r<NN>().lam[m][0][0];
    const double seed = ylm_seed(m, mub);
    double y1 = 0.0, y2 = 0.0;  // Y_{l-1}^m(mu0), Y_{l-2}^m(mu0)
    // Y_l^m = 0 for l < m (tables and recurrence): the pairs below m/2 add exact zeros
#pragma nounroll
    for (int l2 = m >> 1; l2 < NN; ++l2) {
      const int la = 2 * l2, lb = la + 1;
      const double ya =
          la < m ? 0.0 : (la == m ? seed : fma(c_rcoef.ra[m][la] * mub, y1, -c_rcoef.rb[m][la] * y2));
      y2 = y1;
      y1 = ya;
      const double yb =
          lb < m ? 0.0 : (lb == m ? seed : fma(c_rcoef.ra[m][lb] * mub, y1, -c_rcoef.rb[m][lb] * y2));
      y2 = y1;
      y1 = yb;
      const int le = mp ? lb : la, lo = mp ? la : lb;
      const double pe0 = mp ? yb : ya, po0 = mp ? ya : yb;
      const double che = le == 0 ? 1.0 : (le <= nm ? q[1 + le] : 0.0);
      const double cho = lo == 0 ? 1.0 : (lo <= nm ? q[1 + lo] : 0.0);
      const double ge = (2 * le + 1) * (che - f) * rf;
      const double go = (2 * lo + 1) * (cho - f) * rf;
      const double* te = lam + le * NN;
      const double* to = lam + lo * NN;
      double ue[NN], uo[NN];
#pragma unroll
      for (int i = 0; i < NN; ++i) {
        ue[i] = ge * te[i];
        uo[i] = go * to[i];
        xs[i] = fma(ue[i], pe0, xs[i]);
        xd[i] = fma(uo[i], po0, xd[i]);
      }
#pragma unroll
      for (int i = 0; i < NN; ++i)
#pragma unroll
        for (int j = i; j < NN; ++j) {
          ap[i][j] = fma(ue[i], te[j], ap[i][j]);
          lch[i][j] = fma(uo[i], to[j], lch[i][j]);
        }
    }
  }
#pragma unroll
  for (int i = 0; i < NN; ++i)
#pragma unroll
    for (int j = i; j < NN; ++j) {
      const double diag = (i == j) ? Qc.rmu[i] : 0.0;
      const double sij = Qc.sd[i] * Qc.sd[j];
      lch[i][j] = fma(-sij, lch[i][j], diag);
      ap[i][j] = fma(-sij, ap[i][j], diag);
    }
  double rdl[NN];
  if (!chol_inplace<NN>(lch, rdl)) st |= kStEigen;

  double* rr = RadAt<NN>::rec(A.rrd, R::size, lc, nu, u);

  double y2[NN], lxd[NN];
  const double fb2 = fb * ((m == 0 ? 0.5 : 1.0) / kPi);
  if (beam) {
    double y[NN], z[NN];
#pragma unroll
    for (int i = 0; i < NN; ++i) y[i] = Qc.sd[i] * (fb2 * xs[i]);
#pragma unroll
    for (int i = 0; i < NN; ++i) {
      double t = 0.0;
#pragma unroll
      for (int k = i; k < NN; ++k) t = fma(lch[k][i], y[k], t);
      z[i] = t;
    }
#pragma unroll
    for (int i = 0; i < NN; ++i) {
      double t = 0.0;
#pragma unroll
      for (int k = 0; k <= i; ++k) t = fma(lch[i][k], z[k], t);
      y[i] = t;
    }
#pragma unroll
    for (int i = 0; i < NN; ++i) {
      const double xdi = -fb2 * xd[i];
      const double rv = fma(-y[i], Qc.rg[i], xdi * rmu0 * Qc.rmu[i]);
      y2[i] = Qc.g[i] * rv;
      lxd[i] = Qc.sd[i] * xdi;
    }
    lower_solve<NN>(lch, rdl, y2);  // V^T y2 below
    lower_solve<NN>(lch, rdl, lxd);
    lower_t_solve<NN>(lch, rdl, lxd);
  } else {
#pragma unroll
    for (int i = 0; i < NN; ++i) y2[i] = lxd[i] = 0.0;
  }
  // thermal (m = 0): cvec = dB + 2 (dB/tau') h,  h = W^-1 D^1/2 L^-T L^-1 D^1/2 mu
  double cvec[NN];
  double db = 0.0, bsum = 0.0;
  if (therm) {
    const double bt = A.planckv[(size_t)(L - lc) * A.ns + sl];
    const double bb = taup > 0.0 ? A.planckv[(size_t)(L - lc - 1) * A.ns + sl] : bt;
    db = bb - bt;
    bsum = bt + bb;
    const double b1 = taup > 0.0 ? 2.0 * db / taup : 0.0;
#pragma unroll
    for (int i = 0; i < NN; ++i) cvec[i] = Qc.sd[i] * Qc.mu[i];
    lower_solve<NN>(lch, rdl, cvec);
    lower_t_solve<NN>(lch, rdl, cvec);
#pragma unroll
    for (int i = 0; i < NN; ++i) {
      rec_st<kRadNt>(&rr[(R::H + i) * nu], Qc.rg[i] * cvec[i]);
      cvec[i] = fma(b1 * Qc.rg[i], cvec[i], db);
    }
    rec_st<kRadNt>(&rr[R::Bt * nu], bt);
    rec_st<kRadNt>(&rr[R::Sl * nu], 0.5 * b1);
  } else {
#pragma unroll
    for (int i = 0; i < NN; ++i) {
      cvec[i] = 0.0;
      rec_st<kRadNt>(&rr[(R::H + i) * nu], 0.0);
    }
    rec_st<kRadNt>(&rr[R::Bt * nu], 0.0);
    rec_st<kRadNt>(&rr[R::Sl * nu], 0.0);
  }
  rec_st<kRadNt>(&rr[R::Tp * nu], taup);
  rec_st<kRadNt>(&rr[R::Om * nu], om);
  {  // L (packed lower, row-major)
    int e = R::L;
#pragma unroll
    for (int i = 0; i < NN; ++i)
#pragma unroll
      for (int k = 0; k <= i; ++k) rec_st<kRadNt>(&rr[(e++) * nu], lch[i][k]);
  }

  // ---- eigenpairs (hd_layer_kernel's form): C C^T = -A+, X = L^T C, Sym = X X^T;
  // the one-sided Jacobi on X's columns gives B = X W with k_j = |b_j| and
  // V = B K^-1 (stored for the later kernels), U = L V ----
  double rdc[NN];
  if (!chol_inplace<NN>(ap, rdc)) st |= kStEigen;  // lower ap <- C
  double v[NN][NN];  // X, then B, then V, then Omega = L V Delta^1/2
#pragma unroll
  for (int i = 0; i < NN; ++i)
#pragma unroll
    for (int j = 0; j < NN; ++j) {  // X_ij = sum_{k >= max(i,j)} L_ki C_kj
      double t = 0.0;
#pragma unroll
      for (int k = (i > j ? i : j); k < NN; ++k) t = fma(lch[k][i], ap[k][j], t);
      v[i][j] = t;
    }
  if (!jacobi_os<NN>(v, A.max_sweeps)) st |= kStEigen;
  double kk[NN];  // k_j^2 first (hd_layer_kernel's form), then k_j
  column_norms2<NN>(v, kk);
  if (jacobi_os_polish<NN>(v, beam && near_resonance<NN>(kk, rmu0 * rmu0, kResPolish)))
    column_norms2<NN>(v, kk);
#pragma unroll
  for (int j = 0; j < NN; ++j) {
    const double k2 = kk[j];
    if (!(k2 > 0.0)) st |= kStEigen;
    const double rk = k2 > 0.0 ? rsq_nr(k2) : 0.0;
    kk[j] = k2 * rk;
    rec_st<kRadNt>(&rr[(R::K + j) * nu], kk[j]);
#pragma unroll
    for (int i = 0; i < NN; ++i) v[i][j] *= rk;  // V = B K^-1
  }

  // ---- beam particular solution at the layer top ----
  double zp[NN], zm[NN];
  double e0 = 0.0;
  if (beam) {
    double tt[NN];
    const double r2 = rmu0 * rmu0;
#pragma unroll
    for (int j = 0; j < NN; ++j) {  // tt = V^T y2 / (1/mu0^2 - k^2)
      double t = 0.0;
#pragma unroll
      for (int i = 0; i < NN; ++i) t = fma(v[i][j], y2[i], t);
      double den = fma(-kk[j], kk[j], r2);
      if (fabs(den) < kResClamp * r2) {
        st |= kStResonance;
        den = den < 0.0 ? -kResClamp * r2 : kResClamp * r2;
      }
      tt[j] = t / den;
    }
    double sv[NN], y[NN];
#pragma unroll
    for (int i = 0; i < NN; ++i) {  // V tt
      double t = 0.0;
#pragma unroll
      for (int j = 0; j < NN; ++j) t = fma(v[i][j], tt[j], t);
      y[i] = t;
    }
#pragma unroll
    for (int i = NN - 1; i >= 0; --i) {  // s = W^-1 D^1/2 L V tt
      double t = 0.0;
#pragma unroll
      for (int k = 0; k <= i; ++k) t = fma(lch[i][k], y[k], t);
      sv[i] = Qc.rg[i] * t;
    }
#pragma unroll
    for (int i = 0; i < NN; ++i) y[i] = Qc.sd[i] * Qc.mu[i] * sv[i];
    lower_solve<NN>(lch, rdl, y);
    lower_t_solve<NN>(lch, rdl, y);
    double att;
    if constexpr (kSpher) {
      att = 0.5 * exp(-chtop);
    } else {
      const double tauc = A.tauc[(size_t)lc * A.ns + sl];
      att = 0.5 * exp(-tauc * rmu0);
    }
#pragma unroll
    for (int i = 0; i < NN; ++i) {
      const double dd = Qc.rg[i] * fma(-y[i], rmu0, lxd[i]);
      zp[i] = (sv[i] + dd) * att;
      zm[i] = (sv[i] - dd) * att;
    }
    e0 = exp(-taup * rmu0);
  } else {
#pragma unroll
    for (int i = 0; i < NN; ++i) zp[i] = zm[i] = 0.0;
  }
#pragma unroll
  for (int i = 0; i < NN; ++i) {
    rec_st<kRadNt>(&rr[(R::Zp + i) * nu], zp[i]);
    rec_st<kRadNt>(&rr[(R::Zm + i) * nu], zm[i]);
  }

  // ---- layer operators in the flux-weighted basis (as hd_layer_kernel) ----
  double dsq[NN], gsq[NN];
#pragma unroll
  for (int j = 0; j < NN; ++j) {
    const double x = kk[j] * taup;
    const double mm = -expm1(-x);
    const double th = mm * rcp_nr(2.0 - mm);
    const double delta = x > 1.0e-8 ? th * rcp_nr(kk[j] > 0.0 ? kk[j] : 1.0) : 0.5 * taup;
    dsq[j] = sqrt(delta);
    gsq[j] = sqrt(kk[j] * th);
    rec_st<kRadNt>(&rr[(R::Ek + j) * nu], 1.0 - mm);  // exp(-k tau') for the user-angle kernel
  }
  rec_st<kRadNt>(&rr[R::E0 * nu], e0);
#pragma unroll
  for (int j = 0; j < NN; ++j) {  // V (stored), Psi^T = L^-T V Gamma^1/2 -> LDS
    double x[NN];
#pragma unroll
    for (int i = 0; i < NN; ++i) {
      rec_st<kRadNt>(&rr[(R::V + i * NN + j) * nu], v[i][j]);
      x[i] = v[i][j] * gsq[j];
    }
    lower_t_solve<NN>(lch, rdl, x);
#pragma unroll
    for (int i = 0; i < NN; ++i) psi_at(i * NN + j) = x[i];
  }
#pragma unroll
  for (int j = 0; j < NN; ++j)  // Omega = L V Delta^1/2, in place (rows bottom-up)
#pragma unroll
    for (int i = 0; i < NN; ++i) v[i][j] *= dsq[j];
#pragma unroll
  for (int i = NN - 1; i >= 0; --i)
#pragma unroll
    for (int j = 0; j < NN; ++j) {
      double t = 0.0;
#pragma unroll
      for (int k = 0; k <= i; ++k) t = fma(lch[i][k], v[k][j], t);
      v[i][j] = t;
    }

  double* out = RadAt<NN>::rec(A.rsw, O::size, lc, nu, u);
  double ga[NN], gb[NN];
#pragma unroll
  for (int i = 0; i < NN; ++i) {
    ga[i] = Qc.g[i] * (cvec[i] - fma(-zp[i], e0, zm[i]));
    gb[i] = Qc.g[i] * (fma(zp[i], e0, zm[i]) + bsum);
  }
  // Woodbury (as hd_layer_kernel): Q~- = I - A-, Q~+ = A+ - I with
  // A- = (I + Omega Omega^T)^-1, A+ = (I + Psi^T Psi)^-1; R~ = A+ - A-, T~ = A- + A+ - I
  double pvec[NN], am_[NN][NN];
  {
#pragma unroll
    for (int i = 0; i < NN; ++i)
#pragma unroll
      for (int j = i; j < NN; ++j) {
        double t = (i == j) ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < NN; ++k) t = fma(v[i][k], v[j][k], t);
        am_[i][j] = t;
      }
    double rdh[NN];
    if (!chol_inplace<NN>(am_, rdh)) st |= kStEigen;
    spd_inverse_upper<NN>(am_, rdh);
#pragma unroll
    for (int i = 0; i < NN; ++i) {  // p = Q~- ga = ga - A- ga
      double t = ga[i];
#pragma unroll
      for (int j = 0; j < NN; ++j) t = fma(-HD_SYM(am_, i, j), ga[j], t);
      pvec[i] = t;
    }
  }
  double ap_[NN][NN], qvec[NN];
  {
    double pt_[NN][NN];  // pt_[i][j] = Psi^T[i][j]
#pragma unroll
    for (int i = 0; i < NN; ++i)
#pragma unroll
      for (int j = 0; j < NN; ++j) pt_[i][j] = psi_at(i * NN + j);
#pragma unroll
    for (int i = 0; i < NN; ++i)
#pragma unroll
      for (int j = i; j < NN; ++j) {
        double t = (i == j) ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < NN; ++k) t = fma(pt_[i][k], pt_[j][k], t);
        ap_[i][j] = t;
      }
    double rdh[NN];
    if (!chol_inplace<NN>(ap_, rdh)) st |= kStEigen;
    spd_inverse_upper<NN>(ap_, rdh);
#pragma unroll
    for (int i = 0; i < NN; ++i) {  // q = Q~+ gb = A+ gb - gb
      double t = -gb[i];
#pragma unroll
      for (int j = 0; j < NN; ++j) t = fma(HD_SYM(ap_, i, j), gb[j], t);
      qvec[i] = t;
    }
  }
  double chk = 0.0;
  {
    int e = 0;
#pragma unroll
    for (int i = 0; i < NN; ++i)
#pragma unroll
      for (int j = i; j < NN; ++j) {
        const double r = ap_[i][j] - am_[i][j];
        const double t = (am_[i][j] + ap_[i][j]) - ((i == j) ? 1.0 : 0.0);
        rec_st<kRadNt>(&out[(O::R + e) * nu], r);
        rec_st<kRadNt>(&out[(O::T + e) * nu], t);
        chk += r + t;
        ++e;
      }
  }
#pragma unroll
  for (int i = 0; i < NN; ++i) {
    const double sp = Qc.g[i] * (zp[i] * (1.0 - e0) - db) + pvec[i] - qvec[i];
    const double sm = Qc.g[i] * (-zm[i] * (1.0 - e0) + db) - pvec[i] - qvec[i];
    rec_st<kRadNt>(&out[(O::Sp + i) * nu], sp);
    rec_st<kRadNt>(&out[(O::Sm + i) * nu], sm);
    chk += sp + sm;
  }
  rec_st<kRadNt>(&out[O::Tau * nu], taup);
  if (!isfinite(chk + taup)) st |= kStNonFinite;
  flag(A, s, st);
}

// ============================================================================
// per-unit adding sweep + back-substitution keeping I+/I- at every level
// ============================================================================
// kSpher: the surface is lit by the beam at its slant depth, exp(-ch'_0)
template <int NN>
#ifndef HD_RAD_SWEEP_WAVES
#define HD_RAD_SWEEP_WAVES 1
#endif
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(HD_RAD_SWEEP_WAVES)))
void hd_rad_sweep_kernel(RadArgs A) {
  const Quad<NN>& Qc = quad_r<NN>();
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= A.nu) return;
  const int m = u / A.ns;
  const int sl = u - m * A.ns;
  const long s = A.s0 + sl;
  const int L = A.nlyr;
  const size_t nu = A.nu;
  using O = RadOps<NN>;
  using B = RadBsub<NN>;
  using Lv = RadLev<NN>;
  int st = 0;

  const double mu0 = A.umu0 ? A.umu0[s] : 1.0;
  const double fb = A.fbeam ? A.fbeam[s] : 0.0;
  const bool beam = fb > 0.0 && mu0 > 0.0;
  double alb = A.albedo ? A.albedo[s] : 0.0;
  if (!(alb >= 0.0) || !(alb <= 1.0)) st |= kStBadInput;
  double top = A.fisot ? A.fisot[s] : 0.0;
  double bsurf = 0.0;
  if (A.planck) {
    bsurf = A.planckv[(size_t)(L + 1) * A.ns + sl];
    top += A.planckv[(size_t)(L + 2) * A.ns + sl];
  }
  if (m > 0) alb = top = bsurf = 0.0;  // Lambert surface, isotropic top: mode 0 only
  const double rmu0 = beam ? 1.0 / mu0 : 0.0;
  const double f0mu0 = (beam && m == 0) ? fb * mu0 : 0.0;

  double ra[NN][NN];
  double sd[NN];
#pragma unroll
  for (int i = 0; i < NN; ++i) {
    sd[i] = Qc.g[i] * top;
#pragma unroll
    for (int j = i; j < NN; ++j) ra[i][j] = 0.0;
  }
  double tauc = 0.0;
  for (int lc = 0; lc < L; ++lc) {
    const double* lp = RadAt<NN>::rec(A.rsw, O::size, lc, nu, u);
    double* bp = RadAt<NN>::rec(A.bsub, B::size, lc, nu, u);
    {  // stack above this layer: R_above (packed upper) and S_down
      int e = 0;
#pragma unroll
      for (int i = 0; i < NN; ++i)
#pragma unroll
        for (int j = i; j < NN; ++j) bp[(B::Ra + (e++)) * nu] = ra[i][j];
#pragma unroll
      for (int i = 0; i < NN; ++i) bp[(B::Sd + i) * nu] = sd[i];
    }
    double rl[NN][NN], spl[NN];
    {
      int e = O::R;
#pragma unroll
      for (int i = 0; i < NN; ++i)
#pragma unroll
        for (int j = i; j < NN; ++j) rl[i][j] = lp[(size_t)(e++) * nu];
#pragma unroll
      for (int i = 0; i < NN; ++i) spl[i] = lp[(size_t)(O::Sp + i) * nu];
    }
    double am[NN][NN], w1[NN][NN], t1[NN];
#pragma unroll
    for (int i = 0; i < NN; ++i)
#pragma unroll
      for (int j = 0; j < NN; ++j) am[i][j] = HD_SYM(ra, i, j);
#pragma unroll
    for (int i = 0; i < NN; ++i) {
#pragma unroll
      for (int j = 0; j < NN; ++j) {
        double t = (i == j) ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < NN; ++k) t = fma(-HD_SYM(rl, i, k), am[k][j], t);
        w1[i][j] = t;
      }
      double t = spl[i];
#pragma unroll
      for (int k = 0; k < NN; ++k) t = fma(HD_SYM(rl, i, k), sd[k], t);
      t1[i] = t;
    }
#pragma unroll
    for (int k = 0; k < NN; ++k) {
      const double piv = w1[k][k];
      if (!(fabs(piv) > 1.0e-12)) st |= kStPivot;
      const double rp = rcp_nr(piv);
      w1[k][k] = rp;
#pragma unroll
      for (int i = k + 1; i < NN; ++i) {
        const double l = w1[i][k] * rp;
        w1[i][k] = l;
#pragma unroll
        for (int j = k + 1; j < NN; ++j) w1[i][j] = fma(-l, w1[k][j], w1[i][j]);
      }
    }
#pragma unroll
    for (int i = 0; i < NN; ++i)
#pragma unroll
      for (int k = 0; k < i; ++k) t1[i] = fma(-w1[i][k], t1[k], t1[i]);
#pragma unroll
    for (int i = NN - 1; i >= 0; --i) {
#pragma unroll
      for (int k = i + 1; k < NN; ++k) t1[i] = fma(-w1[i][k], t1[k], t1[i]);
      t1[i] *= w1[i][i];
    }
    double uvec[NN];
#pragma unroll
    for (int i = 0; i < NN; ++i) {
      double t = sd[i];
#pragma unroll
      for (int k = 0; k < NN; ++k) t = fma(am[i][k], t1[k], t);
      uvec[i] = t;
      bp[(size_t)(B::Tv + i) * nu] = t1[i];
    }
#pragma unroll
    for (int r = 0; r < NN; ++r) {
#pragma unroll
      for (int j = 0; j < NN; ++j) {
        double t = am[r][j];
#pragma unroll
        for (int k = 0; k < j; ++k) t = fma(-am[r][k], w1[k][j], t);
        am[r][j] = t * w1[j][j];
      }
#pragma unroll
      for (int j = NN - 1; j >= 0; --j) {
        double t = am[r][j];
#pragma unroll
        for (int k = j + 1; k < NN; ++k) t = fma(-am[r][k], w1[k][j], t);
        am[r][j] = t;
      }
    }
    double tl[NN][NN];
    {
      int e = O::T;
#pragma unroll
      for (int i = 0; i < NN; ++i)
#pragma unroll
        for (int j = i; j < NN; ++j) tl[i][j] = lp[(size_t)(e++) * nu];
    }
#pragma unroll
    for (int j = 0; j < NN; ++j) {
      double x[NN];
#pragma unroll
      for (int i = 0; i < NN; ++i) x[i] = HD_SYM(tl, i, j);
#pragma unroll
      for (int i = 0; i < NN; ++i)
#pragma unroll
        for (int k = 0; k < i; ++k) x[i] = fma(-w1[i][k], x[k], x[i]);
#pragma unroll
      for (int i = NN - 1; i >= 0; --i) {
#pragma unroll
        for (int k = i + 1; k < NN; ++k) x[i] = fma(-w1[i][k], x[k], x[i]);
        x[i] *= w1[i][i];
      }
#pragma unroll
      for (int i = 0; i < NN; ++i) bp[(size_t)(B::Z + i * NN + j) * nu] = x[i];
    }
#pragma unroll
    for (int r = 0; r < NN; ++r) {
      double row[NN];
#pragma unroll
      for (int j = 0; j < NN; ++j) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < NN; ++k) t = fma(am[r][k], HD_SYM(tl, k, j), t);
        row[j] = t;
      }
#pragma unroll
      for (int j = 0; j < NN; ++j) am[r][j] = row[j];
    }
#pragma unroll
    for (int i = 0; i < NN; ++i) {
#pragma unroll
      for (int j = i; j < NN; ++j) {
        double t = rl[i][j];
#pragma unroll
        for (int k = 0; k < NN; ++k) t = fma(HD_SYM(tl, i, k), am[k][j], t);
        ra[i][j] = t;
      }
      double t = lp[(size_t)(O::Sm + i) * nu];
#pragma unroll
      for (int k = 0; k < NN; ++k) t = fma(HD_SYM(tl, i, k), uvec[k], t);
      sd[i] = t;
    }
    tauc += lp[(size_t)O::Tau * nu];
  }

  // ---- Lambertian surface (mode 0): I+ = x for every stream ----
  double gsd = 0.0, grg = 0.0;
#pragma unroll
  for (int i = 0; i < NN; ++i) {
    gsd += Qc.g[i] * sd[i];
#pragma unroll
    for (int j = 0; j < NN; ++j) grg += Qc.g[i] * HD_SYM(ra, i, j) * Qc.g[j];
  }
  double esurf = (1.0 - alb) * bsurf;
  if constexpr (kSpher) {  // the beam-on flag is read here, not held across the sweep
    if (beam && sph_beam_on(A, sl))
      esurf += alb * f0mu0 * exp(-A.chp[(size_t)L * A.ns + sl]) / kPi;
  } else {
    if (beam) esurf += alb * f0mu0 * exp(-tauc * rmu0) / kPi;
  }
  const double x = (2.0 * alb * gsd + esurf) / (1.0 - 2.0 * alb * grg);
  double ip[NN];
  double chk = 0.0;
  {
    double* lv = RadElemMajor::rec(A.lev, Lv::size, L, nu, u);
#pragma unroll
    for (int i = 0; i < NN; ++i) ip[i] = Qc.g[i] * x;
#pragma unroll
    for (int i = 0; i < NN; ++i) {
      double t = sd[i];
#pragma unroll
      for (int j = 0; j < NN; ++j) t = fma(HD_SYM(ra, i, j), ip[j], t);
      lv[(Lv::Ip + i) * nu] = x;
      lv[(Lv::Im + i) * nu] = t * Qc.rg[i];
      chk += t;
    }
  }
  // ---- back-substitution bottom -> top ----
  for (int lc = L - 1; lc >= 0; --lc) {
    const double* bp = RadAt<NN>::rec(A.bsub, B::size, lc, nu, u);
    double nip[NN];
#pragma unroll
    for (int i = 0; i < NN; ++i) {
      double t = bp[(size_t)(B::Tv + i) * nu];
#pragma unroll
      for (int j = 0; j < NN; ++j) t = fma(bp[(size_t)(B::Z + i * NN + j) * nu], ip[j], t);
      nip[i] = t;
    }
    double* lv = RadElemMajor::rec(A.lev, Lv::size, lc, nu, u);
#pragma unroll
    for (int i = 0; i < NN; ++i) ip[i] = nip[i];
    int e = 0;
    double dn[NN];
#pragma unroll
    for (int i = 0; i < NN; ++i) dn[i] = bp[(size_t)(B::Sd + i) * nu];
#pragma unroll
    for (int i = 0; i < NN; ++i)
#pragma unroll
      for (int j = i; j < NN; ++j) {
        const double r = bp[(size_t)(B::Ra + (e++)) * nu];
        dn[i] = fma(r, ip[j], dn[i]);
        if (j != i) dn[j] = fma(r, ip[i], dn[j]);
      }
#pragma unroll
    for (int i = 0; i < NN; ++i) {
      lv[(Lv::Ip + i) * nu] = ip[i] * Qc.rg[i];
      lv[(Lv::Im + i) * nu] = dn[i] * Qc.rg[i];
      chk += ip[i] + dn[i];
    }
  }
  if (!isfinite(chk)) st |= kStNonFinite;
  flag(A, s, st);
}

// ============================================================================
// per-(unit, user angle) source-function integration from the const kernel's maps
// (nstr <= 16): the layer's source projections are two NN x NN products with the
// angle's Y_l^m row (ce = Me ye, cx = Mo yo) instead of hd_rad_user_kernel's
// per-angle Legendre sums, triangular solve and V^T products; the beam and thermal
// amplitudes are dot products.  Everything after that -- the whole-layer terms,
// interior user depths, the scan over layers -- is hd_rad_user_kernel's.
// ============================================================================
#ifndef HD_RAD_UMAP_WAVES
#define HD_RAD_UMAP_WAVES 2
#endif
#ifndef HD_RAD_UMAP_UTAU_REG
#define HD_RAD_UMAP_UTAU_REG 1
#endif
constexpr bool kUmapUtauReg = HD_RAD_UMAP_UTAU_REG != 0;
// kSpher: the beam source of layer lc is ab exp(-lam t) with sph_beam's secant (the maps
// carry exp(-ch'_top) in ab); both whole-layer beam quotients, 1 + |mu| lam and
// 1 - |mu| lam, can vanish and go through dexp
template <int NN>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(HD_RAD_UMAP_WAVES)))
void hd_rad_user_map_kernel(RadArgs A) {
  constexpr int N = 2 * NN;
  using R = RadRec<NN>;
  using M = RadMap<NN>;
  using C = RadCst<NN>;
  const Quad<NN>& Qc = quad_r<NN>();
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long)A.ns * A.numu) return;
  const int sl = (int)(id / A.numu);
  const int iu = (int)(id - (long)sl * A.numu);
  const int m = blockIdx.y;
  const int u = m * A.ns + sl;
  const long s = A.s0 + sl;
  const int L = A.nlyr;
  const size_t nu = A.nu;
  const double muu = user_mu(A, s, iu);
  const double mu0 = A.umu0 ? A.umu0[s] : 1.0;
  const double fb = A.fbeam ? A.fbeam[s] : 0.0;
  bool beam = fb > 0.0 && mu0 > 0.0;
  if constexpr (kSpher) beam = beam && sph_beam_on(A, sl);
  double rmu0 = beam ? 1.0 / mu0 : 0.0;  // kSpher: the layer's secant, set per layer
  const bool therm = A.planck && m == 0;
  const int par = m & 1;
  double ye[NN], yo[NN];
  {
    double yu[N];
    ylm_row<N>(m, muu, yu);
#pragma unroll
    for (int l2 = 0; l2 < NN; ++l2) {
      ye[l2] = yu[2 * l2 + par];
      yo[l2] = yu[2 * l2 + 1 - par];
    }
  }
  const bool up = muu > 0.0;

  double cur = 0.0;
  if (up) {
    if (m == 0) {
      const double* lv = RadElemMajor::rec(A.lev, RadLev<NN>::size, L, nu, u);
      double fdn = 0.0;
#pragma unroll
      for (int i = 0; i < NN; ++i) fdn = fma(Qc.g[i] * Qc.g[i], lv[(RadLev<NN>::Im + i) * nu], fdn);
      fdn *= 2.0 * kPi;
      const double alb = A.albedo ? A.albedo[s] : 0.0;
      if constexpr (kSpher) {
        if (beam) fdn += fb * mu0 * exp(-A.chp[(size_t)L * A.ns + sl]);
      } else if (beam) {
        const double tb = A.tauc[(size_t)(L - 1) * A.ns + sl] +
                          RadAt<NN>::rec(A.rrd, R::size, L - 1, nu, u)[R::Tp * nu];
        fdn += fb * mu0 * exp(-tb * rmu0);
      }
      cur = alb / kPi * fdn + (A.planck ? (1.0 - alb) * A.planckv[(size_t)(L + 1) * A.ns + sl]
                                        : 0.0);
    }
  } else if (m == 0) {
    cur = A.fisot ? A.fisot[s] : 0.0;
    if (A.planck) cur += A.planckv[(size_t)(L + 2) * A.ns + sl];
  }
  int k = up ? A.ntau - 1 : 0;
  // the next user depth in ray order, held in a register: reloaded only when a depth
  // is consumed, not on every layer's loop test (a dependent load per layer)
  auto utau_at = [&](int kk) { return kk >= 0 && kk < A.ntau ? user_tau(A, kk, sl) : 0.0; };
  double utk = kUmapUtauReg ? utau_at(k) : 0.0;
  double chk = 0.0;
  for (int step = 0; step < L; ++step) {
    const int lc = up ? L - 1 - step : step;
    const double ttop = A.taus[(size_t)lc * A.ns + sl];
    const double tbot = A.taus[(size_t)(lc + 1) * A.ns + sl];
    const double* rr = RadAt<NN>::rec(A.rrd, R::size, lc, nu, u);
    const double* m1 = RadAt<NN>::rec(A.rsw, RadOps<NN>::size, lc, nu, u);
    const double* m2 = RadAt<NN>::rec(A.bsub, RadBsub<NN>::size, lc, nu, u);
    const double* co = RadElemMajor::rec(A.cst, C::size, lc, nu, u);
    const double bt = rr[R::Bt * nu], slope = rr[R::Sl * nu], taup = rr[R::Tp * nu];
    if constexpr (kSpher) rmu0 = beam ? sph_beam(A, lc, sl, taup).lam : 0.0;
    double kk[NN], hpl[NN], hmi[NN];
#pragma unroll
    for (int j = 0; j < NN; ++j) {
      double ce = 0.0, cx = 0.0;
#pragma unroll
      for (int l2 = 0; l2 < NN; ++l2) {
        ce = fma(m1[(size_t)(M::Me + j * NN + l2) * nu], ye[l2], ce);
        cx = fma(m2[(size_t)(M::Mo + j * NN + l2) * nu], yo[l2], cx);
      }
      kk[j] = rr[(R::K + j) * nu];
      cx *= -kk[j];
      hpl[j] = co[(C::Cp + j) * nu] * (ce + cx);
      hmi[j] = co[(C::Cm + j) * nu] * (ce - cx);
      // one row of the maps in flight at a time, consumed before the next row's loads
      // (at two waves per SIMD the other wave covers the latency; with the products
      // sunk below all 128 loads the kernel needed 490 registers)
      asm volatile("" : "+v"(hpl[j]), "+v"(hmi[j])::"memory");
    }
    double ab = 0.0, a0 = 0.0, a1t = 0.0;
    if (beam) {
#pragma unroll
      for (int l2 = 0; l2 < NN; ++l2) {
        ab = fma(m1[(size_t)(M::Abe + l2) * nu], ye[l2], ab);
        ab = fma(m1[(size_t)(M::Abo + l2) * nu], yo[l2], ab);
      }
    }
    if (therm) {
      double we = 0.0, wo = 0.0;
#pragma unroll
      for (int l2 = 0; l2 < NN; ++l2) {
        we = fma(m1[(size_t)(M::Tve + l2) * nu], ye[l2], we);
        wo = fma(m2[(size_t)(M::Tvo + l2) * nu], yo[l2], wo);
      }
      const double om = rr[R::Om * nu];
      const double ce0 = (1.0 - om) + 2.0 * we;
      a1t = slope * ce0;
      a0 = fma(bt, ce0, 2.0 * slope * wo);
    }
    // general segment [t1 (evaluation), t2 (far end)] for user depths inside the layer
    auto integ = [&](double t1, double t2) {
      double r = 0.0;
#pragma unroll
      for (int j = 0; j < NN; ++j) {
        r += seg_exp(hpl[j], kk[j], t1, t2, 0.0, muu);
        r += seg_exp(hmi[j], -kk[j], t1, t2, taup, muu);
        asm volatile("" : "+v"(r));  // one eigen-term at a time
      }
      if (beam) r += seg_exp(ab, rmu0, t1, t2, 0.0, muu);
      if (therm) {
        const double e2 = exp(-(t2 - t1) / muu);
        r += (a0 + a1t * t1 + a1t * muu) - (a0 + a1t * t2 + a1t * muu) * e2;
      }
      return r;
    };
    const double anu = fabs(muu);
    const double lmu = taup / anu;
    const double emu = exp(-lmu);
    double lay = 0.0;
#pragma unroll
    for (int j = 0; j < NN; ++j) {
      const double ek = rr[(R::Ek + j) * nu];
      const double reg = (1.0 - ek * emu) / fma(kk[j], anu, 1.0);
      const double sng = dexp(ek, emu, fma(-kk[j], anu, 1.0), lmu);
      lay = up ? fma(hpl[j], reg, fma(hmi[j], sng, lay)) : fma(hpl[j], sng, fma(hmi[j], reg, lay));
      asm volatile("" : "+v"(lay));  // one eigen-term's quotient and series at a time
    }
    if (beam) {
      const double e0l = rr[R::E0 * nu];
      if constexpr (kSpher)
        lay += up ? ab * dexp(1.0, e0l * emu, fma(anu, rmu0, 1.0), lmu)
                  : ab * dexp(e0l, emu, fma(-anu, rmu0, 1.0), lmu);
      else
        lay += up ? ab * (1.0 - e0l * emu) / fma(anu, rmu0, 1.0)
                  : ab * dexp(e0l, emu, fma(-anu, rmu0, 1.0), lmu);
    }
    if (therm) {
      lay += up ? (a0 + a1t * muu) - (a0 + a1t * taup + a1t * muu) * emu
                : (a0 + a1t * taup + a1t * muu) - (a0 + a1t * muu) * emu;
    }
    const double cin = cur;
    const double cout = fma(cin, emu, lay);
    const double tau = tbot - ttop;
    const double scale = tau > 0.0 ? taup / tau : 0.0;
    auto at = [&](double t) {
      const double tin = up ? taup : 0.0;
      if (t == tin) return cin;
      if (t == taup - tin) return cout;
      return cin * exp(-fabs(tin - t) / anu) + integ(t, tin);
    };
    // the user depths in this layer, in ray order (one copy of the interior integral)
    while (up ? (k >= 0 && (kUmapUtauReg ? utk : user_tau(A, k, sl)) >= ttop)
              : (k < A.ntau && (kUmapUtauReg ? utk : user_tau(A, k, sl)) <= tbot)) {
      const double t = fmin(fmax(((kUmapUtauReg ? utk : user_tau(A, k, sl)) - ttop) * scale, 0.0), taup);
      const double val = at(t);
      A.radm[((size_t)k * A.numu + iu) * nu + u] = val;
      chk += val;
      k += up ? -1 : 1;
      if (kUmapUtauReg) utk = utau_at(k);
    }
    cur = cout;
  }
  for (; k < A.ntau && !up; ++k) A.radm[((size_t)k * A.numu + iu) * nu + u] = cur;
  if (!isfinite(chk)) flag(A, s, kStNonFinite);
}

#if !HD_RAD_SPHER
// ============================================================================
// uu[s][j][lu][iu] = sum_m I_m cos(m (phi_j - phi0))
// ============================================================================
__global__ __launch_bounds__(256) void hd_rad_azimuth_kernel(RadArgs A) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long n = (long)A.ns * A.nphi * A.ntau * A.numu;
  if (id >= n) return;
  const int sl = (int)(id % A.ns);
  long r = id / A.ns;
  const int iu = (int)(r % A.numu);
  r /= A.numu;
  const int lu = (int)(r % A.ntau);
  const int j = (int)(r / A.ntau);
  const long s = A.s0 + sl;
  const double ph0 = A.phi0 ? A.phi0[s] : 0.0;
  const double dphi = (A.phi[j] - ph0) * (kPi / 180.0);
  const double* src = A.radm + ((size_t)lu * A.numu + iu) * A.nu + sl;
  double acc = 0.0;
  for (int m = 0; m < A.nm; ++m) acc = fma(src[(size_t)m * A.ns], cos(m * dphi), acc);
  A.uu[(((size_t)s * A.nphi + j) * A.ntau + lu) * A.numu + iu] = acc;
}
#endif  // !HD_RAD_SPHER


// ============================================================================
// IMS step of the Nakajima-Tanaka correction (DISORT 2.0 SECSCA / XIFUNC, STWL
// eqs. A.13-A.16), without the F0/(4 pi) factor: secondary scattering through
// the truncated forward peak, which delta-M (and so the TMS step) treats as
// exactly forward.  The slab above the user depth tu (unscaled; the user's
// layer lu_l down to tu) is replaced by its omega- and f-weighted averages;
// the peak's phase function P'' has moments 1 below nstr and
// g_l = <omega chi_l>/<omega f> from nstr on, and PSPIKE = 2 P'' - P''*P''
// (moments 2 g - g^2).  Same arithmetic as oracle/disort_rad_np.py's
// ims_correction / xi_func.  mu1 = |mu| of a downward user direction.
// ============================================================================
// mu0: the beam's cosine through the slab -- the true mu0, or under the pseudo-spherical
// beam the slab's mean cosine tu / ch(tu) (tms_sum); cos(Theta) in ct keeps the true mu0.
__device__ double ims_term(const RadArgs& A, long s, int nstr, double ct, double mu1, double mu0,
                           double tu, int lu_l) {
  constexpr double kTiny = 1.0e-4;
  const int L = A.nlyr, np = A.nprop, nm = A.nmom;
  if (nm < nstr) return 0.0;  // no truncation: f = 0
  const double* q0 = A.prop + (size_t)s * L * np;
  // dtau of solver layer lc above tu (harp layer L-1-lc); ssalb dithered as in setdis
  auto slab = [&](int lc, double& ssa) {
    const double* q = q0 + (size_t)(L - 1 - lc) * np;
    ssa = np > 1 ? q[1] : 0.0;
    if (ssa == 1.0) ssa = 1.0 - kDither;
    if (lc < lu_l) return q[0];
    const double d = tu - A.taus[(size_t)lc * A.ns + (s - A.s0)];
    return d > 0.0 ? d : 0.0;
  };
  double wsum = 0.0, fsum = 0.0, stau = 0.0;
  for (int lc = 0; lc <= lu_l; ++lc) {
    double ssa;
    const double dt = slab(lc, ssa);
    const double wt = ssa * dt;
    wsum += wt;
    fsum = fma(wt, q0[(size_t)(L - 1 - lc) * np + 1 + nstr], fsum);
    stau += dt;
  }
  if (!(wsum > kTiny) || !(fsum > kTiny) || !(stau > kTiny)) return 0.0;
  const double fw = fsum / stau;  // f-bar omega-bar
  // PSPIKE by the Legendre recurrence at cos(Theta)
  double ps = 1.0, p1 = 1.0, p2 = 0.0;
  for (int k = 1; k <= nm; ++k) {
    const double pk = ((2 * k - 1) * ct * p1 - (k - 1) * p2) / k;
    p2 = p1;
    p1 = pk;
    double wk = 1.0;
    if (k >= nstr) {
      double gs = 0.0;
      for (int lc = 0; lc <= lu_l; ++lc) {
        double ssa;
        const double dt = slab(lc, ssa);
        gs = fma(ssa * dt, q0[(size_t)(L - 1 - lc) * np + 1 + k], gs);
      }
      const double g = gs / fsum;
      wk = g * (2.0 - g);
    }
    ps = fma((2 * k + 1) * wk, pk, ps);
  }
  // xi(mu1, mu2, tu), mu2 = mu0 / (1 - f w)
  const double mu2 = mu0 / (1.0 - fw);
  const double a = 1.0 / mu2 - 1.0 / mu1;
  const double x = a * tu;
  const double e1 = exp(-tu / mu1);
  double xi;
  if (fabs(x) < 0.5) {
    double h = 0.0, term = 1.0, fact = 2.0;  // sum_{k>=2} (-1)^k (k-1)/k! x^(k-2)
    for (int k = 2; k < 24; ++k) {
      h += (k - 1) / fact * term;
      term *= -x;
      fact *= k + 1;
    }
    xi = e1 * tu * tu / (mu1 * mu2) * h;
  } else {
    xi = (e1 - exp(-tu / mu2) * (1.0 + x)) / (a * a * mu1 * mu2);
  }
  return fw * fw / (1.0 - fw) * ps * xi;
}

// ============================================================================
// Nakajima-Tanaka correction (DISORT 2.0 INTCOR): the TMS step (STWL eq. 68),
// exact single scattering (full moment series, omega/(1 - f omega)) minus the
// delta-M one (truncated series, omega'), both on the scaled depths, and for
// downward directions minus the IMS term (ims_term); added to uu
// ============================================================================
// the bracket of the correction at one direction (mu, phi [deg]) and user depth lu of
// solve s = s0 + sl with a beam (fb > 0, mu0 > 0); the correction is fb/(4 pi) times it
// kSpher: the beam at scaled depth t of layer lc is exp(-(top + lam (t - top_lc))) of
// sph_beam in place of exp(-t/mu0), so den = 1 + lam mu with the same series branch, and
// the IMS step takes the mean cosine of the slab above the user depth, tu / ch(tu), ch the
// unscaled slant depth, linear in tau inside the user's layer
__device__ __forceinline__ double tms_sum(const RadArgs& A, long s, int sl, int lu, double mu,
                                          double phi, double mu0, double fb, int nstr) {
  const int L = A.nlyr, np = A.nprop, nm = A.nmom;
  const double ph0 = A.phi0 ? A.phi0[s] : 0.0;
  const double ct = fma(-mu, mu0, sqrt(fmax(0.0, 1.0 - mu * mu)) *
                                      sqrt(fmax(0.0, 1.0 - mu0 * mu0)) *
                                      cos((phi - ph0) * (kPi / 180.0)));
  // user depth -> layer and scaled depth
  const double tu = user_tau(A, lu, sl);
  int lu_l = 0;
  while (lu_l < L - 1 && tu > A.taus[(size_t)(lu_l + 1) * A.ns + sl]) ++lu_l;
  double rmu0 = 1.0 / mu0;  // kSpher: the layer's secant, set per layer
  double acc = 0.0, tau_u = 0.0;
  for (int pass = 0; pass < 2; ++pass) {  // pass 0: scaled depth of the user level
    const int lo = pass == 0 ? lu_l : (mu > 0.0 ? lu_l : 0);
    const int hi = pass == 0 ? lu_l : (mu > 0.0 ? L - 1 : lu_l);
    for (int lc = lo; lc <= hi; ++lc) {
      const double* q = A.prop + ((size_t)s * L + (L - 1 - lc)) * np;
      const double tau = q[0];
      double ssa = np > 1 ? q[1] : 0.0;
      if (ssa == 1.0) ssa = 1.0 - kDither;
      const double f = nm >= nstr ? q[1 + nstr] : 0.0;
      const double taup = (1.0 - ssa * f) * tau;
      const double top = A.tauc[(size_t)lc * A.ns + sl];
      if (pass == 0) {
        const double ttop = A.taus[(size_t)lc * A.ns + sl];
        const double scale = tau > 0.0 ? taup / tau : 0.0;
        tau_u = top + fmin(fmax((tu - ttop) * scale, 0.0), taup);
        continue;
      }
      const double bot = top + taup;
      const double t1 = mu > 0.0 ? fmax(tau_u, top) : fmin(tau_u, bot);
      const double t2 = mu > 0.0 ? bot : top;
      double b0 = 0.0;  // the beam at depth t of this layer is exp(-(b0 + rmu0 t))
      if constexpr (kSpher) {
        const SphBeam sb = sph_beam(A, lc, sl, taup);
        rmu0 = sb.lam;
        b0 = fma(-sb.lam, top, sb.top);
      }
      // phase functions at cos(Theta): full series and delta-M truncated series
      double pa = 1.0, pm = 1.0;  // k = 0 terms: chi_0 = 1, (chi_0 - f)/(1 - f) = 1
      double p1 = 1.0, p2 = 0.0;
      const int kmax = nm > nstr - 1 ? nm : nstr - 1;
      for (int k = 1; k <= kmax; ++k) {
        const double pk = ((2 * k - 1) * ct * p1 - (k - 1) * p2) / k;
        p2 = p1;
        p1 = pk;
        const double chi = k <= nm ? q[1 + k] : 0.0;
        if (k <= nm) pa = fma((2 * k + 1) * chi, pk, pa);
        if (k < nstr) pm = fma((2 * k + 1) * (chi - f) / (1.0 - f), pk, pm);
      }
      const double om = ssa * (1.0 - f) / (1.0 - ssa * f);
      const double w = ssa * pa / (1.0 - f * ssa) - om * pm;
      // int_{t1}^{t2} e^{-t/mu0} e^{-(t - tau_u)/mu} dt/mu
      const double e1 = kSpher ? exp(-fma(t1, rmu0, b0) - (t1 - tau_u) / mu)
                              : exp(-t1 * rmu0 - (t1 - tau_u) / mu);
      const double den = fma(rmu0, mu, 1.0);
      const double x = den * (t2 - t1) / mu;
      double seg;
      if (fabs(x) < 0.5) {
        const double phx = x == 0.0 ? 1.0 : -expm1(-x) / x;
        seg = e1 * (t2 - t1) / mu * phx;
      } else {
        seg = (e1 - (kSpher ? exp(-fma(t2, rmu0, b0) - (t2 - tau_u) / mu)
                           : exp(-t2 * rmu0 - (t2 - tau_u) / mu))) / den;
      }
      acc = fma(w, seg, acc);
    }
  }
  if constexpr (kSpher) {
    if (mu < 0.0 && fb > 1.0e-4) {
      const double ttop = A.taus[(size_t)lu_l * A.ns + sl];
      const double dtl = A.taus[(size_t)(lu_l + 1) * A.ns + sl] - ttop;
      const double c0 = A.ch[(size_t)lu_l * A.ns + sl], c1 = A.ch[(size_t)(lu_l + 1) * A.ns + sl];
      const double chu = dtl > 0.0 ? fma(c1 - c0, fmin(fmax((tu - ttop) / dtl, 0.0), 1.0), c0) : c0;
      const double mub = chu > 0.0 ? fmin(tu / chu, 1.0) : mu0;
      acc -= ims_term(A, s, nstr, ct, -mu, mub, tu, lu_l);
    }
    return acc;
  }
  if (mu < 0.0 && fb > 1.0e-4) acc -= ims_term(A, s, nstr, ct, -mu, mu0, tu, lu_l);  // SECSCA: fbeam > tiny
  return acc;
}

#if !HD_RAD_SPHER
__global__ __launch_bounds__(256) void hd_rad_tms_kernel(RadArgs A, int nstr) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long n = (long)A.ns * A.nphi * A.ntau * A.numu;
  if (id >= n) return;
  const int sl = (int)(id % A.ns);
  long r = id / A.ns;
  const int iu = (int)(r % A.numu);
  r /= A.numu;
  const int lu = (int)(r % A.ntau);
  const int j = (int)(r / A.ntau);
  const long s = A.s0 + sl;
  const double mu0 = A.umu0 ? A.umu0[s] : 1.0;
  const double fb = A.fbeam ? A.fbeam[s] : 0.0;
  if (!(fb > 0.0 && mu0 > 0.0)) return;
  const double acc = tms_sum(A, s, sl, lu, A.umu[iu], A.phi[j], mu0, fb, nstr);
  A.uu[(((size_t)s * A.nphi + j) * A.ntau + lu) * A.numu + iu] += fb / (4.0 * kPi) * acc;
}
#endif  // !HD_RAD_SPHER

// ============================================================================
// ray epilogue (hd_solve_rays): user angle r of a solve is one outgoing ray with its
// own cosine and azimuth (shared, or the solve's column's own).  Per (solve, depth,
// ray): the azimuth sum at the ray's phi and, with corint, the Nakajima-Tanaka
// correction at the ray's (mu, phi) -- one evaluation per ray where the grid kernels
// do nphi * numu.  A bad cosine (not finite, 0, |mu| > 1: the user-angle kernels ran
// on 1 in its place) gives NaN and flags the solve.
// ============================================================================
__device__ __forceinline__ double ray_radiance(const RadArgs& A, int sl, int lu, int r,
                                               int nstr) {
  const long s = A.s0 + sl;
  const size_t ro = user_angle(A, s, r);
  const double mu = A.ray_umu[ro];
  if (!(mu != 0.0) || !(fabs(mu) <= 1.0)) {
    if (lu == 0) flag(A, s, kStBadInput);
    return __builtin_nan("");
  }
  const double phi = A.phi[ro];
  const double ph0 = A.phi0 ? A.phi0[s] : 0.0;
  const double dphi = (phi - ph0) * (kPi / 180.0);
  const double* src = A.radm + ((size_t)lu * A.numu + r) * A.nu + sl;
  double acc = 0.0;
  for (int m = 0; m < A.nm; ++m) acc = fma(src[(size_t)m * A.ns], cos(m * dphi), acc);
  if (A.corint && A.tauc) {
    const double mu0 = A.umu0 ? A.umu0[s] : 1.0;
    const double fb = A.fbeam ? A.fbeam[s] : 0.0;
    bool beam = fb > 0.0 && mu0 > 0.0;
    if constexpr (kSpher) beam = beam && sph_beam_on(A, sl);
    if (beam)
      acc = fma(fb / (4.0 * kPi), tms_sum(A, s, sl, lu, mu, phi, mu0, fb, nstr), acc);
  }
  return acc;
}

// BAND = false: one lane per (solve, depth, ray), solve fastest (the radm reads of a
// wave are contiguous), rad[s][lu][r] stored.
// BAND = true: one lane per (column, depth, ray), column fastest; the lane takes the
// chunk's solves of its column in ascending wave order and carries
//   brad[c][lu][r] = fma(weight[w], rad[w][c][lu][r], brad[c][lu][r])
// from 0 at w = 0 on, through memory between chunks: one fma per wave in wave order
// whatever the chunk size (hd_band_sum's sequence, no atomics); rad stored if given
template <bool BAND>
__global__ __launch_bounds__(256) void hd_rad_ray_kernel(RadArgs A, int nstr) {
  const int nx = BAND ? A.ncol : A.ns;
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long)nx * A.ntau * A.numu) return;
  const int x = (int)(id % nx);
  const long q = id / nx;
  const int r = (int)(q % A.numu);
  const int lu = (int)(q / A.numu);
  if constexpr (!BAND) {
    A.rad[((size_t)(A.s0 + x) * A.ntau + lu) * A.numu + r] = ray_radiance(A, x, lu, r, nstr);
  } else {
    int w = (int)((A.s0 - x + A.ncol - 1) / A.ncol);  // first wave with w ncol + x >= s0
    long s = (long)w * A.ncol + x;
    const long s1 = A.s0 + A.ns;
    if (s >= s1) return;  // no solve of this column in the chunk
    const size_t o = ((size_t)x * A.ntau + lu) * A.numu + r;
    double acc = w == 0 ? 0.0 : A.brad[o];
    for (; s < s1; s += A.ncol, ++w) {
      const double v = ray_radiance(A, (int)(s - A.s0), lu, r, nstr);
      if (A.rad) A.rad[((size_t)s * A.ntau + lu) * A.numu + r] = v;
      acc = fma(A.weight[w], v, acc);
    }
    A.brad[o] = acc;
  }
}

#if !HD_RAD_SPHER
__global__ __launch_bounds__(256) void hd_ray_cosines_kernel(const double* umu, double* out,
                                                             long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double mu = umu[i];
  out[i] = (mu != 0.0 && fabs(mu) <= 1.0) ? mu : 1.0;
}

hipError_t launch_ray_cosines(const double* umu, double* out, long n, hipStream_t stream) {
  hipLaunchKernelGGL(hd_ray_cosines_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     stream, umu, out, n);
  return hipGetLastError();
}
#endif  // !HD_RAD_SPHER

// ============================================================================
// host side
// ============================================================================
// called once per device, under hd_api.cpp's global table lock (ensure_rad_tables),
// so the function-static staging buffers below are never filled concurrently
hipError_t upload_rad_tables(const QuadHost* per_nn) {
  static RadTabs<1, kMaxRegNN> c;  // ~60 KB: keep off the stack
  static RadCoef coef;
  fill_rad(c, per_nn);
  fill_rad_coef(coef);
  hipError_t e = hipSuccess;
#if !HD_RAD_SPHER
  // the nstr 18..32 instantiations keep their own tables (hd_rad_wide.hip), and so do the
  // pseudo-spherical ones of nstr <= 16 (hd_rad_spher.hip)
  e = wide::upload_rad_tables(per_nn);
  if (e != hipSuccess) return e;
  e = spher::upload_rad_tables(per_nn);
  if (e != hipSuccess) return e;
#endif
  e = hipMemcpyToSymbol(HIP_SYMBOL(c_rcoef), &coef, sizeof(RadCoef));
  if (e != hipSuccess) return e;
  return hipMemcpyToSymbol(HIP_SYMBOL(c_rad), &c, sizeof(c));
}

// the one-lane kernels of this file at one NN <= kMaxRegNN (null above it: the team and
// rolled launchers run there) and the ray epilogues of every nstr, in this translation
// unit's form
RegKernels reg_kernels(int nn) {
  RegKernels k{};
  k.ray = hd_rad_ray_kernel<false>;
  k.ray_band = hd_rad_ray_kernel<true>;
  (void)dispatch_nn<1, kMaxRegNN>(nn, [&](auto NN) {
    k.layer = hd_rad_layer_kernel<NN>;
    k.sweep = hd_rad_sweep_kernel<NN>;
    k.cst = hd_rad_const_kernel<NN>;
    k.flux = hd_rad_flux_kernel<NN>;
    k.user_map = hd_rad_user_map_kernel<NN>;
    return hipSuccess;
  });
  return k;
}

#if !HD_RAD_SPHER
// HD_RAD_USER=rolled: nstr 18..32 user angles by the one-lane-per-(unit, angle) kernel
static bool rad_user_rolled() {
  static const bool v = [] {
    const char* e = ab_env("HD_RAD_USER");
    return e && std::strcmp(e, "rolled") == 0;
  }();
  return v;
}

// One chunk of the intensity path, nstr 2..32.  Each stage is the one-lane kernel of
// this file (reg: nstr <= 16), or at nstr 18..32 the team launcher (hd_team_mfma.hip)
// or the rolled one-lane launcher (hd_rad_wide.hip).
hipError_t launch_rad_chunk(int nn, const RadArgs& a, bool radiances, hipStream_t st) {
  if (nn < 1 || nn > kRadMaxNN) return hipErrorInvalidValue;
  const bool reg = nn <= kMaxRegNN;
  // the pseudo-spherical beam (a.chp given): the paired-ray call at nstr <= 16 only, with
  // hd_spher_kernel's three arrays (the prologue ran with ch requested)
  const bool spher = a.chp != nullptr;
  if (spher && !(reg && a.ray_umu && a.lam && a.ch)) return hipErrorInvalidValue;
  const RegKernels k = spher ? spher::reg_kernels(nn) : reg_kernels(nn);
  // the launchers of the other sources return (and clear) their launch error: keep the first
  hipError_t err = hipSuccess;
  auto keep = [&](hipError_t e) {
    if (err == hipSuccess) err = e;
  };
  const unsigned ns_b = (unsigned)((a.ns + 255) / 256);
  hipLaunchKernelGGL(hd_rad_taus_kernel, dim3(ns_b), dim3(256), 0, st, a);
  const unsigned nb1 = (unsigned)(((a.nu + 63) / 64) *
                                  ((a.nlyr + kLayersPerBlockR - 1) / kLayersPerBlockR));
  if (reg) {
    hipLaunchKernelGGL(k.layer, dim3(nb1), dim3(kLayerBlockR), 0, st, a);
    hipLaunchKernelGGL(k.sweep, dim3((unsigned)((a.nu + 63) / 64)), dim3(64), 0, st, a);
  } else {
    keep(launch_rad_team_layer(nn, a, st));
    keep(launch_rad_team_sweep(nn, a, st));
  }
  const bool rad = radiances && a.numu > 0 && a.nphi > 0;
  // nstr 18..32 with radiances: the team user-angle kernel also forms the layers'
  // homogeneous constants (hd_team_mfma.hip), so the const kernel does not run
  const bool team_user =
      !reg && rad && a.numu <= rad_layer_record_doubles(nn) && !rad_user_rolled() &&
      a.umu_stride == 0;  // a team's four units share one user cosine: per-column rays
                          // take the one-lane user kernel
  // nstr <= 16 with radiances: the const kernel writes the angle-independent maps and
  // the user angles run hd_rad_user_map_kernel
  const bool umap = reg && rad;
  RadArgs ac = a;
  ac.umap = umap ? 1 : 0;
  if (team_user) {
    keep(launch_rad_team_user(nn, a, st));
  } else if (reg) {
    const long nc = (long)a.ns * a.nlyr;
    hipLaunchKernelGGL(k.cst, dim3((unsigned)((nc + 255) / 256), (unsigned)a.nm), dim3(256), 0, st,
                       ac);
  } else {
    keep(wide::launch_rad_const(nn, ac, st));
  }
  const long nf = (long)a.ns * a.ntau;
  if (a.flux) {  // optional along rays only
    if (reg)
      hipLaunchKernelGGL(k.flux, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, a);
    else
      keep(wide::launch_rad_flux(nn, a, st));
  }
  if (rad) {
    const long nr = (long)a.ns * a.numu;
    if (umap)
      hipLaunchKernelGGL(k.user_map, dim3((unsigned)((nr + 63) / 64), (unsigned)a.nm), dim3(64), 0,
                         st, ac);
    else if (!team_user)
      keep(wide::launch_rad_user(nn, a, st));
    if (a.ray_umu) {
      const long ny = (long)a.ntau * a.numu;
      void (*ray)(RadArgs, int) = a.brad ? k.ray_band : k.ray;
      const long nx = a.brad ? a.ncol : a.ns;
      hipLaunchKernelGGL(ray, dim3((unsigned)((nx * ny + 255) / 256)), dim3(256), 0, st, a,
                         2 * nn);
      keep(hipGetLastError());
      return err;
    }
    const long na = (long)a.ns * a.nphi * a.ntau * a.numu;
    hipLaunchKernelGGL(hd_rad_azimuth_kernel, dim3((unsigned)((na + 255) / 256)), dim3(256), 0,
                       st, a);
    if (a.corint && a.tauc)
      hipLaunchKernelGGL(hd_rad_tms_kernel, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, st,
                         a, 2 * nn);
  }
  keep(hipGetLastError());
  return err;
}
#endif  // !HD_RAD_SPHER

#if HD_RAD_SPHER
}  // namespace spher
#endif
}  // namespace hd
