// hd_rad_lane.hpp -- the intensity-path kernels that run one lane per problem at every
// nstr: the layers' homogeneous constants and the fluxes at the user depths, with the
// small device helpers of the one-lane kernels.  This body is compiled in two forms,
// chosen by HD_UNROLL_NN (hd_device.hpp) alone: hd_rad.hip includes it with the NN-loops
// unrolled and instantiates NN 1..8 (matrices in registers); hd_rad_wide.hip includes
// it with them rolled, in hd::wide, and instantiates NN 9..16 (matrices in private
// memory).  Include it inside the namespace, after hd_rad.hpp and after the source's
// own tables in constant memory, RadTabs<LO, HI> c_rad and RadCoef c_rcoef, and its constant
// bool kSpher (the pseudo-spherical beam: hd_rad_spher.hip alone sets it).
// No include guard: one inclusion per translation unit.

namespace {

template <int NN>
__device__ __forceinline__ const Quad<NN>& quad_r() {
  return rad_tabs<NN>(c_rad).q;
}
template <int NN>
__device__ __forceinline__ const RadTab<NN>& tab_r() {
  return rad_tabs<NN>(c_rad).t;
}

// Y_m^m(x) = seed_m (1 - x^2)^(m/2)
__device__ __forceinline__ double ylm_seed(int m, double x) {
  const double s = sqrt(fmax(0.0, 1.0 - x * x));
  double p = c_rcoef.seed[m];
  for (int i = 0; i < m; ++i) p *= s;
  return p;
}

// Y_l^m(x), l < N (compile-time l, runtime m)
template <int N>
__device__ __forceinline__ void ylm_row(int m, double x, double (&y)[N]) {
  const double seed = ylm_seed(m, x);
  double y1 = 0.0, y2 = 0.0;
#pragma unroll
  for (int l = 0; l < N; ++l) {
    const double v =
        l < m ? 0.0 : (l == m ? seed : fma(c_rcoef.ra[m][l] * x, y1, -c_rcoef.rb[m][l] * y2));
    y[l] = v;
    y2 = y1;
    y1 = v;
  }
}

__device__ __forceinline__ void flag(const RadArgs& A, long s, int st) {
  if (st) {
    atomicOr(&A.status[s], st);
    if (st & 0x0F) atomicOr(A.anyerr, 1);
  }
}

}  // namespace

// ============================================================================
// per-(unit, layer) homogeneous constants from the level intensities
//   C+ = (X^-1 s_top + Y^-1 d_top)/2,  C- = (X^-1 s_bot - Y^-1 d_bot)/2
//   X^-1 = V^T L^-1 diag(g),  Y^-1 = -K^-1 V^T L^T diag(g)
// ============================================================================
template <int NN>
__device__ __forceinline__ void load_layer(const RadArgs& A, int lc, int u, double (&lch)[NN][NN],
                                           double (&rd)[NN], double (&v)[NN][NN],
                                           double (&kk)[NN]) {
  using R = RadRec<NN>;
  const size_t nu = A.nu;
  const size_t rs = RadAt<NN>::stride(nu);
  const double* rr = RadAt<NN>::rec(A.rrd, R::size, lc, nu, u);
  int e = R::L;
HD_UNROLL_NN
  for (int i = 0; i < NN; ++i)
HD_UNROLL_NN
    for (int k = 0; k <= i; ++k) lch[i][k] = rr[(e++) * rs];
HD_UNROLL_NN
  for (int i = 0; i < NN; ++i) rd[i] = 1.0 / lch[i][i];
HD_UNROLL_NN
  for (int i = 0; i < NN; ++i)
HD_UNROLL_NN
    for (int j = 0; j < NN; ++j) v[i][j] = rr[(R::V + i * NN + j) * rs];
HD_UNROLL_NN
  for (int j = 0; j < NN; ++j) kk[j] = rr[(R::K + j) * rs];
}

// kSpher (a constant of the including source; nstr <= 16 in hd_rad_spher.hip only): the
// beam of the layer is exp(-(top + lam t)) of sph_beam (hd_rad.hpp) in place of
// exp(-(tauc + t)/mu0)
template <int NN>
#ifndef HD_RAD_CONST_WAVES
#define HD_RAD_CONST_WAVES 1
#endif
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(HD_RAD_CONST_WAVES)))
void hd_rad_const_kernel(RadArgs A) {
  using R = RadRec<NN>;
  const Quad<NN>& Qc = quad_r<NN>();
  // grid.y = mode (uniform per block: the mode-m tables of the maps are scalar loads)
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long)A.ns * A.nlyr) return;
  const int lc = (int)(id / A.ns);
  const int sl = (int)(id - (long)lc * A.ns);
  const int m = blockIdx.y;
  const int u = m * A.ns + sl;
  const long s = A.s0 + sl;
  const size_t nu = A.nu;
  const size_t rs = RadAt<NN>::stride(nu);
  double lch[NN][NN], rd[NN], v[NN][NN], kk[NN];
  load_layer<NN>(A, lc, u, lch, rd, v, kk);
  const double* rr = RadAt<NN>::rec(A.rrd, R::size, lc, nu, u);
  const double bt = rr[R::Bt * rs], slope = rr[R::Sl * rs], taup = rr[R::Tp * rs];
  const double mu0 = A.umu0 ? A.umu0[s] : 1.0;
  const double fb = A.fbeam ? A.fbeam[s] : 0.0;
  double rmu0 = (fb > 0.0 && mu0 > 0.0) ? 1.0 / mu0 : 0.0;
  double chtop = 0.0;  // kSpher: slant depth of the beam at the layer top
  if constexpr (kSpher) {
    const SphBeam sb = sph_beam(A, lc, sl, taup);
    rmu0 = sph_beam_on(A, sl) ? sb.lam : 0.0;
    chtop = sb.top;
  }
  double cp[NN], cm[NN];
HD_UNROLL_NN
  for (int side = 0; side < 2; ++side) {  // 0: layer top, 1: layer bottom
    const double t = side ? taup : 0.0;
    const double eb = exp(-t * rmu0);
    const double b2 = 2.0 * fma(slope, t, bt);
    const double* lv = RadElemMajor::rec(A.lev, RadLev<NN>::size, lc + side, nu, u);
    double xs[NN], yd[NN];
HD_UNROLL_NN
    for (int i = 0; i < NN; ++i) {
      const double ipl = lv[(RadLev<NN>::Ip + i) * nu], imi = lv[(RadLev<NN>::Im + i) * nu];
      const double zp = rr[(R::Zp + i) * rs], zm = rr[(R::Zm + i) * rs], h = rr[(R::H + i) * rs];
      xs[i] = Qc.g[i] * (ipl + imi - (zp + zm) * eb - b2);
      yd[i] = Qc.g[i] * (ipl - imi - (zp - zm) * eb - 2.0 * slope * h);
    }
    lower_solve<NN>(lch, rd, xs);
    double ly[NN];
HD_UNROLL_NN
    for (int i = 0; i < NN; ++i) {  // L^T yd
      double a = 0.0;
HD_UNROLL_NN
      for (int k = i; k < NN; ++k) a = fma(lch[k][i], yd[k], a);
      ly[i] = a;
    }
HD_UNROLL_NN
    for (int j = 0; j < NN; ++j) {
      double a = 0.0, b = 0.0;
HD_UNROLL_NN
      for (int i = 0; i < NN; ++i) {
        a = fma(v[i][j], xs[i], a);
        b = fma(v[i][j], ly[i], b);
      }
      b = kk[j] > 0.0 ? -b / kk[j] : 0.0;
      if (side == 0) cp[j] = 0.5 * (a + b);
      else cm[j] = 0.5 * (a - b);
    }
  }
  double* co = RadElemMajor::rec(A.cst, RadCst<NN>::size, lc, nu, u);
HD_UNROLL_NN
  for (int j = 0; j < NN; ++j) {
    co[(RadCst<NN>::Cp + j) * nu] = cp[j];
    co[(RadCst<NN>::Cm + j) * nu] = cm[j];
  }
  if constexpr (NN <= kMaxRegNN) {  // nstr <= 16: with radiances, the user-angle maps
    if (A.umap) {
      // The user-angle integration's angle-independent part, per (unit, layer).  For a
      // user cosine mu with Y_l^m(mu) = yu_l, split by the parity of l + m into
      // ye (l = 2 l2 + par) and yo (l = 2 l2 + 1 - par), par = m & 1:
      //   ce = Me ye,  Me = V^T L^T D Lam_e^T G_e      (the even source projection)
      //   cx = Mo yo,  Mo = V^T L^-1 D Lam_o^T G_o     (the odd one)
      //   beam amplitude  ab = abe . ye + abo . yo,  thermal  we = tve . ye, wo = tvo . yo
      // with D = diag(sqrt(w/mu)), Lam[l][i] = Y_l^m(mu_i), G = diag(gl/2) -- what
      // hd_rad_user_kernel forms per (unit, angle) from L, V and the moments, regrouped so
      // that it is formed once per (unit, layer) and each angle pays 2 NN^2 FMAs.
      // Written over the layer's rsw and bsub records: RadMap (hd_rad_layout.hpp).
      using M = RadMap<NN>;
      static_assert(M::Me == 0 && M::Mo == 0, "Me / Mo open their records");
      constexpr int N = 2 * NN;
      double* m1 = RadAt<NN>::rec(A.rsw, RadOps<NN>::size, lc, nu, u);
      double* m2 = RadAt<NN>::rec(A.bsub, RadBsub<NN>::size, lc, nu, u);
      const int L = A.nlyr, np = A.nprop, nmo = A.nmom;
      const double* q = A.prop + ((size_t)s * L + (L - 1 - lc)) * np;
      double ssa = np > 1 ? q[1] : 0.0;
      if (ssa == 1.0) ssa = 1.0 - kDither;
      const double f = nmo >= N ? q[1 + N] : 0.0;
      const double om = ssa * (1.0 - f) / (1.0 - ssa * f);
      const double rf = om / (1.0 - f);
      bool beam = fb > 0.0 && mu0 > 0.0;
      if constexpr (kSpher) beam = beam && sph_beam_on(A, sl);
      double y0[N];
      ylm_row<N>(m, beam ? mu0 : 0.0, y0);
      const double fac = (m == 0 ? 1.0 : 2.0) * fb / (4.0 * kPi);
      double eb;
      if constexpr (kSpher) eb = beam ? fac * exp(-chtop) : 0.0;
      else eb = beam ? fac * exp(-A.tauc[(size_t)lc * A.ns + sl] * rmu0) : 0.0;
      const int par = m & 1;
      const double* lam = &tab_r<NN>().lam[m][0][0];
      double zs[NN], zd[NN], hh[NN];
HD_UNROLL_NN
      for (int i = 0; i < NN; ++i) {
        const double zp = rr[(R::Zp + i) * rs], zm = rr[(R::Zm + i) * rs];
        zs[i] = beam ? Qc.w[i] * (zp + zm) : 0.0;
        zd[i] = beam ? Qc.w[i] * (zp - zm) : 0.0;
        hh[i] = Qc.w[i] * rr[(R::H + i) * rs];
      }
#pragma nounroll
      for (int l2 = 0; l2 < NN; ++l2) {
HD_UNROLL_NN
        for (int half = 0; half < 2; ++half) {  // 0: even part, 1: odd part
          const int l = 2 * l2 + (half ? 1 - par : par);
          const double chi = l == 0 ? 1.0 : (l <= nmo ? q[1 + l] : 0.0);
          const double gl = (2 * l + 1) * (chi - f) * rf;
          const double gh = 0.5 * gl;
          const double yl0 = ((l + m) & 1) ? -y0[l] : y0[l];  // Y_l^m(-mu0)
          double x[NN], sb = 0.0, st = 0.0;
HD_UNROLL_NN
          for (int i = 0; i < NN; ++i) {
            const double lm = lam[l * NN + i];
            x[i] = Qc.sd[i] * (gh * lm);
            sb = fma(half ? zd[i] : zs[i], lm, sb);
            st = half ? fma(hh[i], lm, st) : fma(Qc.w[i], lm, st);
          }
          double y[NN];
          if (half == 0) {  // L^T x
HD_UNROLL_NN
            for (int k = 0; k < NN; ++k) {
              double a = 0.0;
HD_UNROLL_NN
              for (int i = k; i < NN; ++i) a = fma(lch[i][k], x[i], a);
              y[k] = a;
            }
          } else {  // L^-1 x
HD_UNROLL_NN
            for (int i = 0; i < NN; ++i) {
              double t = x[i];
HD_UNROLL_NN
              for (int k = 0; k < i; ++k) t = fma(-lch[i][k], y[k], t);
              y[i] = t * rd[i];
            }
          }
          double* mo = half ? m2 : m1;  // Mo in bsub, Me in rsw: both at element 0
HD_UNROLL_NN
          for (int j = 0; j < NN; ++j) {
            double a = 0.0;
HD_UNROLL_NN
            for (int i = 0; i < NN; ++i) a = fma(v[i][j], y[i], a);
            mo[(size_t)(j * NN + l2) * rs] = a;
          }
          const double abv = fma(eb * gl, yl0, gh * sb);
          m1[(size_t)((half ? M::Abo : M::Abe) + l2) * rs] = abv;
          if (half == 0) m1[(size_t)(M::Tve + l2) * rs] = gh * st;
          else m2[(size_t)(M::Tvo + l2) * rs] = gh * st;
        }
      }
    }
  }
}


// ============================================================================
// fluxes at the user depths from the m = 0 field (unit u = sl)
// ============================================================================
// kSpher: the particular solution and the direct term mu0 F0 exp(-(top + lam t)) on
// sph_beam's secant and slant depth
template <int NN>
__global__ __launch_bounds__(256) void hd_rad_flux_kernel(RadArgs A) {
  using R = RadRec<NN>;
  const Quad<NN>& Qc = quad_r<NN>();
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long)A.ns * A.ntau) return;
  const int lu = (int)(id / A.ns);
  const int sl = (int)(id - (long)lu * A.ns);
  const int u = sl;  // mode 0
  const long s = A.s0 + sl;
  const int L = A.nlyr;
  const size_t nu = A.nu;
  const size_t rs = RadAt<NN>::stride(nu);
  const double tu = user_tau(A, lu, sl);
  int lc = 0;
  while (lc < L - 1 && tu > A.taus[(size_t)(lc + 1) * A.ns + sl]) ++lc;
  const double ttop = A.taus[(size_t)lc * A.ns + sl];
  const double tau = A.taus[(size_t)(lc + 1) * A.ns + sl] - ttop;
  double lch[NN][NN], rd[NN], v[NN][NN], kk[NN];
  load_layer<NN>(A, lc, u, lch, rd, v, kk);
  const double* rr = RadAt<NN>::rec(A.rrd, R::size, lc, nu, u);
  const double bt = rr[R::Bt * rs], slope = rr[R::Sl * rs], taup = rr[R::Tp * rs];
  const double scale = tau > 0.0 ? taup / tau : 0.0;
  const double t = fmin(fmax((tu - ttop) * scale, 0.0), taup);
  const double mu0 = A.umu0 ? A.umu0[s] : 1.0;
  const double fb = A.fbeam ? A.fbeam[s] : 0.0;
  bool beam = fb > 0.0 && mu0 > 0.0;
  double rmu0 = beam ? 1.0 / mu0 : 0.0;
  double chtop = 0.0;  // kSpher: slant depth of the beam at the layer top
  if constexpr (kSpher) {
    beam = beam && sph_beam_on(A, sl);
    const SphBeam sb = sph_beam(A, lc, sl, taup);
    rmu0 = beam ? sb.lam : 0.0;
    chtop = sb.top;
  }
  const double* co = RadElemMajor::rec(A.cst, RadCst<NN>::size, lc, nu, u);
  double al[NN], be[NN];
HD_UNROLL_NN
  for (int j = 0; j < NN; ++j) {
    const double a = co[(RadCst<NN>::Cp + j) * nu] * exp(-kk[j] * t);
    const double b = co[(RadCst<NN>::Cm + j) * nu] * exp(-kk[j] * (taup - t));
    al[j] = a + b;
    be[j] = kk[j] * (a - b);
  }
  double gs[NN], gd[NN];
HD_UNROLL_NN
  for (int i = 0; i < NN; ++i) {  // V al, V (k be)
    double a = 0.0, b = 0.0;
HD_UNROLL_NN
    for (int j = 0; j < NN; ++j) {
      a = fma(v[i][j], al[j], a);
      b = fma(v[i][j], be[j], b);
    }
    gs[i] = a;
    gd[i] = b;
  }
HD_UNROLL_NN
  for (int i = NN - 1; i >= 0; --i) {  // gs <- L gs (rows bottom-up, in place)
    double a = 0.0;
HD_UNROLL_NN
    for (int k = 0; k <= i; ++k) a = fma(lch[i][k], gs[k], a);
    gs[i] = a;
  }
  lower_t_solve<NN>(lch, rd, gd);  // g (I+ - I-)_hom = -L^-T V K be
  const double eb = exp(-t * rmu0);
  const double bb = fma(slope, t, bt);
  double up = 0.0, dn = 0.0;
HD_UNROLL_NN
  for (int i = 0; i < NN; ++i) {
    const double zp = rr[(R::Zp + i) * rs], zm = rr[(R::Zm + i) * rs], h = rr[(R::H + i) * rs];
    const double ipl = 0.5 * (gs[i] - gd[i]) + Qc.g[i] * (zp * eb + bb + slope * h);
    const double imi = 0.5 * (gs[i] + gd[i]) + Qc.g[i] * (zm * eb + bb - slope * h);
    up = fma(Qc.g[i], ipl, up);
    dn = fma(Qc.g[i], imi, dn);
  }
  up *= 2.0 * kPi;
  dn *= 2.0 * kPi;
  if constexpr (kSpher) {
    // (user depths only: at the layer boundaries hd_solve_rays_spher takes the fluxes from
    // the flux solve, where the level below a layer of zero depth has its own ch')
    if (beam) dn += fb * mu0 * exp(-fma(rmu0, t, chtop));
  } else {
    if (beam) dn += fb * mu0 * exp(-(A.tauc[(size_t)lc * A.ns + sl] + t) * rmu0);
  }
  double* fo = A.flux + ((size_t)s * A.ntau + (A.ntau - 1 - lu)) * 2;
  fo[0] = up;
  fo[1] = dn;
  if (!isfinite(up + dn)) flag(A, s, kStNonFinite);
}

