// hd_rad_wide.hip -- the one-lane intensity-path kernels of nstr 18..32 (NN 9..16),
// with their NN-loops rolled: one lane per problem as at nstr <= 16, the per-lane
// NN x NN matrices in private memory instead of registers.  It is the coverage path of
// radiances at large nstr (the layer setup, the sweep and, where it applies, the user
// angles run on the team kernels of hd_team_mfma.hip).  Symbols live in hd::wide.
//
//   hd_rad_const_kernel<NN>  hd_rad_lane.hpp, rolled
//   hd_rad_flux_kernel<NN>   hd_rad_lane.hpp, rolled
//   hd_rad_user_kernel<NN>   per (unit, user angle): source-function integration
//                            along the ray through every layer       [c_usrint]
//
// The records are unit-contiguous at these sizes (RadAt, hd_rad_layout.hpp).
#define HD_UNROLL_NN _Pragma("nounroll")  // before hd_device.hpp: its helpers roll too
#include <cmath>

#include "hd_rad.hpp"

namespace hd {
namespace wide {

namespace {

__constant__ RadTabs<kMaxRegNN + 1, kRadMaxNN> c_rad;  // quadrature, Y_l^m table of NN 9..16
__constant__ RadCoef c_rcoef;                          // the Y_l^m recurrence coefficients
constexpr bool kSpher = false;  // the rolled kernels have no pseudo-spherical form

}  // namespace

// quad_r / tab_r / ylm_row / flag, hd_rad_const_kernel and hd_rad_flux_kernel, rolled
#include "hd_rad_lane.hpp"

// ============================================================================
// per-(unit, user angle) source-function integration along the ray
// ============================================================================
template <int NN>
// HD_RAD_USER_WAVES: waves per SIMD the one-lane user-angle kernel is compiled for
#ifndef HD_RAD_USER_WAVES
#define HD_RAD_USER_WAVES 1
#endif
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(HD_RAD_USER_WAVES)))
void hd_rad_user_kernel(RadArgs A) {
  constexpr int N = 2 * NN;
  using R = RadRec<NN>;
  using C = RadCst<NN>;
  const Quad<NN>& Qc = quad_r<NN>();
  // grid.y = mode (uniform per block: the mode-m tables are scalar loads);
  // user angle fastest inside a block: the lanes of one unit read the same
  // layer records (one cache segment per unit instead of one per angle)
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long)A.ns * A.numu) return;
  const int sl = (int)(id / A.numu);
  const int iu = (int)(id - (long)sl * A.numu);
  const int m = blockIdx.y;
  const int u = m * A.ns + sl;
  const long s = A.s0 + sl;
  const int L = A.nlyr, np = A.nprop, nm = A.nmom;
  const size_t nu = A.nu;
  const size_t rs = RadAt<NN>::stride(nu);
  const double muu = user_mu(A, s, iu);
  const double mu0 = A.umu0 ? A.umu0[s] : 1.0;
  const double fb = A.fbeam ? A.fbeam[s] : 0.0;
  const bool beam = fb > 0.0 && mu0 > 0.0;
  const double rmu0 = beam ? 1.0 / mu0 : 0.0;
  const bool therm = A.planck && m == 0;
  const double fac = (m == 0 ? 1.0 : 2.0) * fb / (4.0 * kPi);
  double yu[N], y0[N];
  ylm_row<N>(m, muu, yu);
  ylm_row<N>(m, beam ? mu0 : 0.0, y0);
#pragma nounroll
  for (int l = 0; l < N; ++l) y0[l] = ((l + m) & 1) ? -y0[l] : y0[l];  // Y_l^m(-mu0)
  const double* lam = &tab_r<NN>().lam[m][0][0];
  const bool up = muu > 0.0;

  double cur;
  if (up) {
    cur = 0.0;
    if (m == 0) {
      const double* lv = RadElemMajor::rec(A.lev, RadLev<NN>::size, L, nu, u);
      double fdn = 0.0;
#pragma nounroll
      for (int i = 0; i < NN; ++i)
        fdn = fma(Qc.g[i] * Qc.g[i], lv[(RadLev<NN>::Im + i) * nu], fdn);
      fdn *= 2.0 * kPi;
      const double alb = A.albedo ? A.albedo[s] : 0.0;
      if (beam) {
        const double tb = A.tauc[(size_t)(L - 1) * A.ns + sl] +
                          RadAt<NN>::rec(A.rrd, R::size, L - 1, nu, u)[R::Tp * rs];
        fdn += fb * mu0 * exp(-tb * rmu0);
      }
      cur = alb / kPi * fdn + (A.planck ? (1.0 - alb) * A.planckv[(size_t)(L + 1) * A.ns + sl]
                                        : 0.0);
    }
  } else {
    cur = 0.0;
    if (m == 0) {
      cur = A.fisot ? A.fisot[s] : 0.0;
      if (A.planck) cur += A.planckv[(size_t)(L + 2) * A.ns + sl];
    }
  }
  int k = up ? A.ntau - 1 : 0;
  double chk = 0.0;
  for (int step = 0; step < L; ++step) {
    const int lc = up ? L - 1 - step : step;
    const double ttop = A.taus[(size_t)lc * A.ns + sl];
    const double tbot = A.taus[(size_t)(lc + 1) * A.ns + sl];
    // ---- delta-M moments of this layer, mode-m phase row at muu ----
    const double* q = A.prop + ((size_t)s * L + (L - 1 - lc)) * np;
    double ssa = np > 1 ? q[1] : 0.0;
    if (ssa == 1.0) ssa = 1.0 - kDither;
    const double f = nm >= N ? q[1 + N] : 0.0;
    const double om = ssa * (1.0 - f) / (1.0 - ssa * f);
    const double rf = om / (1.0 - f);
    double cue[NN], cuo[NN];
    double x0 = 0.0;
    double gy[N];
#pragma nounroll
    for (int l = 0; l < N; ++l) {
      const double chi = l == 0 ? 1.0 : (l <= nm ? q[1 + l] : 0.0);
      const double gl = (2 * l + 1) * (chi - f) * rf;
      gy[l] = 0.5 * gl * yu[l];
      x0 = fma(gl * yu[l], y0[l], x0);
    }
    // even/odd parts in l + m: m is uniform per block, so is the branch
    auto lsum = [&](int par) {
#pragma nounroll
      for (int i = 0; i < NN; ++i) {
        double e = 0.0, o = 0.0;
#pragma nounroll
        for (int l2 = 0; l2 < NN; ++l2) {
          e = fma(gy[2 * l2 + par], lam[(2 * l2 + par) * NN + i], e);
          o = fma(gy[2 * l2 + 1 - par], lam[(2 * l2 + 1 - par) * NN + i], o);
        }
        cue[i] = e;
        cuo[i] = o;
      }
    };
    if (m & 1) lsum(1);
    else lsum(0);
    const double* rr = RadAt<NN>::rec(A.rrd, R::size, lc, nu, u);
    const double bt = rr[R::Bt * rs], slope = rr[R::Sl * rs], taup = rr[R::Tp * rs];
    // ce = V^T L^T (sd cue), co = -k V^T L^-1 (sd cuo); L and V streamed from the
    // record (each element used once), not held in registers
    double a1[NN], b1[NN];
#pragma nounroll
    for (int i = 0; i < NN; ++i) {
      a1[i] = 0.0;
      b1[i] = Qc.sd[i] * cuo[i];
    }
#pragma nounroll
    for (int i = 0; i < NN; ++i) {  // row i of L: a1 += L[i][:]^T (sd cue)_i ; b1 forward subst.
      const double* li = rr + (size_t)(R::L + i * (i + 1) / 2) * rs;
      const double ce_i = Qc.sd[i] * cue[i];
      double t = b1[i];
#pragma nounroll
      for (int k2 = 0; k2 < i; ++k2) {
        const double l = li[k2 * rs];
        a1[k2] = fma(l, ce_i, a1[k2]);
        t = fma(-l, b1[k2], t);
      }
      const double d = li[i * rs];
      a1[i] = fma(d, ce_i, a1[i]);
      b1[i] = t / d;
    }
    const double* co = RadElemMajor::rec(A.cst, C::size, lc, nu, u);
    const double* vr = rr + (size_t)R::V * rs;
    double kk[NN], hpl[NN], hmi[NN];
#pragma nounroll
    for (int j = 0; j < NN; ++j) {
      hpl[j] = hmi[j] = 0.0;
      kk[j] = rr[(R::K + j) * rs];
    }
#pragma nounroll
    for (int i = 0; i < NN; ++i)
#pragma nounroll
      for (int j = 0; j < NN; ++j) {
        const double vij = vr[(i * NN + j) * rs];
        hpl[j] = fma(vij, a1[i], hpl[j]);  // ce
        hmi[j] = fma(vij, b1[i], hmi[j]);  // V^T b1
      }
#pragma nounroll
    for (int j = 0; j < NN; ++j) {
      const double ce = hpl[j], cx = -kk[j] * hmi[j];
      hpl[j] = co[(C::Cp + j) * nu] * (ce + cx);
      hmi[j] = co[(C::Cm + j) * nu] * (ce - cx);
    }
    double ab = 0.0, a0 = 0.0, a1t = 0.0;
    if (beam) {
      double sc = 0.0;
#pragma nounroll
      for (int i = 0; i < NN; ++i) {
        const double zp = rr[(R::Zp + i) * rs], zm = rr[(R::Zm + i) * rs];
        sc = fma(Qc.w[i], fma(cue[i], zp + zm, cuo[i] * (zp - zm)), sc);
      }
      ab = fma(fac * x0, exp(-A.tauc[(size_t)lc * A.ns + sl] * rmu0), sc);
    }
    if (therm) {
      double we = 0.0, wo = 0.0;
#pragma nounroll
      for (int i = 0; i < NN; ++i) {
        we = fma(Qc.w[i], cue[i], we);
        wo = fma(Qc.w[i] * cuo[i], rr[(R::H + i) * rs], wo);
      }
      const double ce0 = (1.0 - om) + 2.0 * we;
      a1t = slope * ce0;
      a0 = fma(bt, ce0, 2.0 * slope * wo);
    }
    // general segment [t1 (evaluation), t2 (far end)] for user depths inside the layer
    auto integ = [&](double t1, double t2) {
      double r = 0.0;
#pragma nounroll
      for (int j = 0; j < NN; ++j) {
        r += seg_exp(hpl[j], kk[j], t1, t2, 0.0, muu);
        r += seg_exp(hmi[j], -kk[j], t1, t2, taup, muu);
      }
      if (beam) r += seg_exp(ab, rmu0, t1, t2, 0.0, muu);
      if (therm) {
        const double e2 = exp(-(t2 - t1) / muu);
        r += (a0 + a1t * t1 + a1t * muu) - (a0 + a1t * t2 + a1t * muu) * e2;
      }
      return r;
    };
    // whole layer, entry -> exit, from the stored exp(-k tau'), exp(-tau'/mu0)
    // and one exp(-tau'/|mu|): the +k terms decay along upward rays, the -k
    // terms along downward ones; the other family meets 1 - k|mu| -> 0 and goes
    // through dexp's (1 - e^-y)/y series
    const double anu = fabs(muu);
    const double lmu = taup / anu;
    const double emu = exp(-lmu);
    double lay = 0.0;
#pragma nounroll
    for (int j = 0; j < NN; ++j) {
      const double ek = rr[(R::Ek + j) * rs];
      const double reg = (1.0 - ek * emu) / fma(kk[j], anu, 1.0);
      const double sng = dexp(ek, emu, fma(-kk[j], anu, 1.0), lmu);
      lay = up ? fma(hpl[j], reg, fma(hmi[j], sng, lay)) : fma(hpl[j], sng, fma(hmi[j], reg, lay));
    }
    if (beam) {
      const double e0l = rr[R::E0 * rs];
      lay += up ? ab * (1.0 - e0l * emu) / fma(anu, rmu0, 1.0)
                : ab * dexp(e0l, emu, fma(-anu, rmu0, 1.0), lmu);
    }
    if (therm) {  // (a0 + a1 t1 + a1 mu) - (a0 + a1 t2 + a1 mu) e^{-(t2-t1)/mu}
      lay += up ? (a0 + a1t * muu) - (a0 + a1t * taup + a1t * muu) * emu
                : (a0 + a1t * taup + a1t * muu) - (a0 + a1t * muu) * emu;
    }
    const double cin = cur;                // at the entry boundary
    const double cout = fma(cin, emu, lay);  // at the exit boundary
    const double tau = tbot - ttop;
    const double scale = tau > 0.0 ? taup / tau : 0.0;
    // value at local depth t: boundaries from cin/cout, interior by integ
    auto at = [&](double t) {
      const double tin = up ? taup : 0.0;  // entry depth
      if (t == tin) return cin;
      if (t == taup - tin) return cout;
      return cin * exp(-fabs(tin - t) / anu) + integ(t, tin);
    };
    if (up) {
      while (k >= 0 && user_tau(A, k, sl) >= ttop) {
        const double t = fmin(fmax((user_tau(A, k, sl) - ttop) * scale, 0.0), taup);
        const double val = at(t);
        A.radm[((size_t)k * A.numu + iu) * nu + u] = val;
        chk += val;
        --k;
      }
    } else {
      while (k < A.ntau && user_tau(A, k, sl) <= tbot) {
        const double t = fmin(fmax((user_tau(A, k, sl) - ttop) * scale, 0.0), taup);
        const double val = at(t);
        A.radm[((size_t)k * A.numu + iu) * nu + u] = val;
        chk += val;
        ++k;
      }
    }
    cur = cout;
  }
  // user depths beyond the bottom (flagged by the taus kernel): bottom value
  for (; k < A.ntau && !up; ++k) A.radm[((size_t)k * A.numu + iu) * nu + u] = cur;
  if (!isfinite(chk)) flag(A, s, kStNonFinite);
}

// ============================================================================
// host side
// ============================================================================
// called once per device from hd::upload_rad_tables, under its lock
hipError_t upload_rad_tables(const QuadHost* per_nn) {
  static RadTabs<kMaxRegNN + 1, kRadMaxNN> c;  // ~560 KB: keep off the stack
  static RadCoef coef;
  fill_rad(c, per_nn);
  fill_rad_coef(coef);
  hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(c_rad), &c, sizeof(c));
  if (e != hipSuccess) return e;
  return hipMemcpyToSymbol(HIP_SYMBOL(c_rcoef), &coef, sizeof(RadCoef));
}

hipError_t launch_rad_const(int nn, const RadArgs& a, hipStream_t stream) {
  return dispatch_nn<kMaxRegNN + 1, kRadMaxNN>(nn, [&](auto NN) {
    const long nc = (long)a.ns * a.nlyr;
    hipLaunchKernelGGL(hd_rad_const_kernel<NN>, dim3((unsigned)((nc + 255) / 256), (unsigned)a.nm),
                       dim3(256), 0, stream, a);
    return hipGetLastError();
  });
}

hipError_t launch_rad_flux(int nn, const RadArgs& a, hipStream_t stream) {
  return dispatch_nn<kMaxRegNN + 1, kRadMaxNN>(nn, [&](auto NN) {
    const long nf = (long)a.ns * a.ntau;
    hipLaunchKernelGGL(hd_rad_flux_kernel<NN>, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0,
                       stream, a);
    return hipGetLastError();
  });
}

hipError_t launch_rad_user(int nn, const RadArgs& a, hipStream_t stream) {
  return dispatch_nn<kMaxRegNN + 1, kRadMaxNN>(nn, [&](auto NN) {
    const long nr = (long)a.ns * a.numu;
    hipLaunchKernelGGL(hd_rad_user_kernel<NN>, dim3((unsigned)((nr + 63) / 64), (unsigned)a.nm),
                       dim3(64), 0, stream, a);
    return hipGetLastError();
  });
}

}  // namespace wide
}  // namespace hd
