// hd_kernels.hip -- gfx950 kernels of the flux-only discrete-ordinate solve.
//
//   hd_planck_kernel     one lane per (solve, level): Planck radiance of every
//                        level + surface + top emission   [cdisort c_planck_func1]
//   hd_layer_kernel<NN>  one lane per (solve, layer): delta-M, phase-matrix
//                        assembly, symmetric eigenproblem (Cholesky + Jacobi),
//                        beam/thermal particular solutions, and the layer's
//                        reflection/transmission operators + sources in the
//                        flux-weighted basis.   [c_setdis, c_soleig, c_upbeam,
//                        c_upisot]
//   hd_sweep_kernel<NN>  one lane per solve: adding sweep top->bottom,
//                        Lambertian surface, back-substitution bottom->top,
//                        level fluxes in harp layout.  [c_setmtx, c_solve0,
//                        c_fluxes; pydisort gather + level reversal]
//
// Scratch layout per chunk (solve-interleaved: lane = solve, so every global
// access of a wave is 64 consecutive doubles):
//   planck      [L+3][nsc]       B(level 0..L, harp order), B(btemp), temis*B(ttemp)
//   layer ops   [lc][pair][nsc] double2: RecL (R~ upper, T~ upper, S~+, S~-,
//                                tau'; 45 pairs at NN = 8)
//   back-sub    [lc][pair][nsc] double2: RecB (ZT column-major, t, rc, cs; 41
//                                pairs at NN = 8)
//   (16 bytes per lane and record access: half the memory instructions, so half
//   the vmcnt-ordered round trips of the one-wave-per-SIMD sweep)
#include <cmath>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "hd_kernels.hpp"

namespace hd {

// quadrature tables for every NN, in the constant address space
struct QuadTables {
  Quad<1> q1;
  Quad<2> q2;
  Quad<3> q3;
  Quad<4> q4;
  Quad<5> q5;
  Quad<6> q6;
  Quad<7> q7;
  Quad<8> q8;
};
__constant__ QuadTables c_quad;
// hd_solve_flx: h = g / mu of every NN (row NN-1), the mean-intensity functional
// sum_i w_i I_i = sum_i h_i psi_i -- a table of its own, so that Quad keeps its layout
__constant__ double c_quad_h[kMaxRegNN][kMaxRegNN];
// The layer kernel's Legendre tables with the basis scale folded in, likewise tables of
// their own (the team and radiance kernels share Quad): spt[l][i] = sd_i P_l(mu_i), so
// that -A+ and -A- accumulate as diag - sum_l g_l spt[l][i] spt[l][j] with no scaling pass
// after the loop, and rmusd_i = 1 / (mu_i sd_i) for the beam source that arrives scaled
template <int NN>
struct QuadS {
  double spt[2 * NN][NN];
  double rmusd[NN];
};
struct QuadSTables {
  QuadS<1> q1;
  QuadS<2> q2;
  QuadS<3> q3;
  QuadS<4> q4;
  QuadS<5> q5;
  QuadS<6> q6;
  QuadS<7> q7;
  QuadS<8> q8;
};
__constant__ QuadSTables c_quad_s;
template <int NN>
__device__ __forceinline__ const QuadS<NN>& quad_s() {
  if constexpr (NN == 1) return c_quad_s.q1;
  else if constexpr (NN == 2) return c_quad_s.q2;
  else if constexpr (NN == 3) return c_quad_s.q3;
  else if constexpr (NN == 4) return c_quad_s.q4;
  else if constexpr (NN == 5) return c_quad_s.q5;
  else if constexpr (NN == 6) return c_quad_s.q6;
  else if constexpr (NN == 7) return c_quad_s.q7;
  else return c_quad_s.q8;
}
// 1/n for the beam's Legendre recursion (uniform index: scalar loads)
__constant__ double c_inv_int[2 * kMaxRegNN + 2] = {
    0.0,        1.0,        1.0 / 2,  1.0 / 3,  1.0 / 4,  1.0 / 5,  1.0 / 6,
    1.0 / 7,    1.0 / 8,    1.0 / 9,  1.0 / 10, 1.0 / 11, 1.0 / 12, 1.0 / 13,
    1.0 / 14,   1.0 / 15,   1.0 / 16, 1.0 / 17};

template <int NN>
__device__ __forceinline__ const Quad<NN>& quad() {
  if constexpr (NN == 1) return c_quad.q1;
  else if constexpr (NN == 2) return c_quad.q2;
  else if constexpr (NN == 3) return c_quad.q3;
  else if constexpr (NN == 4) return c_quad.q4;
  else if constexpr (NN == 5) return c_quad.q5;
  else if constexpr (NN == 6) return c_quad.q6;
  else if constexpr (NN == 7) return c_quad.q7;
  else return c_quad.q8;
}

// one wave per block: a layer-kernel wave can take any SIMD the previous chunk's
// sweep leaves free (hd_solve runs the two on separate streams)
constexpr int kLayerBlock = 64;
// The layer kernel warms L2 with the prop record of the block dispatched this many blocks
// later (same XCD; 0: off).  Swept on the GPU, profiles/r06/layer_prefetch_ab.txt: layer
// kernel alone 1.70 -> 1.60-1.65 ms; C4 +0.7 %, the 8-GPU rank shape +4 % at 384.
#ifndef HD_LAYER_PREFETCH
#define HD_LAYER_PREFETCH 384
#endif
constexpr int kLayersPerBlock = kLayerBlock / 64;

// phase boundary: keeps the scheduler from hoisting the next phase's loads
// (and their registers) above the current phase
#define HD_PHASE() __builtin_amdgcn_sched_barrier(0)

// ============================================================================
// K0: Planck radiance per (solve, level)
// ============================================================================
__global__ __launch_bounds__(256) void hd_planck_kernel(PlanckArgs A) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int nl = A.nlyr + 3;
  if (tid >= (long)A.nsc * nl) return;
  const int lev = (int)(tid / A.nsc);
  const int sl = (int)(tid - (long)lev * A.nsc);
  const long s = solve_of(A.s0 + sl, A.cmaj, A.nwave, A.ncol);
  const int w = (int)(s / A.ncol);
  const int c = (int)(s - (long)w * A.ncol);
  double b;
  if (lev <= A.nlyr) {
    b = plkavg(A.wlo[w], A.whi[w], A.temf[(size_t)c * (A.nlyr + 1) + lev]);
  } else if (lev == A.nlyr + 1) {
    b = plkavg(A.wlo[w], A.whi[w], A.btemp ? A.btemp[s] : 0.0);
  } else {
    const double te = A.temis ? A.temis[s] : 0.0;
    b = te != 0.0 ? te * plkavg(A.wlo[w], A.whi[w], A.ttemp ? A.ttemp[s] : 0.0) : 0.0;
  }
  A.out[(size_t)lev * A.nsc + sl] = b;
}

// ============================================================================
// K0b: cumulative delta-M-scaled optical depth above every layer (beam only)
// ============================================================================
__global__ __launch_bounds__(256) void hd_tauc_kernel(TaucArgs A) {
  const long sl = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (sl >= A.nsc) return;
  const long s = solve_of(A.s0 + sl, A.cmaj, A.nwave, A.ncol);
  const int L = A.nlyr, np = A.nprop;
  const double* p = A.prop + (size_t)s * L * np;
  double tauc = 0.0;
  for (int lc = 0; lc < L; ++lc) {  // solver order: top (harp layer L-1) first
    const double* q = p + (size_t)(L - 1 - lc) * np;
    double a = np > 1 ? q[1] : 0.0;
    if (a == 1.0) a = 1.0 - kDither;
    const double f = A.use_f ? q[A.f_slot] : 0.0;
    A.out[(size_t)lc * A.nsc + sl] = tauc;
    tauc += (1.0 - a * f) * q[0];
  }
}

// ============================================================================
// K0c (hd_solve_flx): the terms of the flux record that need the input optics, per
// solver level lc (0 = top): rfldir = mu0 F0 exp(-tau/mu0) on the UNSCALED depth,
// uavgso = F0 exp(-tau'/mu0) / (4 pi) on the delta-M scaled one (hd_tauc_kernel's
// sum), and (1 - ssa_in) 4 pi of the layer above the level (the top level: the top
// layer; the input albedo, no dither, no scaling -- cdisort's layru at a boundary)
// ============================================================================
// SPHER (hd_solve_flx_spher): the two beam terms on hd_spher_kernel's slant depths,
// rfldir = mu0 F0 exp(-ch), uavgso = F0 exp(-ch') / (4 pi)
template <bool SPHER>
__device__ __forceinline__ void flx_level_body(const FlxLevelArgs& A, const SphArgs* P) {
  const long sl = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (sl >= A.nsc) return;
  const long s = A.s0 + sl;
  const int L = A.nlyr, np = A.nprop;
  const size_t nsc = A.nsc;
  const double* p = A.prop + (size_t)s * L * np;
  const double mu0 = A.umu0 ? A.umu0[s] : 1.0;
  const double fb = A.fbeam ? A.fbeam[s] : 0.0;
  bool beam = fb > 0.0 && mu0 > 0.0;
  if constexpr (SPHER) beam = beam && P->chp[(size_t)(L + 1) * nsc + sl] != 0.0;
  const double rmu0 = beam ? 1.0 / mu0 : 0.0;
  const double f0mu0 = beam ? fb * mu0 : 0.0;
  const double f04pi = beam ? fb / (4.0 * kPi) : 0.0;
  double* o_dir = A.out;
  double* o_so = A.out + (size_t)(L + 1) * nsc;
  double* o_abs = A.out + 2 * (size_t)(L + 1) * nsc;
  double tau = 0.0, tauc = 0.0, absl = 0.0;
  for (int lc = 0; lc <= L; ++lc) {  // solver order: top (harp layer L-1) first
    if constexpr (SPHER) {
      o_dir[(size_t)lc * nsc + sl] = f0mu0 * exp(-P->ch[(size_t)lc * nsc + sl]);
      o_so[(size_t)lc * nsc + sl] = f04pi * exp(-P->chp[(size_t)lc * nsc + sl]);
      if (lc < L) {
        const double a_in = np > 1 ? p[(size_t)(L - 1 - lc) * np + 1] : 0.0;
        if (lc == 0) absl = (1.0 - a_in) * (4.0 * kPi);
        o_abs[(size_t)lc * nsc + sl] = absl;
        absl = (1.0 - a_in) * (4.0 * kPi);
      } else {
        o_abs[(size_t)lc * nsc + sl] = absl;
      }
    } else if (lc < L) {
      const double* q = p + (size_t)(L - 1 - lc) * np;
      const double a_in = np > 1 ? q[1] : 0.0;
      if (lc == 0) absl = (1.0 - a_in) * (4.0 * kPi);
      o_dir[(size_t)lc * nsc + sl] = f0mu0 * exp(-tau * rmu0);
      o_so[(size_t)lc * nsc + sl] = f04pi * exp(-tauc * rmu0);
      o_abs[(size_t)lc * nsc + sl] = absl;
      absl = (1.0 - a_in) * (4.0 * kPi);
      const double a = a_in == 1.0 ? 1.0 - kDither : a_in;
      const double f = A.use_f ? q[A.f_slot] : 0.0;
      tau += q[0];
      tauc += (1.0 - a * f) * q[0];
    } else {
      o_dir[(size_t)lc * nsc + sl] = f0mu0 * exp(-tau * rmu0);
      o_so[(size_t)lc * nsc + sl] = f04pi * exp(-tauc * rmu0);
      o_abs[(size_t)lc * nsc + sl] = absl;
    }
  }
}
__global__ __launch_bounds__(256) void hd_flx_level_kernel(FlxLevelArgs A) {
  flx_level_body<false>(A, nullptr);
}
__global__ __launch_bounds__(256) void hd_flx_level_spher_kernel(FlxLevelArgs A, SphArgs P) {
  flx_level_body<true>(A, &P);
}

// ============================================================================
// K0d (hd_solve_spher, hd_solve_flx_spher): pseudo-spherical beam geometry, one lane per
// solve.  The slant optical depth to harp level l through the
// spherical shells above it,
//   ch_l = sum_{j >= l} dtau_j g(l, j),  g(l, j) = (2R + z_{j+1} + z_j) / (a(l, j+1) + a(l, j)),
//   a(l, m) = sqrt((z_m - z_l)(2R + z_m + z_l) + ((R + z_l) mu0)^2)
// (the argument of the root in this form has no cancellation; g -> 1/mu0 as R -> inf and
// g = 1 at mu0 = 1), on the delta-M scaled layer depths (ch', what the solve uses) and,
// for the flux record, on the unscaled ones (ch, rfldir only); and per solver layer the
// secant lambda = (ch'_bottom - ch'_top) / dtau' of the beam's single exponential inside
// it (dtau' = 0: g(j, j)).  lambda may be zero, negative or large.  A zd that is not
// finite, not strictly increasing or reaches the planet's centre sets kStBadInput on the
// solve and turns its beam off (row nlyr+1 of chp).
// ============================================================================
__global__ __launch_bounds__(256) void hd_spher_kernel(SpherProArgs A) {
  const long sl = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (sl >= A.nsc) return;
  const long s = solve_of(A.s0 + sl, A.cmaj, A.nwave, A.ncol);
  const int L = A.nlyr, np = A.nprop;
  const size_t nsc = A.nsc;
  const long col = s % A.ncol;
  const double* z = A.zd + (A.per_column ? (size_t)col * (L + 1) : 0);
  const double R = A.radius;
  bool ok = R + z[0] > 0.0;
  for (int m = 0; m <= L; ++m) {
    const double zm = z[m];
    if (!isfinite(zm) || (m > 0 && !(zm > z[m - 1]))) ok = false;
  }
  if (!ok) {
    atomicOr(&A.status[s], kStBadInput);
    atomicOr(A.anyerr, 1);
  }
  const double mu0 = A.umu0 ? A.umu0[s] : 1.0;
  const double fb = A.fbeam ? A.fbeam[s] : 0.0;
  const bool beam = ok && fb > 0.0 && mu0 > 0.0;
  A.chp[(size_t)(L + 1) * nsc + sl] = beam ? 1.0 : 0.0;
  A.chp[sl] = 0.0;
  if (A.ch) A.ch[sl] = 0.0;
  if (!beam) {
    for (int lc = 0; lc < L; ++lc) {
      A.chp[(size_t)(lc + 1) * nsc + sl] = 0.0;
      A.lam[(size_t)lc * nsc + sl] = 0.0;
      if (A.ch) A.ch[(size_t)(lc + 1) * nsc + sl] = 0.0;
    }
    return;
  }
  // the layer depths by solver layer (top first), staged solve-interleaved: the double
  // loop below reads them coalesced
  double* dtp = A.dts;
  double* dtu = A.dts + (size_t)L * nsc;
  {
    const double* p = A.prop + (size_t)s * L * np;
    for (int lc = 0; lc < L; ++lc) {
      const double* q = p + (size_t)(L - 1 - lc) * np;
      double a = np > 1 ? q[1] : 0.0;
      if (a == 1.0) a = 1.0 - kDither;
      const double f = A.use_f ? q[A.f_slot] : 0.0;
      dtp[(size_t)lc * nsc + sl] = (1.0 - a * f) * q[0];
      dtu[(size_t)lc * nsc + sl] = q[0];
    }
  }
  double chp_top = 0.0;
  for (int lv = 1; lv <= L; ++lv) {  // solver level lv = harp level l = L - lv
    const int l = L - lv;
    const double zl = z[l];
    const double rm = (R + zl) * mu0;
    const double rm2 = rm * rm;
    double a0 = rm;  // a(l, l)
    double sp = 0.0, su = 0.0, g0 = 0.0;
    double zj = zl;
    for (int j = l; j < L; ++j) {  // harp layer j = solver layer L-1-j
      const double zj1 = z[j + 1];
      const double a1 = sqrt(fma(zj1 - zl, 2.0 * R + zj1 + zl, rm2));
      const double g = (2.0 * R + zj1 + zj) / (a1 + a0);
      if (j == l) g0 = g;
      sp = fma(dtp[(size_t)(L - 1 - j) * nsc + sl], g, sp);
      if (A.ch) su = fma(dtu[(size_t)(L - 1 - j) * nsc + sl], g, su);
      a0 = a1;
      zj = zj1;
    }
    A.chp[(size_t)lv * nsc + sl] = sp;
    if (A.ch) A.ch[(size_t)lv * nsc + sl] = su;
    const double dt = dtp[(size_t)(lv - 1) * nsc + sl];
    A.lam[(size_t)(lv - 1) * nsc + sl] = dt > 0.0 ? (sp - chp_top) / dt : g0;
    chp_top = sp;
  }
}

// ============================================================================
// K1: per-(solve, layer) setup
// ============================================================================
// Psi^T staging per lane; also holds L while the Jacobi runs (NN = 2: 5 > 4 doubles)
template <int NN>
__host__ __device__ constexpr int psi_doubles() {
  return NN > 1 ? (NN == 2 ? 5 : NN * NN) : 1;
}

// The layer setup of (solve s, solver layer lc) into its RecL record through `out`.
// psi_lds: this wave's Psi^T staging, element e of lane lt at e * kLayerBlock + lt.
// Returns the status bits.
// SPHER (pseudo-spherical beam): the beam's secant in this layer
// is hd_spher_kernel's lambda (any sign, or zero) in place of 1/mu0, its amplitude at the
// layer top exp(-ch'_top) and its transmission exp(-(ch'_bottom - ch'_top)); the phase
// function keeps the true mu0.  On a resonance lambda^2 = k_j^2 the layer is solved for
// the moved secant of hd_device.hpp's kResMove, which keeps lambda's sign
template <int NN, bool NT, bool SPHER = false>
__device__ __forceinline__ int layer_body(const LayerArgs& A, long s, int sl, int lc,
                                          double* psi_lds, int lt, PairOutT<NT>& out,
                                          const double* pf = nullptr, float* pf_sink = nullptr,
                                          const SphArgs* P = nullptr) {
  constexpr int N = 2 * NN;
  constexpr int kPsi = psi_doubles<NN>();
  const Quad<NN>& Qc = quad<NN>();
  const int L = A.nlyr;
  const int nm = A.nmom;
  const int np = A.nprop;
  int st = 0;

  // ---- inputs of this layer (harp layer L-1-lc) + delta-M (c_setdis) ----
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
  if constexpr (SPHER) {
    beam = beam && P->chp[(size_t)(L + 1) * A.nsc + sl] != 0.0;
    rmu0 = beam ? P->lam[(size_t)lc * A.nsc + sl] : 0.0;
  }
  const double mub = beam ? mu0 : 0.0;

  // ---- phase matrix even/odd parts (-A+ in ap, -A- in lch, upper) and the
  //      beam source vectors; one even/odd Legendre pair per iteration so the
  //      constant tables stream through a few scalar registers ----
  //      The tables carry the basis scale (spt[l][i] = sd_i P_l(mu_i)) and the
  //      coefficients their sign, so the accumulators start at diag(1/mu) and end as
  //      -A+ and -A-; xs and xd end as -sd_i times the beam sums
  const QuadS<NN>& Qs = quad_s<NN>();
  double lch[NN][NN], ap[NN][NN], xs[NN], xd[NN];
#pragma unroll
  for (int i = 0; i < NN; ++i) {
    xs[i] = xd[i] = 0.0;
#pragma unroll
    for (int j = i; j < NN; ++j) lch[i][j] = ap[i][j] = (i == j) ? Qc.rmu[i] : 0.0;
  }
  {
    double pprev = 0.0, pcur = 1.0;  // P_{l-1}(mu0), P_l(mu0) for the beam
#pragma nounroll
    for (int l2 = 0; l2 < NN; ++l2) {
      const int le = 2 * l2, lo = le + 1;
      const double che = le == 0 ? 1.0 : (le <= nm ? q[1 + le] : 0.0);
      const double cho = lo <= nm ? q[1 + lo] : 0.0;
      const double ge = -(2 * le + 1) * (che - f) * rf;
      const double go = -(2 * lo + 1) * (cho - f) * rf;
      const double pe0 = pcur;  // P_le(mu0)
      const double po0 = ((2 * lo - 1) * mub * pcur - (lo - 1) * pprev) * c_inv_int[lo];
      pprev = po0;
      pcur = ((2 * lo + 1) * mub * po0 - lo * pe0) * c_inv_int[lo + 1];
      double ue[NN], uo[NN];
#pragma unroll
      for (int i = 0; i < NN; ++i) {
        ue[i] = ge * Qs.spt[le][i];
        uo[i] = go * Qs.spt[lo][i];
        xs[i] = fma(ue[i], pe0, xs[i]);
        xd[i] = fma(uo[i], po0, xd[i]);
      }
#pragma unroll
      for (int i = 0; i < NN; ++i)
#pragma unroll
        for (int j = i; j < NN; ++j) {
          ap[i][j] = fma(ue[i], Qs.spt[le][j], ap[i][j]);
          lch[i][j] = fma(uo[i], Qs.spt[lo][j], lch[i][j]);
        }
    }
  }
  // L L^T = -A-  (lower triangle of lch)
  double rdl[NN];
  if (!chol_inplace<NN>(lch, rdl)) st |= kStEigen;

  // ---- pre-Jacobi vectors (depend on L only) ----
  // beam: y2 = L^-1 W D^-1/2 rv, rv = -(M D^1/2)^-1 L L^T D^1/2 xs + M^-1 xd/mu0,
  //       lxd = L^-T L^-1 D^1/2 xd  (linv(xd) = (sd/w) lxd)
  double y2[NN], lxd[NN];
  const double fb2 = fb * (0.5 / kPi);
  if (beam) {
    double y[NN], z[NN];
#pragma unroll
    for (int i = 0; i < NN; ++i) y[i] = -fb2 * xs[i];  // D^1/2 (fb2 xs): xs holds -sd xs
#pragma unroll
    for (int i = 0; i < NN; ++i) {  // z = L^T y
      double t = 0.0;
#pragma unroll
      for (int k = i; k < NN; ++k) t = fma(lch[k][i], y[k], t);
      z[i] = t;
    }
#pragma unroll
    for (int i = 0; i < NN; ++i) {  // y = L z
      double t = 0.0;
#pragma unroll
      for (int k = 0; k <= i; ++k) t = fma(lch[i][k], z[k], t);
      y[i] = t;
    }
#pragma unroll
    for (int i = 0; i < NN; ++i) {
      // rv = (-y/sd + xd/mu0)/mu, with 1/(sd mu) = 1/g; W D^-1/2 = diag(w/sd) = diag(g).
      // xd holds -sd xd, so D^1/2 (-fb2 xd) = fb2 xd[i], and rv takes it over mu sd
      const double sxd = fb2 * xd[i];
      const double rv = fma(-y[i], Qc.rg[i], sxd * rmu0 * Qs.rmusd[i]);
      y2[i] = Qc.g[i] * rv;
      lxd[i] = sxd;
    }
    lower_solve<NN>(lch, rdl, y2);    // V^T y2 below (V = B K^-1 after the Jacobi)
    lower_solve<NN>(lch, rdl, lxd);   // lxd = L^-T L^-1 D^1/2 xd
    lower_t_solve<NN>(lch, rdl, lxd);
  } else {
#pragma unroll
    for (int i = 0; i < NN; ++i) y2[i] = lxd[i] = 0.0;
  }
  // thermal: cvec = dB + 2 (dB/tau') h,  h = W^-1 D^1/2 L^-T L^-1 D^1/2 mu
  double cvec[NN];
  double db = 0.0, bsum = 0.0;
  if (A.planck) {
    const double bt = A.planckv[(size_t)(L - lc) * A.nsc + sl];
    // a transparent layer carries its top level's Planck value through
    // (c_disort's xr1 = 0 when dtaucpr = 0: B(tau) = xr0 = B_top)
    const double bb = taup > 0.0 ? A.planckv[(size_t)(L - lc - 1) * A.nsc + sl] : bt;
    db = bb - bt;
    bsum = bt + bb;
    const double b1 = taup > 0.0 ? 2.0 * db / taup : 0.0;
#pragma unroll
    for (int i = 0; i < NN; ++i) cvec[i] = Qc.sd[i] * Qc.mu[i];
    lower_solve<NN>(lch, rdl, cvec);
    lower_t_solve<NN>(lch, rdl, cvec);
#pragma unroll
    for (int i = 0; i < NN; ++i) cvec[i] = fma(b1 * Qc.rg[i], cvec[i], db);
  } else {
#pragma unroll
    for (int i = 0; i < NN; ++i) cvec[i] = 0.0;
  }

  // ---- eigenpairs (c_soleig): Sym = L^T (-A+) L = V diag(k^2) V^T ----
  // With C C^T = -A+ (SPD exactly when Sym is), X = L^T C has X X^T = Sym: the
  // one-sided Jacobi on X's columns gives B = X W with orthogonal columns, and
  // Sym B = X (X^T X) W = B diag(k^2), so k_j = |b_j| and V = B K^-1 directly --
  // no triangular solve for the eigenvectors, and C is dead before the Jacobi.
  // X^T X = C^T (-A-) C is closer to diagonal than B0^T B0 for B0 = X^T (the
  // round-1..5 form): 4.0 instead of 4.8 sweeps per 64-lane wave at C4
  // (per lane 3.76 vs 3.86; numpy model of this loop).
  double rdc[NN];
  if (!chol_inplace<NN>(ap, rdc)) st |= kStEigen;  // lower ap <- C
  double v[NN][NN];  // X, then B = X W, then Omega = L B K^-1 Delta^1/2
#pragma unroll
  for (int i = 0; i < NN; ++i)
#pragma unroll
    for (int j = 0; j < NN; ++j) {  // X_ij = sum_{k >= max(i,j)} L_ki C_kj
      double t = 0.0;
#pragma unroll
      for (int k = (i > j ? i : j); k < NN; ++k) t = fma(lch[k][i], ap[k][j], t);
      v[i][j] = t;
    }
  // L is not needed again until the beam solution: park it in this lane's (not
  // yet used) Psi staging area of LDS while B and the rotation temporaries hold
  // the registers.
  constexpr int kPark = NN * (NN + 1) / 2 + NN;
  static_assert(kPark <= kPsi || NN == 1, "L does not fit the Psi staging area");
  if constexpr (NN > 1) {
    int e = 0;
#pragma unroll
    for (int i = 0; i < NN; ++i) {
#pragma unroll
      for (int k = 0; k <= i; ++k) psi_lds[(e++) * kLayerBlock + lt] = lch[i][k];
      psi_lds[(e++) * kLayerBlock + lt] = rdl[i];
    }
  }
  asm volatile("" ::: "memory");
#if HD_LAYER_PREFETCH
  // warm L2 with the record of the block dispatched HD_LAYER_PREFETCH blocks later (same
  // XCD): three LDS-DMA dword loads touch the lines of its (2 + nmom)-double record (144
  // bytes at C4; longer records are touched at their first 144 bytes); the data lands in
  // a sink nobody reads.  Issued here, after this layer's own loads are consumed
  // and L is parked, so the Jacobi's ~36 k cycles of pure VALU cover the round trip.
  if (pf) {
    using gp = const __attribute__((address_space(1))) void*;
    using lp = __attribute__((address_space(3))) void*;
    const int o1 = np > 16 ? 16 : np - 1, o2 = np > 17 ? 17 : np - 1;  // inside the record
    __builtin_amdgcn_global_load_lds((gp)(pf), (lp)(pf_sink), 4, 0, 0);
    __builtin_amdgcn_global_load_lds((gp)(pf + o1), (lp)(pf_sink), 4, 0, 0);
    __builtin_amdgcn_global_load_lds((gp)(pf + o2), (lp)(pf_sink), 4, 0, 0);
  }
#endif
  HD_PHASE();
  if (!jacobi_os<NN>(v, A.max_sweeps)) st |= kStEigen;
  // k_j^2 = |b_j|^2, formed once: the resonance test reads it, and only a wave that
  // polished (rare) forms it again from the polished columns
  double k2[NN];
  column_norms2<NN>(v, k2);
  if (jacobi_os_polish<NN>(v, beam && near_resonance<NN>(k2, rmu0 * rmu0, kResPolish)))
    column_norms2<NN>(v, k2);
  HD_PHASE();
  double kk[NN], rk[NN];  // k_j = |b_j|, 1/k_j
#pragma unroll
  for (int j = 0; j < NN; ++j) {
    if (!(k2[j] > 0.0)) st |= kStEigen;
    const double r = k2[j] > 0.0 ? rsq_nr(k2[j]) : 0.0;
    kk[j] = k2[j] * r;
    rk[j] = r;
  }
  // beam, the part that needs only B and k (before L is back: y2 dies first)
  double ybt[NN];  // B K^-1 tt, tt = V^T y2 / (1/mu0^2 - k^2), V = B K^-1
  double rmu0e = rmu0;  // 1/mu0', the secant the layer is solved for (kResMove)
  bool moved = false;   // rmu0e is the moved secant, not the beam's own
  if (beam) {
    double tt[NN];
    const double r2 = rmu0 * rmu0;
    bool near = false;  // a mode within kResMove of the resonance (hd_device.hpp)
#pragma unroll
    for (int j = 0; j < NN; ++j) {
      double t = 0.0;
#pragma unroll
      for (int i = 0; i < NN; ++i) t = fma(v[i][j], y2[i], t);
      const double den = fma(-kk[j], kk[j], r2);
      near = near || fabs(den) < kResMove * r2;
      tt[j] = t * (rk[j] * rk[j]) * rcp_nr(den);  // K^-1 (V^T y2 / den)
    }
    if (near) {
      // the mode nearest the resonance sets the secant 1/mu0'^2, and tt is formed again
      // with it (a second eigenvalue within kResMove of that mode would keep a small
      // denominator: eigenvalues of a layer that close are not known to occur, and
      // kStNonFinite would report it)
      st |= kStResonance;
      moved = true;
      double dmin = 2.0 * r2, r2e = r2;
#pragma unroll
      for (int j = 0; j < NN; ++j) {
        const double den = fma(-kk[j], kk[j], r2);
        if (fabs(den) < dmin) {
          dmin = fabs(den);
          r2e = kk[j] * kk[j] * (den < 0.0 ? 1.0 - kResMove : 1.0 + kResMove);
        }
      }
      rmu0e = sqrt(r2e);
      // SPHER: the layer's secant lambda may be negative (under a thicker layer), and the
      // resonance is at lambda = -k_j too; the move stays on lambda's side of zero
      if constexpr (SPHER) rmu0e = copysign(rmu0e, rmu0);
#pragma unroll
      for (int j = 0; j < NN; ++j) {
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < NN; ++i) t = fma(v[i][j], y2[i], t);
        tt[j] = t * (rk[j] * rk[j]) * rcp_nr(fma(-kk[j], kk[j], r2e));
      }
    }
#pragma unroll
    for (int i = 0; i < NN; ++i) {
      double t = 0.0;
#pragma unroll
      for (int j = 0; j < NN; ++j) t = fma(v[i][j], tt[j], t);
      ybt[i] = t;
    }
  }
  HD_PHASE();
  if constexpr (NN > 1) {  // L back from LDS
    // the empty asm with a memory clobber makes this a real reload (not the
    // parked registers kept live across the Jacobi) and keeps it in place
    asm volatile("" ::: "memory");
    int e = 0;
#pragma unroll
    for (int i = 0; i < NN; ++i) {
#pragma unroll
      for (int k = 0; k <= i; ++k) lch[i][k] = psi_lds[(e++) * kLayerBlock + lt];
      rdl[i] = psi_lds[(e++) * kLayerBlock + lt];
    }
  }
  HD_PHASE();

  // ---- beam particular solution Z+/- (c_upbeam), unit attenuation above ----
  double zp[NN], zm[NN];
  double e0 = 0.0;
  if (beam) {
    double sv[NN], y[NN];
#pragma unroll
    for (int i = NN - 1; i >= 0; --i) {  // s = W^-1 D^1/2 L V tt = W^-1 D^1/2 L (B K^-1 tt)
      double t = 0.0;
#pragma unroll
      for (int k = 0; k <= i; ++k) t = fma(lch[i][k], ybt[k], t);
      sv[i] = Qc.rg[i] * t;
    }
    // dd = (lxd - D^1/2 L^-T L^-1 D^1/2 (mu s) / mu0) / w
#pragma unroll
    for (int i = 0; i < NN; ++i) y[i] = Qc.sd[i] * Qc.mu[i] * sv[i];
    lower_solve<NN>(lch, rdl, y);
    lower_t_solve<NN>(lch, rdl, y);
    // scaled depth of the layer top; without the prologue's depths the beam is
    // taken as unit at the top and the sweep applies exp(-tau_c/mu0)
    double att;
    if constexpr (SPHER) {
      const double ct = P->chp[(size_t)lc * A.nsc + sl];
      const double cb = P->chp[(size_t)(lc + 1) * A.nsc + sl];
      // a layer solved for a moved secant transmits along that secant, as the plain
      // path's does; any other by the difference of its two slant depths
      double d = moved ? -taup * rmu0e : ct - cb;
      // under a much thicker layer the slant depth falls through this one; past kE0Cap
      // (hd_device.hpp) the transmission is held and the top's amplitude lowered to match
      double ta = ct;
      if (taup > 0.0 && d > kE0Cap) {
        d = kE0Cap;
        ta = cb + kE0Cap;
      }
      att = 0.5 * exp(-ta);
      // a layer of zero depth leaves the diffuse field alone (the beam below it still
      // changes: the sweep takes that from ch' of the next level)
      e0 = taup > 0.0 ? exp(d) : 1.0;
    } else {
      const double tauc = A.tauc ? A.tauc[(size_t)lc * A.nsc + sl] : 0.0;
      att = 0.5 * exp(-tauc * rmu0);
    }
#pragma unroll
    for (int i = 0; i < NN; ++i) {
      const double dd = Qc.rg[i] * fma(-y[i], rmu0e, lxd[i]);  // (sd/w)(lxd - y/mu0')
      zp[i] = (sv[i] + dd) * att;
      zm[i] = (sv[i] - dd) * att;
    }
    if constexpr (!SPHER) e0 = exp(-taup * rmu0e);
  } else {
#pragma unroll
    for (int i = 0; i < NN; ++i) zp[i] = zm[i] = 0.0;
  }

  HD_PHASE();
  // ---- layer operators in the flux-weighted basis ----
  // Delta = tanh(k tau'/2)/k, Gamma = k tanh(k tau'/2): Gamma^1/2 K^-1 = Delta^1/2
  double dsq[NN];
  double kt[NN], em[NN];  // k tau', 1 - exp(-k tau')
#pragma unroll
  for (int j = 0; j < NN; ++j) kt[j] = kk[j] * taup;
  hd_m_expm1_neg_n<NN>(kt, em);
  // the empty asm keeps the NN evaluations together and unconditional: without it each
  // is sunk into a branch of its own under the x > 1e-8 test below, with every constant
  // of the series formed again in vector registers
#pragma unroll
  for (int j = 0; j < NN; ++j) asm volatile("" : "+v"(em[j]));
#pragma unroll
  for (int j = 0; j < NN; ++j) {
    const double x = kt[j];
    const double m = em[j];
    const double th = m * rcp_nr(2.0 - m);  // tanh(k tau'/2)
    // 1/k_j is rk[j] already (x > 1e-8 implies k_j > 0)
    const double delta = x > 1.0e-8 ? th * rk[j] : 0.5 * taup;
    dsq[j] = delta > 0.0 ? delta * rsq_nr1(delta) : 0.0;
  }
  // Psi^T = L^-T V Gamma^1/2 = L^-T B Delta^1/2 -> LDS (one column per step)
#pragma unroll
  for (int j = 0; j < NN; ++j) {
    double x[NN];
#pragma unroll
    for (int i = 0; i < NN; ++i) x[i] = v[i][j] * dsq[j];
    lower_t_solve<NN>(lch, rdl, x);
#pragma unroll
    for (int i = 0; i < NN; ++i) psi_lds[(i * NN + j) * kLayerBlock + lt] = x[i];
  }
  HD_PHASE();
  // Omega = U Delta^1/2 = L B K^-1 Delta^1/2, in place over v (rows bottom-up)
#pragma unroll
  for (int j = 0; j < NN; ++j) {
    const double sc = rk[j] * dsq[j];
#pragma unroll
    for (int i = 0; i < NN; ++i) v[i][j] *= sc;
  }
#pragma unroll
  for (int i = NN - 1; i >= 0; --i)
#pragma unroll
    for (int j = 0; j < NN; ++j) {
      double t = 0.0;
#pragma unroll
      for (int k = 0; k <= i; ++k) t = fma(lch[i][k], v[k][j], t);
      v[i][j] = t;
    }
  HD_PHASE();

  using RL = RecL<NN>;
  constexpr int nsym = NN * (NN + 1) / 2;
  double ga[NN], gb[NN];
#pragma unroll
  for (int i = 0; i < NN; ++i) {
    ga[i] = Qc.g[i] * (cvec[i] - fma(-zp[i], e0, zm[i]));
    gb[i] = Qc.g[i] * (fma(zp[i], e0, zm[i]) + bsum);
  }
  // Thin thermal layer: x = g (2 dB/tau') h is O(dB / tau') and Q~- = I - A- is O(tau'),
  // a difference of O(1) numbers.  Q~- = A- Omega Omega^T has no such difference: with
  // w = Omega Omega^T x (O(dB)) and ga0 = g (dB - a) the rest,
  // Q~- (ga0 + x) = ga0 - A- (ga0 - w): ga carries ga0 - w, and ga0 is formed again where
  // p is (from zp, zm, e0, which live on to the sources), so nothing more than ga stays
  // live across the factorisation.
  const bool thin = A.planck && taup > 0.0 && taup < kThinTau;  // hd_device.hpp
  if (thin) {
    double y[NN];
#pragma unroll
    for (int j = 0; j < NN; ++j) {
      double t = 0.0;  // x = g (cvec - dB): the slope part alone (|x| >> dB here)
#pragma unroll
      for (int i = 0; i < NN; ++i) t = fma(v[i][j], Qc.g[i] * (cvec[i] - db), t);
      y[j] = t;
    }
#pragma unroll
    for (int i = 0; i < NN; ++i) {
      double t = 0.0;
#pragma unroll
      for (int j = 0; j < NN; ++j) t = fma(v[i][j], y[j], t);
      ga[i] = Qc.g[i] * (db - fma(-zp[i], e0, zm[i])) - t;
    }
  }
  // By Woodbury, Q~- = Omega (I + Omega^T Omega)^-1 Omega^T = I - A-  and
  // Q~+ = -Psi^T (I + Psi Psi^T)^-1 Psi = A+ - I  with the SPD inverses
  // A- = (I + Omega Omega^T)^-1, A+ = (I + Psi^T Psi)^-1 (eigenvalues in (0, 1]),
  // so R~ = A+ - A-, T~ = A- + A+ - I and the sources need A-/A+ times a vector.
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
    if (thin) {  // ga0 - A- ga: w = ga0 - ga back in
#pragma unroll
      for (int i = 0; i < NN; ++i) pvec[i] += Qc.g[i] * (db - fma(-zp[i], e0, zm[i])) - ga[i];
    }
  }
  double ap_[NN][NN], qvec[NN];
  {
    double pt_[NN][NN];  // pt_[i][j] = Psi^T[i][j]
#pragma unroll
    for (int i = 0; i < NN; ++i)
#pragma unroll
      for (int j = 0; j < NN; ++j) pt_[i][j] = psi_lds[(i * NN + j) * kLayerBlock + lt];
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

  // ---- store: R~ = A+ - A-, T~ = A- + A+ - I (upper), S~+, S~-, tau' ----
  double chk = 0.0;
  {
    int e = 0;
#pragma unroll
    for (int i = 0; i < NN; ++i)
#pragma unroll
      for (int j = i; j < NN; ++j, ++e) {
        const double r = ap_[i][j] - am_[i][j];
        out.put(RL::R + e, r);
        chk += r;
      }
    out.close(RL::R + nsym - 1);
    e = 0;
#pragma unroll
    for (int i = 0; i < NN; ++i)
#pragma unroll
      for (int j = i; j < NN; ++j, ++e) {
        const double t = (am_[i][j] + ap_[i][j]) - ((i == j) ? 1.0 : 0.0);
        out.put(RL::T + e, t);
        chk += t;
      }
    out.close(RL::T + nsym - 1);
  }
  double smv[NN];
#pragma unroll
  for (int i = 0; i < NN; ++i) {
    const double sp = Qc.g[i] * (zp[i] * (1.0 - e0) - db) + pvec[i] - qvec[i];
    smv[i] = Qc.g[i] * (-zm[i] * (1.0 - e0) + db) - pvec[i] - qvec[i];
    out.put(RL::Sp + i, sp);
    chk += sp + smv[i];
  }
  out.close(RL::Sp + NN - 1);
#pragma unroll
  for (int i = 0; i < NN; ++i) out.put(RL::Sm + i, smv[i]);
  out.close(RL::Sm + NN - 1);
  out.put(RL::Tau, taup);
  // the pad after tau' goes out as zero: no kernel reads it (its one reader, the
  // LDS-state nstr-16 sweep of DESIGN.md section 9, took the layer's direct-beam
  // transmission from it)
  out.close(RL::Tau);
  if (!isfinite(chk + taup)) st |= kStNonFinite;
  return st;
}

// The frame of the two layer kernels: block numbering, prefetch target, the record
// writer, layer_body and the status write.  SPHER (hd_solve_spher / hd_solve_flx_spher):
// the pseudo-spherical beam, P the chunk's slant depths.  Shared, hd_layer_kernel<4> and
// <5> take 66 SGPRs for 70, at the same occupancy and speed (profiles/lanewrap/README.md)
template <int NN, bool NT, bool SPHER>
__device__ __forceinline__ void layer_kernel_body(const LayerArgs& A, const SphArgs* P) {
  __shared__ double psi_lds[psi_doubles<NN>() * kLayerBlock];  // Psi^T staged per lane
  // block = 64 consecutive solves (one wave each) x kLayersPerBlock consecutive
  // layers: a wave's stores are coalesced (same layer, consecutive solves).
  // Neighbouring layers of a solve share 128-B lines of prop (18 doubles per
  // record), so the blocks of one solve tile are numbered layer-fastest and
  // dealt to the same XCD (blocks b and b + 8 share an XCD's L2): the second
  // reader of a line finds it in L2 instead of HBM
  const int lt = threadIdx.x;
  const int ntl = (A.nlyr + kLayersPerBlock - 1) / kLayersPerBlock;
  const int nb = (int)gridDim.x;
  auto tile_of = [&](int b, int& ts, int& tl) {
    const int x = b & 7, base = nb >> 3, extra = nb & 7;
    const int logical = x * base + (x < extra ? x : extra) + (b >> 3);
    ts = logical / ntl;
    tl = logical - ts * ntl;
  };
  int ts, tl;
  tile_of((int)blockIdx.x, ts, tl);
  const int sl = ts * 64 + (lt & 63);
  const int lc = tl * kLayersPerBlock + (lt >> 6);  // solver layer, 0 = top
  if (sl >= A.nsc || lc >= A.nlyr) return;
  const long s = solve_of(A.s0 + sl, A.cmaj, A.nwave, A.ncol);
  PairOutT<NT> out{reinterpret_cast<double2*>(A.scr) + (size_t)lc * RecL<NN>::pairs * A.nsc + sl,
                   (size_t)A.nsc, 0.0};
  const double* pf = nullptr;
  float* pf_sink = nullptr;
#if HD_LAYER_PREFETCH
  __shared__ float pf_lds[kLayerBlock];
  pf_sink = pf_lds;
  if ((int)blockIdx.x + HD_LAYER_PREFETCH < nb) {
    int ts2, tl2;
    tile_of((int)blockIdx.x + HD_LAYER_PREFETCH, ts2, tl2);
    int sl2 = ts2 * 64 + (lt & 63);
    const int lc2 = tl2 * kLayersPerBlock + (lt >> 6);
    if (sl2 >= A.nsc) sl2 = A.nsc - 1;
    if (lc2 < A.nlyr) {
      const long s2 = solve_of(A.s0 + sl2, A.cmaj, A.nwave, A.ncol);
      pf = A.prop + ((size_t)s2 * A.nlyr + (A.nlyr - 1 - lc2)) * A.nprop;
    }
  }
#endif
  const int st = layer_body<NN, NT, SPHER>(A, s, sl, lc, psi_lds, lt, out, pf, pf_sink, P);
  if (st) {
    atomicOr(&A.status[s], st);
    if (st & 0x0F) atomicOr(A.anyerr, 1);
  }
}
template <int NN, bool NT>
__global__ __launch_bounds__(kLayerBlock) void hd_layer_kernel(LayerArgs A) {
  layer_kernel_body<NN, NT, false>(A, nullptr);
}
template <int NN, bool NT>
__global__ __launch_bounds__(kLayerBlock) void hd_layer_spher_kernel(LayerArgs A, SphArgs P) {
  layer_kernel_body<NN, NT, true>(A, &P);
}
// ============================================================================
// K2: per-solve adding sweep + back-substitution
// ============================================================================
// hd_solve_flx: the eight components of solver level lc (harp level L - lc) of solve s
// from the level's fluxes (up, total down), its two hemispheric mean intensities and
// Planck value, and the prologue's per-level terms
__device__ __forceinline__ void flx_emit(const FlxArgs& F, long s, long sl, size_t nsc, int L,
                                         int lc, double up, double dn, double uavgup,
                                         double uavgdn, double blev) {
  const size_t nl = (size_t)(L + 1) * nsc;
  const double rfldir = F.lvl[(size_t)lc * nsc + sl];
  const double uavgso = F.lvl[nl + (size_t)lc * nsc + sl];
  const double absl = F.lvl[2 * nl + (size_t)lc * nsc + sl];
  const double uavg = uavgup + uavgdn + uavgso;
  double* o = F.flx + ((size_t)s * (L + 1) + (L - lc)) * kNFlx;
  double2* o2 = reinterpret_cast<double2*>(o);
  o2[0] = make_double2(rfldir, dn - rfldir);
  o2[1] = make_double2(up, absl * (uavg - blev));
  o2[2] = make_double2(uavg, uavgdn);
  o2[3] = make_double2(uavgup, uavgso);
}

// The adding sweep of solve s (chunk lane sl): layer lc's record through
// rec_at(lc), a callable returning a getter e -> RecL element e (loads from the
// HBM record).  Stores the back-substitution records, the surface level and
// x; returns the status bits.  sweep_kernel_body below states the accessor once
// for the three kernels; sharing it moved two VGPRs of one instantiation and no
// occupancy, scratch or speed (profiles/lanewrap/README.md).
// FLX (hd_solve_flx): the records are RecBF -- each level also gets the mean-intensity
// row rh and scalar ch -- and the surface level's eight components go to F->flx.
// SPHER (pseudo-spherical beam): the direct beam at every level is exp(-ch') of
// hd_spher_kernel's slant depth, not exp(-tau_c/mu0) of the running depth; the layer
// records carry the attenuated sources (beam_scale off)
template <int NN, bool NT, bool FLX = false, bool SPHER = false, class RecAt>
__device__ __forceinline__ int sweep_body(const SweepArgs& A, long sl, long s, RecAt&& rec_at,
                                          const FlxArgs* F = nullptr, const SphArgs* P = nullptr) {
  const Quad<NN>& Qc = quad<NN>();
  const int L = A.nlyr;
  const size_t nsc = A.nsc;
  constexpr int nsym = NN * (NN + 1) / 2;
  int st = 0;

  const double mu0 = A.umu0 ? A.umu0[s] : 1.0;
  const double fb = A.fbeam ? A.fbeam[s] : 0.0;
  bool beam = fb > 0.0 && mu0 > 0.0;
  if constexpr (SPHER) beam = beam && P->chp[(size_t)(L + 1) * nsc + sl] != 0.0;
  const double alb = A.albedo ? A.albedo[s] : 0.0;
  if (!(alb >= 0.0) || !(alb <= 1.0)) st |= kStBadInput;
  double top = A.fisot ? A.fisot[s] : 0.0;
  double bsurf = 0.0;
  if (A.planck) {
    bsurf = A.planckv[(size_t)(L + 1) * nsc + sl];
    top += A.planckv[(size_t)(L + 2) * nsc + sl];
  }
  const double twopi = 2.0 * kPi;
  const double rmu0 = beam ? 1.0 / mu0 : 0.0;
  const double f0mu0 = beam ? fb * mu0 : 0.0;
  // direct beam at solver level lc (1 without a beam)
  auto beam_at = [&](int lc, double tauc) {
    if constexpr (SPHER) return beam ? exp(-P->chp[(size_t)lc * nsc + sl]) : 1.0;
    else return exp(-tauc * rmu0);
  };

  double ra[NN][NN];  // reflection of the stack above (upper triangle)
  double sd[NN];      // diffuse downward source at the current interface
#pragma unroll
  for (int i = 0; i < NN; ++i) {
    sd[i] = Qc.g[i] * top;
#pragma unroll
    for (int j = i; j < NN; ++j) ra[i][j] = 0.0;
  }
  double tauc = 0.0;

  for (int lc = 0; lc < L; ++lc) {
    using RL = RecL<NN>;
    using RB = std::conditional_t<FLX, RecBF<NN>, RecB<NN>>;
    auto rec = rec_at(lc);
    PairOutT<NT> bp{reinterpret_cast<double2*>(A.bsub) + (size_t)lc * RB::pairs * nsc + sl, nsc, 0.0};
    // this layer's R~ (upper) and S~+ ; each record element is read once
    double rl[NN][NN], spl[NN];
    {
      int e = 0;
#pragma unroll
      for (int i = 0; i < NN; ++i)
#pragma unroll
        for (int j = i; j < NN; ++j) rl[i][j] = rec(RL::R + (e++));
#pragma unroll
      for (int i = 0; i < NN; ++i) spl[i] = rec(RL::Sp + i);
    }
    // direct beam at the layer top; the sources of a unit-beam record scale with it
    const double eb = beam_at(lc, tauc);
    const double sscale = A.beam_scale ? eb : 1.0;
#pragma unroll
    for (int i = 0; i < NN; ++i) spl[i] *= sscale;

    // level lc (top of layer lc): F_dn = rc . I+ + cs
    {
      double cs = 0.0;
#pragma unroll
      for (int i = 0; i < NN; ++i) {
        double t = 0.0;
#pragma unroll
        for (int j = 0; j < NN; ++j) t = fma(HD_SYM(ra, j, i), Qc.g[j], t);
        bp.put(RB::Rc + i, twopi * t);
        cs = fma(Qc.g[i], sd[i], cs);
      }
      bp.close(RB::Rc + NN - 1);
      bp.put(RB::Cs, fma(twopi, cs, f0mu0 * eb));
      bp.close(RB::Cs);
    }
    if constexpr (FLX) {  // the same level's sum_i w_i I-_i = rh . I+ + ch, h = g / mu
      double ch = 0.0;
#pragma unroll
      for (int i = 0; i < NN; ++i) {
        double t = 0.0;
#pragma unroll
        for (int j = 0; j < NN; ++j) t = fma(HD_SYM(ra, j, i), c_quad_h[NN - 1][j], t);
        bp.put(RB::Rh + i, t);
        ch = fma(c_quad_h[NN - 1][i], sd[i], ch);
      }
      bp.close(RB::Rh + NN - 1);
      bp.put(RB::Ch, ch);
      bp.close(RB::Ch);
    }
    HD_PHASE();
    // A = Ra (read through its upper triangle); W1 = I - R_l A ; v1 = R_l Sd + S+
    double w1[NN][NN], t1[NN];
#pragma unroll
    for (int i = 0; i < NN; ++i) {
#pragma unroll
      for (int j = 0; j < NN; ++j) {
        double t = (i == j) ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < NN; ++k) t = fma(-HD_SYM(rl, i, k), HD_SYM(ra, k, j), t);
        w1[i][j] = t;
      }
      double t = spl[i];
#pragma unroll
      for (int k = 0; k < NN; ++k) t = fma(HD_SYM(rl, i, k), sd[k], t);
      t1[i] = t;
    }
    HD_PHASE();
    // LU without pivoting (W1 = I - product of reflections; pivot watch);
    // reciprocal pivots kept on the diagonal
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
    // t = W1^-1 v1
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
    // u = A t + Sd
    double u[NN];
#pragma unroll
    for (int i = 0; i < NN; ++i) {
      double t = sd[i];
#pragma unroll
      for (int k = 0; k < NN; ++k) t = fma(HD_SYM(ra, i, k), t1[k], t);
      u[i] = t;
      bp.put(RB::Tv + i, t1[i]);
    }
    bp.close(RB::Tv + NN - 1);
    HD_PHASE();
    // M1 = A W1^-1 = A (I - R_l A)^-1 is symmetric with A and R_l ((I - A R_l) A =
    // A (I - R_l A)), so only its upper triangle is formed and kept: row r of
    // x W1 = a  ->  (x L) U = a, the backward substitution stopping at column r
    double m1[NN][NN];
#pragma unroll
    for (int r = 0; r < NN; ++r) {
      double z[NN];
#pragma unroll
      for (int j = 0; j < NN; ++j) {  // z U = a  (forward over columns)
        double t = HD_SYM(ra, r, j);
#pragma unroll
        for (int k = 0; k < j; ++k) t = fma(-z[k], w1[k][j], t);
        z[j] = t * w1[j][j];
      }
#pragma unroll
      for (int j = NN - 1; j >= r; --j) {  // x L = z  (backward, unit L)
        double t = z[j];
#pragma unroll
        for (int k = j + 1; k < NN; ++k) t = fma(-z[k], w1[k][j], t);
        z[j] = t;
        m1[r][j] = t;
      }
    }
    HD_PHASE();
    // T~ (upper), read once, with S~- and tau': the loads are issued before this
    // layer's ZT stores and Sd <- T_l u + S- is formed right away.  Loaded after the
    // stores (where Sd is first needed), each S~- element's s_waitcnt also waited for
    // all 32 ZT stores to retire -- four round trips per layer
    double tl[NN][NN];
    {
      int e = 0;
#pragma unroll
      for (int i = 0; i < NN; ++i)
#pragma unroll
        for (int j = i; j < NN; ++j) tl[i][j] = rec(RL::T + (e++));
    }
    {
      double sm_[NN];
#pragma unroll
      for (int i = 0; i < NN; ++i) sm_[i] = rec(RL::Sm + i);
      const double taul = rec(RL::Tau);
#pragma unroll
      for (int i = 0; i < NN; ++i) {
        double t = sm_[i] * sscale;
#pragma unroll
        for (int k = 0; k < NN; ++k) t = fma(HD_SYM(tl, i, k), u[k], t);
        sd[i] = t;
      }
      tauc += taul;
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
      // ZT column-major: column j is elements j NN .. j NN + NN-1
#pragma unroll
      for (int i = 0; i < NN; ++i) bp.put(RB::Z + j * NN + i, x[i]);
    }
    bp.close(RB::Z + NN * NN - 1);
    HD_PHASE();
    // P = M1 T_l and Ra <- R_l + T_l P (upper).  NN > 4: one column of both at a time --
    // column j of Ra needs column j of P only, so P is never held whole.  NN <= 4, where
    // everything fits the vector registers: P whole, then Ra (the column form cost three
    // nstr-6 spher instantiations a wave per SIMD of occupancy)
    if constexpr (NN > 4) {
#pragma unroll
      for (int j = 0; j < NN; ++j) {
        double pc[NN];
#pragma unroll
        for (int r = 0; r < NN; ++r) {
          double t = 0.0;
#pragma unroll
          for (int k = 0; k < NN; ++k) t = fma(HD_SYM(m1, r, k), HD_SYM(tl, k, j), t);
          pc[r] = t;
        }
#pragma unroll
        for (int i = 0; i <= j; ++i) {
          double t = rl[i][j];
#pragma unroll
          for (int k = 0; k < NN; ++k) t = fma(HD_SYM(tl, i, k), pc[k], t);
          ra[i][j] = t;
        }
      }
    } else {
      double pm[NN][NN];
#pragma unroll
      for (int r = 0; r < NN; ++r) {
#pragma unroll
        for (int j = 0; j < NN; ++j) {
          double t = 0.0;
#pragma unroll
          for (int k = 0; k < NN; ++k) t = fma(HD_SYM(m1, r, k), HD_SYM(tl, k, j), t);
          pm[r][j] = t;
        }
      }
      HD_PHASE();
#pragma unroll
      for (int i = 0; i < NN; ++i) {
#pragma unroll
        for (int j = i; j < NN; ++j) {
          double t = rl[i][j];
#pragma unroll
          for (int k = 0; k < NN; ++k) t = fma(HD_SYM(tl, i, k), pm[k][j], t);
          ra[i][j] = t;
        }
      }
    }
  }

  // ---- Lambertian surface: I+ = g x ----
  double gsd = 0.0, grg = 0.0;
#pragma unroll
  for (int i = 0; i < NN; ++i) {
    gsd += Qc.g[i] * sd[i];
#pragma unroll
    for (int j = 0; j < NN; ++j) grg += Qc.g[i] * HD_SYM(ra, i, j) * Qc.g[j];
  }
  double esurf = (1.0 - alb) * bsurf;
  const double dirsurf = f0mu0 * beam_at(L, tauc);
  if (beam) esurf += alb * dirsurf / kPi;
  const double x = (2.0 * alb * gsd + esurf) / (1.0 - 2.0 * alb * grg);
  double ip[NN];
#pragma unroll
  for (int i = 0; i < NN; ++i) ip[i] = Qc.g[i] * x;
  double chk = 0.0;
  {
    double up = 0.0, dn = 0.0;
#pragma unroll
    for (int i = 0; i < NN; ++i) {
      up += Qc.g[i] * ip[i];
      double t = sd[i];
#pragma unroll
      for (int j = 0; j < NN; ++j) t += HD_SYM(ra, i, j) * ip[j];
      dn += Qc.g[i] * t;
    }
    const double f0 = twopi * up, f1 = twopi * dn + dirsurf;
    if (A.flux) {
      double* fo = A.flux + (size_t)s * (L + 1) * 2;
      fo[0] = f0;
      fo[1] = f1;
    }
    if (A.fsurf) {  // band epilogue: the back-substitution sums the surface level too
      A.fsurf[sl] = f0;
      A.fsurf[nsc + sl] = f1;
    }
    chk += f0 + f1;
    if constexpr (FLX) {
      double hu = 0.0, hd_ = 0.0;
#pragma unroll
      for (int i = 0; i < NN; ++i) {
        const double h = c_quad_h[NN - 1][i];
        hu = fma(h, ip[i], hu);
        double t = sd[i];
#pragma unroll
        for (int j = 0; j < NN; ++j) t += HD_SYM(ra, i, j) * ip[j];
        hd_ = fma(h, t, hd_);
      }
      const double bl = A.planck ? A.planckv[sl] : 0.0;  // B at harp level 0
      flx_emit(*F, s, sl, nsc, L, L, f0, f1, 0.5 * hu, 0.5 * hd_, bl);
    }
  }
  A.xsurf[sl] = x;
  if (!isfinite(chk)) st |= kStNonFinite;
  return st;
}

// The frame of the three one-lane sweep kernels: the lane's solve, the layer records'
// accessor, sweep_body and the status write
template <int NN, bool NT, bool FLX, bool SPHER>
__device__ __forceinline__ void sweep_kernel_body(const SweepArgs& A, const FlxArgs* F,
                                                  const SphArgs* P) {
  const long sl = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (sl >= A.nsc) return;
  // hd_solve_flx never orders a chunk column-major (cmaj is 0 on its calls)
  long s = A.s0 + sl;
  if constexpr (!FLX || SPHER) s = solve_of(s, A.cmaj, A.nwave, A.ncol);
  const size_t nsc = A.nsc;
  auto rec_at = [&](int lc) {
    const double2* lp =
        reinterpret_cast<const double2*>(A.scr) + (size_t)lc * RecL<NN>::pairs * nsc + sl;
    return [lp, nsc](int e) { return pair_get<NT>(lp, nsc, e); };
  };
  const int st = sweep_body<NN, NT, FLX, SPHER>(A, sl, s, rec_at, F, P);
  if (st) {
    atomicOr(&A.status[s], st);
    if (st & 0x0F) atomicOr(A.anyerr, 1);
  }
}
template <int NN, bool NT>
__global__ __launch_bounds__(64) void hd_sweep_kernel(SweepArgs A) {
  sweep_kernel_body<NN, NT, false, false>(A, nullptr, nullptr);
}
// hd_solve_flx's sweep: the second functional (RecBF records)
template <int NN, bool NT>
__global__ __launch_bounds__(64) void hd_sweep_flx_kernel(SweepArgs A, FlxArgs F) {
  sweep_kernel_body<NN, NT, true, false>(A, &F, nullptr);
}
// hd_solve_spher / hd_solve_flx_spher: the pseudo-spherical beam
template <int NN, bool NT, bool FLX>
__global__ __launch_bounds__(64) void hd_sweep_spher_kernel(SweepArgs A, FlxArgs F, SphArgs P) {
  sweep_kernel_body<NN, NT, FLX, true>(A, &F, &P);
}

template <int NN, bool PRE, bool NT, bool FLX = false>
__device__ __forceinline__ void backsub_body(const SweepArgs& A, const FlxArgs* F = nullptr);


// ============================================================================
// K2 for nstr 4 and 8 (NN = 2, 4) in NN-lane teams: the adding sweep of
// hd_sweep_kernel with one solve per team, lane i holding row i of every NN x NN
// matrix (A = Ra, R~, T~, W1, ZT, P) and element i of every vector; rows reach
// the team's other lanes by DPP quad permutations (one v_mov_b64_dpp per element,
// no LDS).  At these sizes the one-lane sweep is latency-bound -- a call of a few
// hundred or thousand solves runs one or two waves per SIMD, each walking its
// layers through dependent chains (C1 amars_lw: 16 solves, ~70 us of a ~120 us
// step) -- and NN lanes per solve cut each lane's chain by ~NN and give the SIMDs
// NN times the waves.  The pivot-free LU becomes a Gauss-Jordan elimination of
// [W1 | T~ | v1] with the same pivots (lane i ends with row i of ZT = W1^-1 T~
// and t1_i); records as the one-lane sweep (RecL in, RecB out), so the
// back-substitution kernels are shared.
// ============================================================================
namespace {
// lane k of this lane's NN-lane team (NN = 2: pairs, 4: quads) via quad_perm
template <int NN, int K>
__device__ __forceinline__ double qbc(double x) {
  constexpr int ctrl = NN == 4 ? (K | (K << 2) | (K << 4) | (K << 6))
                               : (K | (K << 2) | ((2 + K) << 4) | ((2 + K) << 6));
  return __builtin_amdgcn_update_dpp(0.0, x, ctrl, 0xF, 0xF, true);
}
// sum over the team (a butterfly: every lane holds the same bits)
template <int NN>
__device__ __forceinline__ double qsum(double x) {
  x += __builtin_amdgcn_update_dpp(0.0, x, 1 | (0 << 2) | (3 << 4) | (2 << 6), 0xF, 0xF, true);
  if constexpr (NN == 4)
    x += __builtin_amdgcn_update_dpp(0.0, x, 2 | (3 << 2) | (0 << 4) | (1 << 6), 0xF, 0xF, true);
  return x;
}
template <int B, int E, class F, int... Is>
__device__ __forceinline__ void qfor_impl(F&& f, std::integer_sequence<int, Is...>) {
  (f(std::integral_constant<int, B + Is>{}), ...);
}
template <int B, int E, class F>
__device__ __forceinline__ void qfor(F&& f) {  // f(k), k = B .. E-1 (compile-time)
  if constexpr (E > B) qfor_impl<B, E>(f, std::make_integer_sequence<int, E - B>{});
}
#define HD_Q(x) decltype(x)::value
}  // namespace

template <int NN>
__global__ __launch_bounds__(64) void hd_sweep_quad_kernel(SweepArgs A) {
  static_assert(NN == 2 || NN == 4, "pair / quad teams");
  const Quad<NN>& Qc = quad<NN>();
  const int lane = (int)threadIdx.x;
  const int i = lane & (NN - 1);
  const long slq = ((long)blockIdx.x * 64 + lane) / NN;
  // a team past the chunk repeats the chunk's last solve and stores nothing: every
  // lane of a quad takes part in its DPP exchanges
  const bool valid = slq < A.nsc;
  const long sl = valid ? slq : A.nsc - 1;
  const long s = solve_of(A.s0 + sl, A.cmaj, A.nwave, A.ncol);
  const int L = A.nlyr;
  const size_t nsc = A.nsc;
  using RL = RecL<NN>;
  using RB = RecB<NN>;
  int st = 0;

  const double mu0 = A.umu0 ? A.umu0[s] : 1.0;
  const double fb = A.fbeam ? A.fbeam[s] : 0.0;
  const bool beam = fb > 0.0 && mu0 > 0.0;
  const double alb = A.albedo ? A.albedo[s] : 0.0;
  if (!(alb >= 0.0) || !(alb <= 1.0)) st |= kStBadInput;
  double top = A.fisot ? A.fisot[s] : 0.0;
  double bsurf = 0.0;
  if (A.planck) {
    bsurf = A.planckv[(size_t)(L + 1) * nsc + sl];
    top += A.planckv[(size_t)(L + 2) * nsc + sl];
  }
  const double twopi = 2.0 * kPi;
  const double rmu0 = beam ? 1.0 / mu0 : 0.0;
  const double f0mu0 = beam ? fb * mu0 : 0.0;
  const double g_i = Qc.g[i];
  // record element e of this solve in a layer's record ([pair][nsc] of double2)
  auto eoff = [&](int e) { return ((size_t)(e >> 1) * nsc + sl) * 2 + (e & 1); };

  double ra[NN];  // row i of the reflection of the stack above
#pragma unroll
  for (int j = 0; j < NN; ++j) ra[j] = 0.0;
  double sd = g_i * top;
  double tauc = 0.0;

  // layer records one layer ahead: a wave walks its layers one after another, and
  // at 16 or 20 000 solves nothing else hides a record load's latency (C1 is one wave)
  double rn[NN], tn[NN], spn, smn, tpn;
  auto fetch = [&](int lc) {
    const double* lb = A.scr + (size_t)lc * RL::pairs * nsc * 2;
#pragma unroll
    for (int j = 0; j < NN; ++j) {
      rn[j] = lb[eoff(RL::R + sym_index<NN>(i, j))];
      tn[j] = lb[eoff(RL::T + sym_index<NN>(i, j))];
    }
    spn = lb[eoff(RL::Sp + i)];
    smn = lb[eoff(RL::Sm + i)];
    tpn = lb[eoff(RL::Tau)];
  };
  fetch(0);
  for (int lc = 0; lc < L; ++lc) {
    double* bb = A.bsub + (size_t)lc * RB::pairs * nsc * 2;
    double r[NN], tr[NN];
#pragma unroll
    for (int j = 0; j < NN; ++j) {
      r[j] = rn[j];
      tr[j] = tn[j];
    }
    const double eb = exp(-tauc * rmu0);
    const double sscale = A.beam_scale ? eb : 1.0;
    const double spl = spn * sscale;
    const double sml = smn * sscale;
    const double taup = tpn;
    fetch(lc + 1 < L ? lc + 1 : lc);

    // level lc (top of layer lc): F_dn = rc . I+ + cs  (A symmetric: column i = row i)
    {
      double rc = 0.0;
#pragma unroll
      for (int j = 0; j < NN; ++j) rc = fma(ra[j], Qc.g[j], rc);
      const double cs = qsum<NN>(g_i * sd);
      if (valid) {
        bb[eoff(RB::Rc + i)] = twopi * rc;
        if (i == 0) bb[eoff(RB::Cs)] = fma(twopi, cs, f0mu0 * eb);
      }
    }
    // W1 = I - R A ; v1 = R Sd + S+
    double w[NN];
#pragma unroll
    for (int j = 0; j < NN; ++j) w[j] = i == j ? 1.0 : 0.0;
    double v = spl;
    qfor<0, NN>([&](auto K) {
      constexpr int k = HD_Q(K);
#pragma unroll
      for (int j = 0; j < NN; ++j) w[j] = fma(-r[k], qbc<NN, k>(ra[j]), w[j]);
      v = fma(r[k], qbc<NN, k>(sd), v);
    });
    // Gauss-Jordan on [W1 | T~ | v1] (the one-lane sweep's LU pivots), rows
    // normalised at the end: lane i ends with d_i [e_i | ZT_i | t1_i]
    double z[NN], d = 1.0;
#pragma unroll
    for (int j = 0; j < NN; ++j) z[j] = tr[j];
    qfor<0, NN>([&](auto K) {
      constexpr int k = HD_Q(K);
      const double pk = qbc<NN, k>(w[k]);
      st |= fabs(pk) > 1.0e-12 ? 0 : kStPivot;
      d = i == k ? pk : d;
      const double f = i == k ? 0.0 : w[k] * rcp_nr(pk);
      qfor<k + 1, NN>([&](auto J) { w[HD_Q(J)] = fma(-f, qbc<NN, k>(w[HD_Q(J)]), w[HD_Q(J)]); });
#pragma unroll
      for (int j = 0; j < NN; ++j) z[j] = fma(-f, qbc<NN, k>(z[j]), z[j]);
      v = fma(-f, qbc<NN, k>(v), v);
    });
    {
      const double rd = rcp_nr(d);
#pragma unroll
      for (int j = 0; j < NN; ++j) z[j] *= rd;  // row i of ZT
      v *= rd;                                  // t1_i
    }
    if (valid) {
#pragma unroll
      for (int j = 0; j < NN; ++j) bb[eoff(RB::Z + j * NN + i)] = z[j];
      bb[eoff(RB::Tv + i)] = v;
    }
    // u = A t1 + Sd ; P = A ZT ; Ra <- R + T P ; Sd <- T u + S-
    double u = sd, p_[NN];
#pragma unroll
    for (int j = 0; j < NN; ++j) p_[j] = 0.0;
    qfor<0, NN>([&](auto K) {
      constexpr int k = HD_Q(K);
      u = fma(ra[k], qbc<NN, k>(v), u);
#pragma unroll
      for (int j = 0; j < NN; ++j) p_[j] = fma(ra[k], qbc<NN, k>(z[j]), p_[j]);
    });
    double sdn = sml;
#pragma unroll
    for (int j = 0; j < NN; ++j) ra[j] = r[j];
    qfor<0, NN>([&](auto K) {
      constexpr int k = HD_Q(K);
#pragma unroll
      for (int j = 0; j < NN; ++j) ra[j] = fma(tr[k], qbc<NN, k>(p_[j]), ra[j]);
      sdn = fma(tr[k], qbc<NN, k>(u), sdn);
    });
    sd = sdn;
    tauc += taup;
  }

  // ---- Lambertian surface: I+ = g x ----
  double rgi = 0.0;
#pragma unroll
  for (int j = 0; j < NN; ++j) rgi = fma(ra[j], Qc.g[j], rgi);
  const double gsd = qsum<NN>(g_i * sd);
  const double grg = qsum<NN>(g_i * rgi);
  double esurf = (1.0 - alb) * bsurf;
  const double dirsurf = f0mu0 * exp(-tauc * rmu0);
  if (beam) esurf += alb * dirsurf / kPi;
  const double x = (2.0 * alb * gsd + esurf) / (1.0 - 2.0 * alb * grg);
  const double up = qsum<NN>(g_i * (g_i * x));
  const double dn = qsum<NN>(g_i * fma(rgi, x, sd));
  const double f0 = twopi * up, f1 = twopi * dn + dirsurf;
  if (valid && i == 0) {
    if (A.flux) {
      double* fo = A.flux + (size_t)s * (L + 1) * 2;
      fo[0] = f0;
      fo[1] = f1;
    }
    if (A.fsurf) {
      A.fsurf[sl] = f0;
      A.fsurf[nsc + sl] = f1;
    }
    A.xsurf[sl] = x;
  }
  if (!isfinite(f0 + f1)) st |= kStNonFinite;
  if (valid && st && i == 0) {
    atomicOr(&A.status[s], st);
    if (st & 0x0F) atomicOr(A.anyerr, 1);
  }
}

// ============================================================================
// K3: per-solve back-substitution bottom -> top.  Split from the adding sweep
// so that it runs at the occupancy of its own small register footprint (the
// sweep's register file allows one wave per SIMD): a pure stream over the
// back-substitution records, I+_top = t + ZT I+_bottom, fluxes per level.
// ============================================================================
// The arithmetic of both back-substitution kernels (identical expression order,
// so a solve's fluxes do not depend on which kernel ran its chunk).  PRE: the
// next layer's record is loaded into registers before this layer is computed.
// FLX (hd_solve_flx): RecBF records; every level's eight components go to F->flx.
template <int NN, bool PRE, bool NT, bool FLX>
__device__ __forceinline__ void backsub_body(const SweepArgs& A, const FlxArgs* F) {
  const Quad<NN>& Qc = quad<NN>();
  const long lane_sl = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = lane_sl < A.nsc;
  const bool band = A.part != nullptr;
  // with the band epilogue every lane of a wave takes part in the cross-lane
  // sums: lanes past the chunk run on the last solve's records with weight 0
  if (!live && !band) return;
  const long sl = live ? lane_sl : A.nsc - 1;
  const long s = solve_of(A.s0 + sl, A.cmaj, A.nwave, A.ncol);
  const int L = A.nlyr;
  const size_t nsc = A.nsc;
  const double twopi = 2.0 * kPi;
  const double x = A.xsurf[sl];
  double ip[NN];
#pragma unroll
  for (int i = 0; i < NN; ++i) ip[i] = Qc.g[i] * x;
  double* fo = A.flux ? A.flux + (size_t)s * (L + 1) * 2 : nullptr;
  double chk = 0.0;
  // band epilogue (cmaj order, q = col*nwave + w): lanes of one column form a
  // run; Hillis-Steele suffix sums inside the run leave the run's total (fixed
  // association order) in its first lane, which stores the wave's partial
  double wgt = 0.0;
  unsigned same = 0;  // bit k: lane + 2^k is in this lane's run
  bool head = false;
  double* pp = nullptr;
  if (band) {
    const long q = A.s0 + lane_sl;
    const long col = q / A.nwave;
    const int lane = (int)(lane_sl & 63);
    wgt = live ? A.wts[q - col * A.nwave] : 0.0;
    for (int k = 0; k < A.rsteps; ++k) {
      const int d = 1 << k;
      const long oc = __shfl_down(col, d);
      if (lane + d < 64 && oc == col) same |= 1u << k;
    }
    head = live && (lane == 0 || q % A.nwave == 0);
    const long wv = lane_sl >> 6;
    const long cfirst = (A.s0 + (wv << 6)) / A.nwave;
    pp = A.part + ((size_t)wv * A.nslot + (size_t)(col - cfirst)) * (L + 1) * 2;
  }
  auto emit = [&](int lev, double up, double dn, bool write_flux) {
    if (write_flux && fo && live) {
      fo[2 * lev] = up;
      fo[2 * lev + 1] = dn;
    }
    if (band) {
      double a = wgt * up, b = wgt * dn;
      for (int k = 0; k < A.rsteps; ++k) {
        const double a2 = __shfl_down(a, 1 << k);
        const double b2 = __shfl_down(b, 1 << k);
        if (same & (1u << k)) {
          a += a2;
          b += b2;
        }
      }
      if (head) {
        pp[2 * lev] = a;
        pp[2 * lev + 1] = b;
      }
    }
  };
  if (band) {  // surface level, from the sweep
    const double f0 = A.fsurf[sl], f1 = A.fsurf[nsc + sl];
    emit(0, f0, f1, false);
  }
  // this layer's record through `get` (RecB element indices: ZT column-major, t,
  // rc, cs)
  using RB = std::conditional_t<FLX, RecBF<NN>, RecB<NN>>;
  auto layer = [&](int lc, auto&& get) {
    double nip[NN];
#pragma unroll
    for (int i = 0; i < NN; ++i) {
      double t = get(RB::Tv + i);
#pragma unroll
      for (int j = 0; j < NN; ++j) t += get(RB::Z + j * NN + i) * ip[j];
      nip[i] = t;
    }
    double up = 0.0, dn = get(RB::Cs);
#pragma unroll
    for (int i = 0; i < NN; ++i) {
      ip[i] = nip[i];
      up += Qc.g[i] * nip[i];
      dn += get(RB::Rc + i) * nip[i];
    }
    const int lev = L - lc;
    emit(lev, twopi * up, dn, true);
    chk += twopi * up + dn;
    if constexpr (FLX) {
      HD_PHASE();  // the level's second functional after its fluxes, not interleaved
      double hu = 0.0, hd_ = get(RB::Ch);
#pragma unroll
      for (int i = 0; i < NN; ++i) {
        hu = fma(c_quad_h[NN - 1][i], nip[i], hu);
        hd_ = fma(get(RB::Rh + i), nip[i], hd_);
      }
      const double bl = A.planck ? A.planckv[(size_t)lev * nsc + sl] : 0.0;
      flx_emit(*F, s, sl, nsc, L, lc, twopi * up, dn, 0.5 * hu, 0.5 * hd_, bl);
      chk += hu + hd_;
    }
  };
  auto rec_ptr = [&](int lc) {
    return reinterpret_cast<const double2*>(A.bsub) + (size_t)lc * RB::pairs * nsc + sl;
  };
  if constexpr (PRE) {
    constexpr int NP = RB::pairs;
    double2 cur[NP], nxt[NP];
    {
      const double2* bp = rec_ptr(L - 1);
#pragma unroll
      for (int e = 0; e < NP; ++e) cur[e] = rec_load<NT>(bp + e * nsc);
    }
    for (int lc = L - 1; lc >= 0; --lc) {
      if (lc > 0) {
        const double2* bp = rec_ptr(lc - 1);
#pragma unroll
        for (int e = 0; e < NP; ++e) nxt[e] = rec_load<NT>(bp + e * nsc);
      }
      layer(lc, [&](int e) { return (e & 1) ? cur[e >> 1].y : cur[e >> 1].x; });
#pragma unroll
      for (int e = 0; e < NP; ++e) cur[e] = nxt[e];
    }
  } else {
    for (int lc = L - 1; lc >= 0; --lc) {
      const double2* bp = rec_ptr(lc);
      layer(lc, [&](int e) { return pair_get<NT>(bp, nsc, e); });
    }
  }
  if (live && !isfinite(chk)) {
    atomicOr(&A.status[s], kStNonFinite);
    atomicOr(A.anyerr, 1);
  }
}

// K3: per-solve back-substitution bottom -> top.  Split from the adding sweep
// so that it runs at the occupancy of its own small register footprint (the
// sweep's register file allows one wave per SIMD): a pure stream over the
// back-substitution records, I+_top = t + ZT I+_bottom, fluxes per level.
// This one runs on the side stream beside the next chunk's layer kernel, so it
// must stay small: at most 96 VGPRs (five waves per SIMD), which fit next to a
// layer-kernel wave as long as that one stays at <= 416 (410 now).  The 16-byte
// record loads want the registers of a whole pair set in flight (8 waves per SIMD,
// 64 VGPRs, spilled).
template <int NN, bool NT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5)))
void hd_backsub_kernel(SweepArgs A) {
  backsub_body<NN, false, NT>(A);
}

// K3 for the last chunk of a call, which nothing overlaps: no occupancy cap,
// a whole layer record in flight at once and the next one loaded while this
// one is computed (the capped kernel issues the 81 loads of a layer in small
// register-limited batches, each waiting out a memory latency).
template <int NN, bool NT>
__global__ __launch_bounds__(64) void hd_backsub_tail_kernel(SweepArgs A) {
  backsub_body<NN, true, NT>(A);
}

// hd_solve_flx's back-substitutions: the same two kernels over RecBF records (two more
// dot products and eight stores per level).  The one that runs beside the next chunk's
// layer kernel has a cap of its own, four waves per SIMD (128 VGPRs; NN = 8: three,
// 168): at hd_backsub_kernel's five it spilled (up to 68 B of scratch at NN 5, 6, 8),
// and at four NN = 8 still did (20 B).
template <int NN, bool NT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NN == 8 ? 3 : 4)))
void hd_backsub_flx_kernel(SweepArgs A, FlxArgs F) {
  backsub_body<NN, false, NT, true>(A, &F);
}
template <int NN, bool NT>
__global__ __launch_bounds__(64) void hd_backsub_flx_tail_kernel(SweepArgs A, FlxArgs F) {
  backsub_body<NN, true, NT, true>(A, &F);
}

// ============================================================================
// K4: fused band epilogue of one chunk (hd_solve_band), per (column, level,
// direction): bflux[c] = (first chunk of c ? 0 : bflux[c]) + the chunk's part,
// summed in wave-point order -- deterministic, no atomics
// ============================================================================
__global__ __launch_bounds__(64) void hd_band_reduce_kernel(BandArgs B) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int per = 2 * B.nlev;
  const long W = B.nwave;
  const long q0 = B.s0, q1 = B.s0 + B.nsc;
  if (B.part) {  // register path, column-major chunk: the waves' run partials
    const long c = q0 / W + tid / per;
    if (c > (q1 - 1) / W) return;
    const int e = (int)(tid % per);
    const long qa = c * W > q0 ? c * W : q0;
    const long qb = ((c + 1) * W < q1 ? (c + 1) * W : q1) - 1;
    double sum = 0.0;
    for (long wv = (qa - q0) >> 6; wv <= (qb - q0) >> 6; ++wv) {
      const long cf = (q0 + (wv << 6)) / W;
      sum += B.part[((size_t)wv * B.nslot + (size_t)(c - cf)) * per + e];
    }
    double* o = B.bflux + (size_t)c * per + e;
    *o = c * W >= q0 ? sum : *o + sum;
  } else {  // team path: the chunk's fluxes, solves s = w*ncol + c in [s0, s1)
    const long c = tid / per;
    if (c >= B.ncol) return;
    const int e = (int)(tid % per);
    const long wa = q0 <= c ? 0 : (q0 - c + B.ncol - 1) / B.ncol;
    if (q1 - 1 < c) return;
    long wb = (q1 - 1 - c) / B.ncol;
    if (wb > W - 1) wb = W - 1;
    if (wa > wb) return;
    double sum = 0.0;
    for (long w = wa; w <= wb; ++w)
      sum += B.wts[w] * B.fchunk[(size_t)(w * B.ncol + c - q0) * per + e];
    double* o = B.bflux + (size_t)c * per + e;
    *o = wa == 0 ? sum : *o + sum;
  }
}

hipError_t launch_band_reduce(const BandArgs& ba, hipStream_t stream) {
  long n;
  if (ba.part) {
    n = ((ba.s0 + ba.nsc - 1) / ba.nwave - ba.s0 / ba.nwave + 1) * 2L * ba.nlev;
  } else {
    n = (long)ba.ncol * 2 * ba.nlev;
  }
  // one-wave blocks: on the side stream beside a team layer kernel (two 239-VGPR waves
  // per SIMD) a 4-wave block waited up to 9 ms for a CU with four free wave slots
  hipLaunchKernelGGL(hd_band_reduce_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0,
                     stream, ba);
  return hipGetLastError();
}

// ============================================================================
// host side: constant tables + launchers
// ============================================================================
// ---- warm-start eigenvectors of the team Jacobi (hd_kernels.hpp) ----
namespace {
typedef long double ld_t;
// cyclic two-sided Jacobi of the symmetric n x n a; v <- its eigenvectors (columns)
void host_sym_eig(int n, ld_t (*a)[kMaxNN], ld_t (*v)[kMaxNN]) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) v[i][j] = i == j ? 1.0L : 0.0L;
  for (int sweep = 0; sweep < 64; ++sweep) {
    ld_t off = 0.0L, dia = 0.0L;
    for (int i = 0; i < n; ++i) {
      dia += a[i][i] * a[i][i];
      for (int j = i + 1; j < n; ++j) off += a[i][j] * a[i][j];
    }
    if (!(off > 1.0e-40L * dia)) break;
    for (int p = 0; p < n; ++p)
      for (int q = p + 1; q < n; ++q) {
        const ld_t apq = a[p][q];
        if (apq == 0.0L) continue;
        const ld_t th = (a[q][q] - a[p][p]) / (2.0L * apq);
        const ld_t t = (th >= 0.0L ? 1.0L : -1.0L) / (fabsl(th) + sqrtl(th * th + 1.0L));
        const ld_t c = 1.0L / sqrtl(t * t + 1.0L), s = t * c;
        for (int k = 0; k < n; ++k) {  // columns p, q of a and v
          const ld_t kp = a[k][p], kq = a[k][q];
          a[k][p] = c * kp - s * kq;
          a[k][q] = s * kp + c * kq;
          const ld_t vp = v[k][p], vq = v[k][q];
          v[k][p] = c * vp - s * vq;
          v[k][q] = s * vp + c * vq;
        }
        for (int k = 0; k < n; ++k) {  // rows p, q of a
          const ld_t pk = a[p][k], qk = a[q][k];
          a[p][k] = c * pk - s * qk;
          a[q][k] = s * pk + c * qk;
        }
      }
  }
}
// lower Cholesky factor in place (the upper triangle is zeroed)
void host_chol(int n, ld_t (*a)[kMaxNN]) {
  for (int j = 0; j < n; ++j) {
    ld_t d = a[j][j];
    for (int k = 0; k < j; ++k) d -= a[j][k] * a[j][k];
    const ld_t r = sqrtl(d > 0.0L ? d : 1.0e-300L);
    a[j][j] = r;
    for (int i = j + 1; i < n; ++i) {
      ld_t x = a[i][j];
      for (int k = 0; k < j; ++k) x -= a[i][k] * a[j][k];
      a[i][j] = x / r;
      a[j][i] = 0.0L;
    }
  }
}
}  // namespace

void warm_eigvecs(int nn, const QuadHost& q, int ia, int ib, double* vout) {
  // the layer kernel's S+ = -A+ and S- = -A- for an HG layer at the bin centre
  const int N = 2 * nn;
  const ld_t ssa = (ia + 0.5L) / kWarmG, g = (ib + 0.5L) / kWarmG;
  const ld_t f = powl(g, (ld_t)N);
  const ld_t om = ssa * (1.0L - f) / (1.0L - ssa * f), rf = om / (1.0L - f);
  ld_t sp[kMaxNN][kMaxNN] = {}, sm[kMaxNN][kMaxNN] = {};
  for (int l = 0; l < N; ++l) {
    const ld_t gl = (2 * l + 1) * ((l == 0 ? 1.0L : powl(g, (ld_t)l)) - f) * rf;
    for (int i = 0; i < nn; ++i)
      for (int k = 0; k < nn; ++k) {
        const ld_t x = gl * (ld_t)q.pt[l][i] * (ld_t)q.pt[l][k];
        if (l % 2 == 0) sp[i][k] += x;
        else sm[i][k] += x;
      }
  }
  for (int i = 0; i < nn; ++i)
    for (int k = 0; k < nn; ++k) {
      const ld_t sij = (ld_t)q.sd[i] * (ld_t)q.sd[k];
      const ld_t dg = i == k ? 1.0L / (ld_t)q.mu[i] : 0.0L;
      sp[i][k] = dg - sij * sp[i][k];
      sm[i][k] = dg - sij * sm[i][k];
    }
  host_chol(nn, sm);  // L
  host_chol(nn, sp);  // C
  ld_t b0[kMaxNN][kMaxNN], sym[kMaxNN][kMaxNN], v[kMaxNN][kMaxNN];
  for (int i = 0; i < nn; ++i)
    for (int k = 0; k < nn; ++k) {
      ld_t t = 0.0L;
      for (int m = 0; m < nn; ++m) t += sp[m][i] * sm[m][k];  // (C^T L)_ik
      b0[i][k] = t;
    }
  for (int i = 0; i < nn; ++i)
    for (int k = 0; k < nn; ++k) {
      ld_t t = 0.0L;
      for (int m = 0; m < nn; ++m) t += b0[m][i] * b0[m][k];
      sym[i][k] = t;
    }
  host_sym_eig(nn, sym, v);
  for (int i = 0; i < nn; ++i)
    for (int j = 0; j < nn; ++j) vout[i * nn + j] = (double)v[i][j];
}

template <int NN>
static void fill_quad_s(QuadS<NN>& q, const QuadHost& h) {
  for (int i = 0; i < NN; ++i) {
    q.rmusd[i] = 1.0 / (h.mu[i] * h.sd[i]);
    for (int l = 0; l < 2 * NN; ++l) q.spt[l][i] = h.sd[i] * h.pt[l][i];
  }
}

hipError_t upload_quad_tables(const QuadHost* per_nn /* [kMaxNN], index nn-1 */) {
  QuadTables t;
  fill_quad<1>(t.q1, per_nn[0]);
  fill_quad<2>(t.q2, per_nn[1]);
  fill_quad<3>(t.q3, per_nn[2]);
  fill_quad<4>(t.q4, per_nn[3]);
  fill_quad<5>(t.q5, per_nn[4]);
  fill_quad<6>(t.q6, per_nn[5]);
  fill_quad<7>(t.q7, per_nn[6]);
  fill_quad<8>(t.q8, per_nn[7]);
  double h[kMaxRegNN][kMaxRegNN] = {};
  for (int nn = 1; nn <= kMaxRegNN; ++nn)
    for (int i = 0; i < nn; ++i) h[nn - 1][i] = per_nn[nn - 1].g[i] / per_nn[nn - 1].mu[i];
  hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(c_quad_h), h, sizeof(h), 0, hipMemcpyHostToDevice);
  if (e != hipSuccess) return e;
  QuadSTables s;
  fill_quad_s<1>(s.q1, per_nn[0]);
  fill_quad_s<2>(s.q2, per_nn[1]);
  fill_quad_s<3>(s.q3, per_nn[2]);
  fill_quad_s<4>(s.q4, per_nn[3]);
  fill_quad_s<5>(s.q5, per_nn[4]);
  fill_quad_s<6>(s.q6, per_nn[5]);
  fill_quad_s<7>(s.q7, per_nn[6]);
  fill_quad_s<8>(s.q8, per_nn[7]);
  e = hipMemcpyToSymbol(HIP_SYMBOL(c_quad_s), &s, sizeof(s), 0, hipMemcpyHostToDevice);
  if (e != hipSuccess) return e;
  return hipMemcpyToSymbol(HIP_SYMBOL(c_quad), &t, sizeof(t), 0, hipMemcpyHostToDevice);
}

hipError_t launch_prologue(const PlanckArgs* pa, const TaucArgs* ta, hipStream_t stream) {
  hipError_t e = hipSuccess;
  if (ta) {
    hipLaunchKernelGGL(hd_tauc_kernel, dim3((unsigned)((ta->nsc + 255) / 256)), dim3(256), 0,
                       stream, *ta);
    e = hipGetLastError();
  }
  if (pa && e == hipSuccess) {
    const long n0 = (long)pa->nsc * (pa->nlyr + 3);
    hipLaunchKernelGGL(hd_planck_kernel, dim3((unsigned)((n0 + 255) / 256)), dim3(256), 0,
                       stream, *pa);
    e = hipGetLastError();
  }
  return e;
}

hipError_t launch_spher_prologue(const SpherProArgs& pa, hipStream_t stream) {
  hipLaunchKernelGGL(hd_spher_kernel, dim3((unsigned)((pa.nsc + 255) / 256)), dim3(256), 0, stream,
                     pa);
  return hipGetLastError();
}

hipError_t launch_flx_level(const FlxLevelArgs& fa, const SphArgs* sp, hipStream_t stream) {
  const dim3 g((unsigned)((fa.nsc + 255) / 256));
  if (sp) hipLaunchKernelGGL(hd_flx_level_spher_kernel, g, dim3(256), 0, stream, fa, *sp);
  else hipLaunchKernelGGL(hd_flx_level_kernel, g, dim3(256), 0, stream, fa);
  return hipGetLastError();
}

hipError_t launch_layer(int nn, const LayerArgs& la, const SphArgs* sp, hipStream_t stream) {
  if (nn > kMaxRegNN) return launch_team_layer(nn, la, sp, stream);
  return dispatch_nn<1, kMaxRegNN>(nn, [&](auto NNc) {
    constexpr int NN = decltype(NNc)::value;
    const dim3 g((unsigned)(((la.nsc + 63) / 64) *
                            ((la.nlyr + kLayersPerBlock - 1) / kLayersPerBlock)));
    if (sp)
      return launch_nt(la.nsc, g, dim3(kLayerBlock), stream,
                       [](auto NT) { return hd_layer_spher_kernel<NN, NT>; }, la, *sp);
    return launch_nt(la.nsc, g, dim3(kLayerBlock), stream,
                     [](auto NT) { return hd_layer_kernel<NN, NT>; }, la);
  });
}

hipError_t launch_sweep(int nn, const SweepArgs& sa, const FlxArgs* fx, const SphArgs* sp,
                        hipStream_t stream) {
  if (nn > kMaxRegNN) return launch_team_sweep(nn, sa, fx, sp, stream);
  return dispatch_nn<1, kMaxRegNN>(nn, [&](auto NNc) {
    constexpr int NN = decltype(NNc)::value;
    const dim3 g((unsigned)((sa.nsc + 63) / 64)), b(64);
    if (sp && fx)
      return launch_nt(sa.nsc, g, b, stream,
                       [](auto NT) { return hd_sweep_spher_kernel<NN, NT, true>; }, sa, *fx, *sp);
    if (sp)
      return launch_nt(sa.nsc, g, b, stream,
                       [](auto NT) { return hd_sweep_spher_kernel<NN, NT, false>; }, sa,
                       FlxArgs{}, *sp);
    if (fx)
      return launch_nt(sa.nsc, g, b, stream,
                       [](auto NT) { return hd_sweep_flx_kernel<NN, NT>; }, sa, *fx);
    if constexpr (NN == 2 || NN == 4) {
      if (sa.quad > 0 || (sa.quad < 0 && sa.nsc <= kQuadMaxSolves)) {  // NN-lane teams
        hipLaunchKernelGGL(hd_sweep_quad_kernel<NN>, dim3((unsigned)((sa.nsc * NN + 63) / 64)), b,
                           0, stream, sa);
        return hipGetLastError();
      }
    }
    return launch_nt(sa.nsc, g, b, stream, [](auto NT) { return hd_sweep_kernel<NN, NT>; }, sa);
  });
}

hipError_t launch_backsub(int nn, const SweepArgs& sa, const FlxArgs* fx, hipStream_t stream,
                          bool tail) {
  return dispatch_nn<1, kMaxRegNN>(nn, [&](auto NNc) {
    constexpr int NN = decltype(NNc)::value;
    const dim3 g((unsigned)((sa.nsc + (tail ? 63 : 255)) / (tail ? 64 : 256))), b(tail ? 64 : 256);
    if (fx && tail)
      return launch_nt(sa.nsc, g, b, stream,
                       [](auto NT) { return hd_backsub_flx_tail_kernel<NN, NT>; }, sa, *fx);
    if (fx)
      return launch_nt(sa.nsc, g, b, stream,
                       [](auto NT) { return hd_backsub_flx_kernel<NN, NT>; }, sa, *fx);
    if (tail)
      return launch_nt(sa.nsc, g, b, stream,
                       [](auto NT) { return hd_backsub_tail_kernel<NN, NT>; }, sa);
    return launch_nt(sa.nsc, g, b, stream, [](auto NT) { return hd_backsub_kernel<NN, NT>; }, sa);
  });
}

// the record sizes of hd_plan.hpp (host arithmetic) are those of the kernels' records
static_assert(RecL<8>::pairs == 45 && RecB<8>::pairs == 41, "C4 record pairs");
static_assert(RecBF<8>::pairs == 46 && RecBF<3>::pairs == RecB<3>::pairs + 3, "flx record pairs");

static_assert(layer_record_doubles(8) == 2 * RecL<8>::pairs &&
                  layer_record_doubles(3) == 2 * RecL<3>::pairs &&
                  bsub_record_doubles(8) == 2 * RecB<8>::pairs &&
                  bsub_record_doubles(3) == 2 * RecB<3>::pairs &&
                  bsub_flx_record_doubles(8) == 2 * RecBF<8>::pairs &&
                  bsub_flx_record_doubles(3) == 2 * RecBF<3>::pairs,
              "hd_plan.hpp record sizes");

}  // namespace hd
