// hd_rad.hpp -- argument block and launchers of the intensity path: every
// azimuthal mode, user optical depths and user angles, nstr <= 32.  A unit is one
// (solve, mode) problem.  Which kernel exists in which form:
//   hd_rad.hip       the kernels without NN (taus, azimuth, tms, ray, ray cosines);
//                    (hd_rad_spher.hip compiles its beam-using kernels a second time, with
//                    the pseudo-spherical beam, into hd::spher)
//                    nstr <= 16 only, NN-loops unrolled, one lane per unit: layer,
//                    sweep, user_map; the chunk's launch sequence for every nstr
//   hd_rad_lane.hpp  const and flux, one lane per problem at every nstr: unrolled in
//                    hd_rad.hip (NN 1..8), rolled in hd_rad_wide.hip (hd::wide, NN 9..16)
//   hd_rad_wide.hip  nstr 18..32 only, rolled: user (HD_RAD_USER=rolled, per-column
//                    rays, more user angles than the team kernel takes)
//   hd_team_mfma.hip nstr 18..32 only, four units per wave: layer, sweep, user
// The records these kernels exchange are laid out in hd_rad_layout.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include "hd_kernels.hpp"
#include "hd_rad_layout.hpp"  // the records, their addressing, the Y_l^m table fill

namespace hd {

struct RadArgs {
  // inputs (per solve, index s = s0 + sl)
  const double* prop;
  const double* fbeam;
  const double* umu0;
  const double* albedo;
  const double* fisot;
  const double* phi0;     // [S] degrees or null
  const double* planckv;  // [nlyr+3][ns] or null
  const double* tauc;     // [nlyr][ns] scaled depth of every layer top (beam) or null
  double* taus;           // [nlyr+1][ns] unscaled depth of every level (written by the taus kernel)
  // user grid (device)
  const double* umu;   // [numu]
  const double* phi;   // [nphi] degrees
  const double* utau;  // [ntau] unscaled, ascending; null = the nlyr+1 levels
  // scratch (unit u = m*ns + sl is the fastest index)
  // records and their addressing: hd_rad_layout.hpp
  double* rsw;   // [nlyr][RadOps][nu]   layer operators; nstr > 16: [nlyr][nu][RadOps]
                 //   (team kernels, unit-contiguous)
  double* rrd;   // [nlyr][RadRec][nu]; nstr > 16: [nlyr][nu][RadRec]
  double* bsub;  // [nlyr][RadBsub][nu]; nstr > 16: [nlyr][nu][RadBsub]
  double* lev;   // [nlyr+1][RadLev][nu]  I+ (NN) then I- (NN) per level, solver order
  double* cst;   // [nlyr][RadCst][nu]    C+ then C-
  double* radm;  // [ntau*numu][nu]     radiance per mode
  // outputs
  double* flux;  // [S][ntau][2], index 0 = deepest user depth
  double* uu;    // [S][nphi][ntau][numu]
  int* status;
  int* anyerr;
  long s0;
  int ns;     // solves in this chunk
  int nm;     // azimuthal modes (nstr with a beam and radiances, else 1)
  int nu;     // ns * nm
  int ncol;
  int nlyr;
  int nprop;
  int nmom;
  int planck;
  int max_sweeps;
  int numu, nphi, ntau;
  int corint;  // Nakajima-Tanaka TMS correction of the single scattering
  // nstr <= 16 with radiances: the const kernel also writes each (unit, layer)'s
  // angle-independent maps into the rsw / bsub regions (dead after the sweep) and the
  // user-angle integration runs hd_rad_user_map_kernel
  int umap;
  double* sink;  // team kernels: target of the stores a lane does not own (>= 64 doubles)
  // paired rays (hd_solve_rays): user angle iu is ray iu, umu/phi hold one (cosine,
  // azimuth) pair per ray and hd_rad_ray_kernel replaces the azimuth and TMS kernels
  int umu_stride;  // 0: umu (rays: and phi) shared by every column -- the grid path;
                   // numu: [ncol][numu], column = (s0 + sl) % ncol
  const double* ray_umu;  // rays: the caller's cosines as given (umu holds them with the
                          // bad ones replaced by 1); null = the grid path
  const double* weight;   // rays: [nwave] band weights or null
  double* rad;            // rays: [S][ntau][numu] or null
  double* brad;           // rays: [ncol][ntau][numu] or null (needs weight)
  // pseudo-spherical beam (hd_solve_rays_spher): hd_spher_kernel's
  // slant depths and secants of the chunk (SphArgs' layout, stride ns), read by the nstr <= 16
  // kernels of hd_rad_spher.hip only; null = the plane-parallel beam
  const double* chp;  // [nlyr+2][ns] scaled slant depth ch' per level; row nlyr+1: beam on
  const double* lam;  // [nlyr][ns]   secant of the beam's one exponential per layer
  const double* ch;   // [nlyr+1][ns] unscaled slant depth per level (the IMS step)
};

// The pseudo-spherical beam inside solver layer lc of chunk solve sl (hd_rad_spher.hip): in
// the layer's own scaled depth t in [0, taup] it is exp(-(top + lam t)).  top is ch' of
// the layer's upper level and lam hd_spher_kernel's secant -- except where ch' falls by
// more than kE0Cap through the layer (hd_device.hpp): there the beam is the one that
// reaches the exact exp(-ch'_bottom) with the transmission held at exp(kE0Cap).
struct SphBeam {
  double lam, top;
};
__device__ __forceinline__ SphBeam sph_beam(const RadArgs& A, int lc, int sl, double taup) {
  const double ct = A.chp[(size_t)lc * A.ns + sl];
  const double cb = A.chp[(size_t)(lc + 1) * A.ns + sl];
  SphBeam b{A.lam[(size_t)lc * A.ns + sl], ct};
  if (taup > 0.0 && ct - cb > kE0Cap) {
    b.lam = -kE0Cap / taup;
    b.top = cb + kE0Cap;
  }
  return b;
}
// whether the pseudo-spherical beam of chunk solve sl is on (a valid zd, fbeam > 0, umu0 > 0)
__device__ __forceinline__ bool sph_beam_on(const RadArgs& A, int sl) {
  return A.chp[(size_t)(A.nlyr + 1) * A.ns + sl] != 0.0;
}

// int_{t1}^{t2} a exp(-c (t - tref)) exp(-(t - t1)/mu) dt/mu, t1 = evaluation
// depth, (t2 - t1)/mu >= 0; the 1 + c mu -> 0 limit through (1 - e^-x)/x
__device__ __forceinline__ double seg_exp(double a, double c, double t1, double t2, double tref,
                                          double mu) {
  const double p1 = exp(-c * (t1 - tref));
  const double den = fma(c, mu, 1.0);
  const double dt = (t2 - t1) / mu;
  const double x = den * dt;
  if (fabs(x) < 0.5) {
    const double ph = x == 0.0 ? 1.0 : -expm1(-x) / x;
    return a * p1 * dt * ph;
  }
  const double p2 = exp(-c * (t2 - tref) - dt);
  return a * (p1 - p2) / den;
}

// (pa - pb)/den where pb = pa e^{-y}, y = den * len: the direct quotient, or
// pa * len * (1 - e^-y)/y by its Taylor series when |y| < 1/2 (den -> 0)
__device__ __forceinline__ double dexp(double pa, double pb, double den, double len) {
  const double y = den * len;
  // sum_{n<=13} (-y)^n/(n+1)!: |y|^14/15! < 5e-17 for |y| < 1/2
  double ph = 1.0 / 87178291200.0;  // 1/14!
  ph = fma(ph, -y, 1.0 / 6227020800.0);
  ph = fma(ph, -y, 1.0 / 479001600.0);
  ph = fma(ph, -y, 1.0 / 39916800.0);
  ph = fma(ph, -y, 1.0 / 3628800.0);
  ph = fma(ph, -y, 1.0 / 362880.0);
  ph = fma(ph, -y, 1.0 / 40320.0);
  ph = fma(ph, -y, 1.0 / 5040.0);
  ph = fma(ph, -y, 1.0 / 720.0);
  ph = fma(ph, -y, 1.0 / 120.0);
  ph = fma(ph, -y, 1.0 / 24.0);
  ph = fma(ph, -y, 1.0 / 6.0);
  ph = fma(ph, -y, 0.5);
  ph = fma(ph, -y, 1.0);
  return fabs(y) < 0.5 ? pa * len * ph : (pa - pb) / den;
}

// user depth lu of solve sl: the caller's utau or the level depths
__device__ __forceinline__ double user_tau(const RadArgs& A, int lu, int sl) {
  return A.utau ? A.utau[lu] : A.taus[(size_t)lu * A.ns + sl];
}

// index of user angle iu of solve s in umu (rays: and in phi): the shared list, or the
// list of the solve's column -- s, not the chunk-local sl: a chunk may start mid-wave
__device__ __forceinline__ size_t user_angle(const RadArgs& A, long s, int iu) {
  // stride 0 (uniform across the launch): no integer division on the grid path
  return A.umu_stride ? (size_t)(s % A.ncol) * A.umu_stride + iu : (size_t)iu;
}
__device__ __forceinline__ double user_mu(const RadArgs& A, long s, int iu) {
  return A.umu[user_angle(A, s, iu)];
}

// The one-lane kernels' tables, one object in constant memory per translation unit: the
// quadrature and the Y_l^m table of every NN in [LO, HI]; rad_tabs<NN>(c) is NN's pair
template <int LO, int HI>
struct RadTabs {
  Quad<LO> q;
  RadTab<LO> t;
  RadTabs<LO + 1, HI> next;
};
template <int HI>
struct RadTabs<HI, HI> {
  Quad<HI> q;
  RadTab<HI> t;
};
template <int NN, int LO, int HI>
__host__ __device__ __forceinline__ const RadTabs<NN, HI>& rad_tabs(const RadTabs<LO, HI>& c) {
  if constexpr (NN == LO) return c;
  else return rad_tabs<NN>(c.next);
}
// host: fills the tables from the host quadratures (index nn-1)
template <int LO, int HI>
inline void fill_rad(RadTabs<LO, HI>& c, const QuadHost* per_nn) {
  fill_quad(c.q, per_nn[LO - 1]);
  fill_rad_tables(LO, per_nn[LO - 1].mu, &c.t.lam[0][0][0]);
  if constexpr (LO < HI) fill_rad(c.next, per_nn);
}

// the one-lane kernels of hd_rad.hip at one NN <= kMaxRegNN (null above it) and its two
// ray epilogues (every nstr)
struct RegKernels {
  void (*layer)(RadArgs);
  void (*sweep)(RadArgs);
  void (*cst)(RadArgs);
  void (*flux)(RadArgs);
  void (*user_map)(RadArgs);
  void (*ray)(RadArgs, int);
  void (*ray_band)(RadArgs, int);
};
// nstr <= 16 with the pseudo-spherical beam (RadArgs::chp given): hd_rad.hip's beam-using
// kernels compiled a second time, with HD_RAD_SPHER, from hd_rad_spher.hip -- the kernels
// launch_rad_chunk takes then, and their tables
namespace spher {
hipError_t upload_rad_tables(const QuadHost* per_nn);
RegKernels reg_kernels(int nn);
}  // namespace spher

hipError_t upload_rad_tables(const QuadHost* per_nn);  // nn 1..kRadMaxNN
// tauc/planck prologue must have run (launch_prologue) for the chunk's solves;
// radiances = false: fluxes at the user depths only (mode 0, no uu)
hipError_t launch_rad_chunk(int nn, const RadArgs& a, bool radiances, hipStream_t stream);
// rays: out[i] = umu[i], or 1 where umu[i] is not a valid user cosine (not finite, 0 or
// |umu| > 1), so the user-angle kernels never see such a value; hd_rad_ray_kernel reads
// the caller's array, answers a bad ray with NaN and flags its solves
hipError_t launch_ray_cosines(const double* umu, double* out, long n, hipStream_t stream);
// nstr 18..32: the adding sweep + back-substitution on the team layout with the
// dense products on FP64 MFMA, four units per wave (hd_team_mfma.hip)
hipError_t launch_rad_team_sweep(int nn, const RadArgs& a, hipStream_t stream);
// nstr 18..32: the per-(unit, layer) setup on the team layout + FP64 MFMA, and its
// Y_l^m tables (uploaded with the other intensity-path tables)
hipError_t launch_rad_team_layer(int nn, const RadArgs& a, hipStream_t stream);
// nstr 18..32: the user-angle integration in two kernels -- per (unit, layer) on the
// team layout + FP64 MFMA (every user angle's whole-layer source term and the
// interior user depths' partial integrals), then a per-(unit, angle) scan over the
// layers.  Needs numu <= rad_layer_record_doubles(nn) (the whole-layer terms reuse
// the layer-operator records, free after the sweep)
hipError_t launch_rad_team_user(int nn, const RadArgs& a, hipStream_t stream);
hipError_t upload_rad_tables_team(const QuadHost* per_nn);
// nstr 18..32: the one-lane kernels with rolled NN-loops (hd_rad_wide.hip) -- the
// layers' homogeneous constants (a.nm modes), the fluxes at the user depths, the
// per-(unit, angle) user-angle integration -- and their tables
namespace wide {
hipError_t upload_rad_tables(const QuadHost* per_nn);
hipError_t launch_rad_const(int nn, const RadArgs& a, hipStream_t stream);
hipError_t launch_rad_flux(int nn, const RadArgs& a, hipStream_t stream);
hipError_t launch_rad_user(int nn, const RadArgs& a, hipStream_t stream);
}  // namespace wide

}  // namespace hd
