// hd_harp_grad.hip -- gfx950 adjoints of the optics step (include/hdharp.h, "Gradients
// of the optics"): hd_attenuate_bwd, hd_band_optics_bwd, hd_band_loop_optics_bwd,
// hd_rfm_attenuate_bwd.
//
// Each adjoint is a recompute of the forward per (wave, col, lyr) and a sum over the
// wave axis, [nwave][ncol][nlyr] -> [ncol][nlyr].  One frame does the sum for all four:
//
//   hd_grad_reduce_kernel<P>   a lane owns one (col, lyr), so consecutive lanes read
//                              consecutive (col, lyr) of the cotangent; it walks blocks of
//                              kWaveBlock consecutive waves, sums each block in ascending
//                              wave order from 0, and either adds the block sums in
//                              ascending block order itself (many columns: grid.y = 1) or
//                              writes each to part[block][value][col, lyr] (few columns:
//                              one block per grid.y)
//   hd_grad_finish_kernel<P>   a wave per (col, lyr) adds the block sums of part in ascending
//                              block order, 64 fetched at a time
//
// The block sums come out of the same loop of the same kernel on either route and the
// additions over blocks are the same sequence, so the routes give the same bits and the
// order is a function of nwave alone.  No atomics.
//
// P (RfmGrad, BandGrad<loop>, AttGrad) supplies the per-lane state (prepare), one wave's
// terms (term) and the write of the totals (emit).  Unlike the forwards this file may
// contract: it owes hd_harp.hip's expression order nothing.
#include <hip/hip_runtime.h>

#include "../../include/hdharp.h"
#include "../../include/hdisort.h"
#include "hd_harp_interp.hpp"
#include "hd_kernels.hpp"

namespace hd {
namespace {

constexpr int kWaveBlock = 32;  // WB of hdharp.h: waves per block of the reduction
constexpr int kMaxAtt = 16;     // as hd_harp.hip
// below this many (col, lyr) a lane per (col, lyr) leaves the device idle: blocks go to
// grid.y and their sums through scratch
constexpr long kDirectLanes = 8192;

unsigned nblk(long n, int b) { return (unsigned)((n + b - 1) / b); }

template <class P>
__global__ __launch_bounds__(256) void hd_grad_reduce_kernel(P prob, int nwave, long ncl,
                                                             int blocks_per_lane, double* part) {
  const long cl = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (cl >= ncl) return;
  const int nwb = (nwave + kWaveBlock - 1) / kWaveBlock;
  const int b0 = (int)blockIdx.y * blocks_per_lane;
  const int b1 = min(nwb, b0 + blocks_per_lane);
  typename P::Lane st;
  prob.prepare(cl, st);
  double tot[P::NOUT];
#pragma unroll
  for (int o = 0; o < P::NOUT; ++o) tot[o] = 0.0;
  for (int b = b0; b < b1; ++b) {
    double blk[P::NOUT];
#pragma unroll
    for (int o = 0; o < P::NOUT; ++o) blk[o] = 0.0;
    const int w1 = min(nwave, (b + 1) * kWaveBlock);
    for (int w = b * kWaveBlock; w < w1; ++w) prob.term(w, cl, ncl, st, blk);
    if (part) {
#pragma unroll
      for (int o = 0; o < P::NOUT; ++o)
        if (o < prob.nout()) part[((size_t)b * prob.nout() + o) * ncl + cl] = blk[o];
    } else {
#pragma unroll
      for (int o = 0; o < P::NOUT; ++o) tot[o] += blk[o];
    }
  }
  if (!part) prob.emit(cl, tot);
}

// a wave per (col, lyr): the lanes fetch 64 blocks' sums at a time (one load latency per 64
// blocks, not per block), then every lane adds them in block order out of its neighbours'
// registers -- the sequence of the lane that walks the blocks itself
template <class P>
__global__ __launch_bounds__(256) void hd_grad_finish_kernel(P prob, int nwb, long ncl,
                                                             const double* part) {
  const long cl = (long)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (cl >= ncl) return;  // whole wave
  const int nout = prob.nout();
  double tot[P::NOUT];
#pragma unroll
  for (int o = 0; o < P::NOUT; ++o) tot[o] = 0.0;
  for (int base = 0; base < nwb; base += 64) {
    const int b = base + lane;
    double v[P::NOUT];
#pragma unroll
    for (int o = 0; o < P::NOUT; ++o)
      v[o] = o < nout && b < nwb ? part[((size_t)b * nout + o) * ncl + cl] : 0.0;
    const int m = min(64, nwb - base);  // (no padding zeros added: -0 + 0 would lose its sign)
    for (int i = 0; i < m; ++i) {
#pragma unroll
      for (int o = 0; o < P::NOUT; ++o)
        if (o < nout) tot[o] += __shfl(v[o], i, 64);
    }
  }
  if (lane == 0) prob.emit(cl, tot);
}

int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    return set_global_error(HD_EHIP, "%s: launch failed: %s", what, hipGetErrorString(e));
  return HD_OK;
}

// the launcher of the frame: nwave > 0, ncl > 0
template <class P>
int reduce_waves(const char* what, const P& prob, int nwave, long ncl, hipStream_t s) {
  const int nwb = (nwave + kWaveBlock - 1) / kWaveBlock;
  if (ncl >= kDirectLanes || nwb == 1 || nwb > 65535) {
    hipLaunchKernelGGL(hd_grad_reduce_kernel<P>, dim3(nblk(ncl, 256)), dim3(256), 0, s, prob,
                       nwave, ncl, nwb, (double*)nullptr);
    return launched(what);
  }
  double* part = nullptr;
  if (hipMallocAsync((void**)&part, (size_t)nwb * prob.nout() * ncl * sizeof(double), s) !=
      hipSuccess) {
    (void)hipGetLastError();
    return set_global_error(HD_ENOMEM, "%s: scratch allocation failed", what);
  }
  hipLaunchKernelGGL(hd_grad_reduce_kernel<P>, dim3(nblk(ncl, 256), nwb), dim3(256), 0, s, prob,
                     nwave, ncl, 1, part);
  hipLaunchKernelGGL(hd_grad_finish_kernel<P>, dim3(nblk(ncl, 4)), dim3(256), 0, s, prob, nwb,
                     ncl, (const double*)part);
  const int rc = launched(what);
  (void)hipFreeAsync(part, s);
  return rc;
}

// ---- RFM ---------------------------------------------------------------------------
// per wave: the wave-axis index pair of the forward and the weight of its second slice
__global__ __launch_bounds__(256) void hd_rfm_wave_bracket_kernel(hd_rfm_table t, int* wi,
                                                                  double* wf) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= t.nwave) return;
  int w1, w2;
  const double x = t.wave[w];
  bracket(t.wave, t.nwave, x, w1, w2);
  const double x1 = t.wave[w1], x2 = t.wave[w2];
  wi[2 * w] = w1;
  wi[2 * w + 1] = w2;
  wf[w] = x2 != x1 ? (x - x1) / (x2 - x1) : 0.0;  // (both slices the same one: weight moot)
}

struct RfmGrad {
  static constexpr int NOUT = 3;  // gconc, gpres, gtemp
  struct Lane {
    size_t o11, o12, o21, o22;  // offsets of the four (ln p, T) corners in a wave's slice
    double fp, ft;              // weights of the second knot (0 where the forward clamps)
    double ip, it;              // 1 / (x2 - x1) per axis, 0 where the forward clamps
    double dtref;               // T_ref'(ln p)
    double invp, c;
  };
  hd_rfm_table t;
  const int* wi;
  const double* wf;
  const double *conc, *pres, *temp, *gout;
  int nspecies;
  double *gconc, *gpres, *gtemp;

  __host__ __device__ int nout() const { return NOUT; }

  // the brackets, the T_ref slope and 1/p depend on (col, lyr) only: once per lane
  __device__ void prepare(long cl, Lane& st) const {
    const double p = pres[cl], lnp = log(p);
    int p1, p2, q1, q2;
    bracket(t.lnp, t.npres, lnp, p1, p2);
    const double xp1 = t.lnp[p1], xp2 = t.lnp[p2];
    st.ip = xp2 != xp1 ? 1.0 / (xp2 - xp1) : 0.0;
    st.fp = (lnp - xp1) * st.ip;
    const double tr1 = t.tref[p1], tr2 = t.tref[p2];
    st.dtref = (tr2 - tr1) * st.ip;
    // T_ref and the anomaly in the forward's own arithmetic: the same T bracket
    const double xt = temp[cl] - lerp_ref(t.lnp, p1, p2, lnp, tr1, tr2);
    bracket(t.tgrid, t.ntemp, xt, q1, q2);
    const double xt1 = t.tgrid[q1], xt2 = t.tgrid[q2];
    st.it = xt2 != xt1 ? 1.0 / (xt2 - xt1) : 0.0;
    st.ft = (xt - xt1) * st.it;
    st.o11 = (size_t)p1 * t.ntemp + q1;
    st.o12 = (size_t)p1 * t.ntemp + q2;
    st.o21 = (size_t)p2 * t.ntemp + q1;
    st.o22 = (size_t)p2 * t.ntemp + q2;
    st.invp = 1.0 / p;
    st.c = conc[cl * nspecies + t.species];
  }

  // value and (ln p, T) slopes of one wave slice
  __device__ void slice(int iw, const Lane& st, double& v, double& dp, double& dt) const {
    const double* d = t.kdata + (size_t)iw * t.npres * t.ntemp;
    const double v11 = d[st.o11], v12 = d[st.o12], v21 = d[st.o21], v22 = d[st.o22];
    const double da = v12 - v11, db = v22 - v21;
    const double a = v11 + st.ft * da, b = v21 + st.ft * db;
    v = a + st.fp * (b - a);
    dp = (b - a) * st.ip;
    dt = (da + st.fp * (db - da)) * st.it;
  }

  __device__ void term(int w, long cl, long ncl, const Lane& st, double* blk) const {
    const int w1 = wi[2 * w], w2 = wi[2 * w + 1];
    const double f = wf[w];
    double v, dp, dt;
    slice(w1, st, v, dp, dt);
    if (f != 0.0) {  // (uniform over the lanes: a table wave sits on its own knot)
      double v2, dp2, dt2;
      slice(w2, st, v2, dp2, dt2);
      v += f * (v2 - v);
      dp += f * (dp2 - dp);
      dt += f * (dt2 - dt);
    }
    const double g = gout[(size_t)w * ncl + cl];
    const double e = 1.E-3 * exp(v);  // recomputed: right at conc = 0
    const double go = g * (e * st.c);
    blk[0] += g * e;
    blk[1] += go * ((dp - dt * st.dtref) * st.invp);
    blk[2] += go * dt;
  }

  __device__ void emit(long cl, const double* tot) const {
    if (gconc) {
      for (int s = 0; s < nspecies; ++s) gconc[cl * nspecies + s] = s == t.species ? tot[0] : 0.0;
    }
    if (gpres) gpres[cl] = tot[1];
    if (gtemp) gtemp[cl] = tot[2];
  }
};

// ---- table attenuators ---------------------------------------------------------------
struct GradTables {
  int nrow[kMaxAtt];
  const double* wl[kMaxAtt];
  const double* k[kMaxAtt];
  const double* s[kMaxAtt];
  const double* g[kMaxAtt];  // HG asymmetry (band loop), or null
  int species[kMaxAtt];
  int natt;
};

// coef[a][w] = {k, ssa, g}(lambda_w), the forward's interpolation
__global__ __launch_bounds__(256) void hd_grad_coef_kernel(GradTables T, const double* coord,
                                                           int kind, int nwave, double* coef) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T.natt * nwave) return;
  const int a = t / nwave, w = t - a * nwave;
  const double x = kind == HD_COORD_WAVENUMBER ? 1.0e4 / coord[w] : coord[w];
  int i1, i2;
  bracket(T.wl[a], T.nrow[a], x, i1, i2);
  coef[(size_t)t * 3] = lerp_ref(T.wl[a], i1, i2, x, T.k[a][i1], T.k[a][i2]);
  coef[(size_t)t * 3 + 1] = lerp_ref(T.wl[a], i1, i2, x, T.s[a][i1], T.s[a][i2]);
  coef[(size_t)t * 3 + 2] = T.g[a] ? lerp_ref(T.wl[a], i1, i2, x, T.g[a][i1], T.g[a][i2]) : 0.0;
}

// hd_attenuate: out0 = k c, out1 = ssa (k c)
struct AttGrad {
  static constexpr int NOUT = 1;
  struct Lane {};
  const double* coef;  // [nwave][3]
  const double* gout;  // [nwave][ncl][2]
  int species, nspecies;
  double* gconc;

  __host__ __device__ int nout() const { return NOUT; }
  __device__ void prepare(long, Lane&) const {}
  __device__ void term(int w, long cl, long ncl, const Lane&, double* blk) const {
    const double* g = gout + ((size_t)w * ncl + cl) * 2;
    const double* cf = coef + (size_t)w * 3;
    blk[0] += cf[0] * (g[0] + cf[1] * g[1]);
  }
  __device__ void emit(long cl, const double* tot) const {
    for (int s = 0; s < nspecies; ++s) gconc[cl * nspecies + s] = s == species ? tot[0] : 0.0;
  }
};

// hd_band_optics (kLoop false) and hd_band_loop_optics (true).  Totals: d/ddz, then one
// per attenuator (d/dc_a).
template <bool kLoop>
struct BandGrad {
  static constexpr int NOUT = kMaxAtt + 1;
  struct Lane {
    double c[kMaxAtt];
    double dz;
  };
  GradTables T;
  const double* coef;  // [natt][nwave][3]
  const double* ext0;  // loop only, or null
  const double *conc, *dz, *gprop;
  int nwave, nspecies, nprop;
  double *gconc, *gdz, *gext0;

  __host__ __device__ int nout() const { return T.natt + 1; }

  __device__ void prepare(long cl, Lane& st) const {
#pragma unroll
    for (int a = 0; a < kMaxAtt; ++a)
      st.c[a] = a < T.natt ? conc[cl * nspecies + T.species[a]] : 0.0;
    st.dz = dz[cl];
  }

  __device__ void term(int w, long cl, long ncl, const Lane& st, double* blk) const {
    const size_t e = (size_t)w * ncl + cl;
    const double* g = gprop + e * nprop;
    const double g0 = g[0], g1 = g[1];
    double h[kMaxAtt];  // h_a = sum_l g_{1+l} chi_al
    double ext = kLoop && ext0 ? ext0[e] : 0.0, sca = 0.0;
#pragma unroll
    for (int a = 0; a < kMaxAtt; ++a) {
      h[a] = 0.0;
      if (a < T.natt) {
        const double* cf = coef + ((size_t)a * nwave + w) * 3;
        const double kc = cf[0] * st.c[a];
        ext += kc;
        sca += cf[1] * kc;
      }
    }
    double dext, dsca, im = 0.0;  // d/dext, d/dsca, 1 / (sca + 1e-10)
    if (kLoop) {
      double sh = 0.0;  // sum_l g_{1+l} m_l = sum_a h_a ssa_a k_a c_a
      if (gconc && nprop > 2) {
#pragma unroll
        for (int a = 0; a < kMaxAtt; ++a) {
          if (a < T.natt && T.g[a]) {
            const double* cf = coef + ((size_t)a * nwave + w) * 3;
            const double ga = cf[2];
            double chi = 1.0, acc = 0.0;
            for (int p = 2; p < nprop; ++p) {
              chi *= ga;
              acc += g[p] * chi;
            }
            h[a] = acc;
            sh += acc * (cf[1] * (cf[0] * st.c[a]));
          }
        }
      }
      const double ie = 1.0 / (ext + 1e-10);
      im = 1.0 / (sca + 1e-10);
      dext = g0 * st.dz - g1 * sca * ie * ie;
      dsca = g1 * ie - sh * im * im;
      if (gext0) gext0[e] = dext;
    } else {
      // ssa = sca / ext, 0 in a layer without extinction: nothing through ssa there
      const double ie = ext != 0.0 ? 1.0 / ext : 0.0;
      dext = g0 * st.dz - g1 * sca * ie * ie;
      dsca = g1 * ie;
    }
    if (gconc) {
#pragma unroll
      for (int a = 0; a < kMaxAtt; ++a)
        if (a < T.natt) {
          const double* cf = coef + ((size_t)a * nwave + w) * 3;
          blk[1 + a] += cf[0] * (dext + cf[1] * (dsca + h[a] * im));
        }
    }
    if (gdz) blk[0] += g0 * ext;
  }

  __device__ void emit(long cl, const double* tot) const {
    if (gconc) {
      for (int sp = 0; sp < nspecies; ++sp) {
        double v = 0.0;  // attenuators of one species add in array order
#pragma unroll
        for (int a = 0; a < kMaxAtt; ++a)
          if (a < T.natt && T.species[a] == sp) v += tot[1 + a];
        gconc[cl * nspecies + sp] = v;
      }
    }
    if (gdz) gdz[cl] = tot[0];
  }
};

int pack_tables(const char* what, const hd_attenuator* atts, int natt, int nspecies,
                GradTables& T) {
  if (natt < 1 || natt > kMaxAtt)
    return set_global_error(HD_EINVAL, "%s: natt=%d not in [1, %d]", what, natt, kMaxAtt);
  T.natt = natt;
  for (int a = 0; a < natt; ++a) {
    const hd_attenuator& at = atts[a];
    T.g[a] = nullptr;
    if (at.nrow < 1 || !at.wavelength || !at.kext || !at.ssa || at.species < 0)
      return set_global_error(HD_EINVAL, "%s: attenuator %d: bad table (nrow=%d species=%d)",
                              what, a, at.nrow, at.species);
    if (at.species >= nspecies)
      return set_global_error(HD_EINVAL, "%s: attenuator %d species %d >= %d", what, a,
                              at.species, nspecies);
    T.nrow[a] = at.nrow;
    T.wl[a] = at.wavelength;
    T.k[a] = at.kext;
    T.s[a] = at.ssa;
    T.species[a] = at.species;
  }
  return HD_OK;
}

bool bad_kind(int kind) { return kind != HD_COORD_WAVELENGTH && kind != HD_COORD_WAVENUMBER; }

// gconc / gdz of a call without waves: zeros
int zero_outputs(const char* what, double* gconc, long nconc, double* a, double* b, long ncl,
                 hipStream_t s) {
  hipError_t e = hipSuccess;
  if (gconc && nconc) e = hipMemsetAsync(gconc, 0, (size_t)nconc * sizeof(double), s);
  if (e == hipSuccess && a && ncl) e = hipMemsetAsync(a, 0, (size_t)ncl * sizeof(double), s);
  if (e == hipSuccess && b && ncl) e = hipMemsetAsync(b, 0, (size_t)ncl * sizeof(double), s);
  if (e != hipSuccess) return set_global_error(HD_EHIP, "%s: memset failed: %s", what, hipGetErrorString(e));
  return HD_OK;
}

// the part of the two band adjoints behind their argument checks
template <bool kLoop>
int band_bwd(const char* what, GradTables& T, const double* ext0, const double* coord, int kind,
             int nwave, const double* conc, int ncol, int nlyr, int nspecies, const double* dz,
             int nprop, const double* gprop, double* gconc, double* gdz, double* gext0,
             hipStream_t s) {
  const long ncl = (long)ncol * nlyr;
  if (ncl == 0) return HD_OK;
  if (nwave == 0) return zero_outputs(what, gconc, ncl * nspecies, gdz, nullptr, ncl, s);
  if (!coord || !conc || !dz || !gprop) return set_global_error(HD_EINVAL, "%s: null array", what);
  if (!gconc && !gdz && !gext0) return HD_OK;
  double* coef = nullptr;
  if (hipMallocAsync((void**)&coef, (size_t)T.natt * nwave * 3 * sizeof(double), s) != hipSuccess) {
    (void)hipGetLastError();
    return set_global_error(HD_ENOMEM, "%s: scratch allocation failed", what);
  }
  hipLaunchKernelGGL(hd_grad_coef_kernel, dim3(nblk((long)T.natt * nwave, 256)), dim3(256), 0, s,
                     T, coord, kind, nwave, coef);
  BandGrad<kLoop> prob{T, coef, ext0, conc, dz, gprop, nwave, nspecies, nprop, gconc, gdz, gext0};
  const int rc = reduce_waves(what, prob, nwave, ncl, s);
  (void)hipFreeAsync(coef, s);
  return rc;
}

}  // namespace
}  // namespace hd

extern "C" {

int hd_attenuate_bwd(const hd_attenuator* att, const double* coord, int coord_kind, int nwave,
                     const double* conc, int ncol, int nlyr, int nspecies, const double* gout,
                     double* gconc, void* stream_) {
  const char* what = "hd_attenuate_bwd";
  if (!att || nwave < 0 || ncol < 0 || nlyr < 0 || nspecies < 1 || hd::bad_kind(coord_kind))
    return hd::set_global_error(HD_EINVAL, "%s: bad arguments", what);
  hd::GradTables T{};
  int rc = hd::pack_tables(what, att, 1, nspecies, T);
  if (rc) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream_);
  const long ncl = (long)ncol * nlyr;
  if (ncl == 0) return HD_OK;
  if (nwave == 0) return hd::zero_outputs(what, gconc, ncl * nspecies, nullptr, nullptr, ncl, s);
  if (!coord || !conc || !gout) return hd::set_global_error(HD_EINVAL, "%s: null array", what);
  if (!gconc) return HD_OK;
  double* coef = nullptr;
  if (hipMallocAsync((void**)&coef, (size_t)nwave * 3 * sizeof(double), s) != hipSuccess) {
    (void)hipGetLastError();
    return hd::set_global_error(HD_ENOMEM, "%s: scratch allocation failed", what);
  }
  hipLaunchKernelGGL(hd::hd_grad_coef_kernel, dim3(hd::nblk(nwave, 256)), dim3(256), 0, s, T,
                     coord, coord_kind, nwave, coef);
  hd::AttGrad prob{coef, gout, att->species, nspecies, gconc};
  rc = hd::reduce_waves(what, prob, nwave, ncl, s);
  (void)hipFreeAsync(coef, s);
  return rc;
}

int hd_band_optics_bwd(const hd_attenuator* atts, int natt, const double* coord, int coord_kind,
                       int nwave, const double* conc, int ncol, int nlyr, int nspecies,
                       const double* dz, int nprop, const double* gprop, double* gconc,
                       double* gdz, void* stream_) {
  const char* what = "hd_band_optics_bwd";
  if (!atts || nwave < 0 || ncol < 0 || nlyr < 0 || nspecies < 1 || nprop < 2 ||
      hd::bad_kind(coord_kind))
    return hd::set_global_error(HD_EINVAL, "%s: bad arguments", what);
  hd::GradTables T{};
  const int rc = hd::pack_tables(what, atts, natt, nspecies, T);
  if (rc) return rc;
  return hd::band_bwd<false>(what, T, nullptr, coord, coord_kind, nwave, conc, ncol, nlyr,
                             nspecies, dz, nprop, gprop, gconc, gdz, nullptr,
                             reinterpret_cast<hipStream_t>(stream_));
}

int hd_band_loop_optics_bwd(const hd_band_attenuator* atts, int natt, const double* ext0,
                            const double* coord, int coord_kind, int nwave, const double* conc,
                            int ncol, int nlyr, int nspecies, const double* dz, int nmom,
                            const double* gprop, double* gconc, double* gdz, double* gext0,
                            void* stream_) {
  const char* what = "hd_band_loop_optics_bwd";
  if (!atts || nwave < 0 || ncol < 0 || nlyr < 0 || nspecies < 1 || nmom < 0 ||
      hd::bad_kind(coord_kind))
    return hd::set_global_error(HD_EINVAL, "%s: bad arguments", what);
  if (natt < 1 || natt > hd::kMaxAtt)
    return hd::set_global_error(HD_EINVAL, "%s: natt=%d not in [1, %d]", what, natt, hd::kMaxAtt);
  hd_attenuator tabs[hd::kMaxAtt];
  for (int a = 0; a < natt; ++a) tabs[a] = atts[a].table;
  hd::GradTables T{};
  const int rc = hd::pack_tables(what, tabs, natt, nspecies, T);
  if (rc) return rc;
  for (int a = 0; a < natt; ++a) T.g[a] = atts[a].gasym;
  return hd::band_bwd<true>(what, T, ext0, coord, coord_kind, nwave, conc, ncol, nlyr, nspecies,
                            dz, 2 + nmom, gprop, gconc, gdz, gext0,
                            reinterpret_cast<hipStream_t>(stream_));
}

int hd_rfm_attenuate_bwd(const hd_rfm_table* t, const double* conc, int ncol, int nlyr,
                         int nspecies, const double* pres, const double* temp,
                         const double* gout, double* gconc, double* gpres, double* gtemp,
                         void* stream_) {
  const char* what = "hd_rfm_attenuate_bwd";
  if (!t || ncol < 0 || nlyr < 0 || nspecies < 1 || t->nwave < 1 || t->npres < 1 ||
      t->ntemp < 1 || t->species < 0 || t->species >= nspecies)
    return hd::set_global_error(HD_EINVAL, "%s: bad arguments", what);
  if (!t->wave || !t->lnp || !t->tgrid || !t->tref || !t->kdata)
    return hd::set_global_error(HD_EINVAL, "%s: null table array", what);
  const long ncl = (long)ncol * nlyr;
  if (ncl == 0) return HD_OK;
  if (!conc || !pres || !temp || !gout) return hd::set_global_error(HD_EINVAL, "%s: null array", what);
  if (!gconc && !gpres && !gtemp) return HD_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream_);
  char* work = nullptr;  // per wave: the index pair (2 ints) and the weight (1 double)
  if (hipMallocAsync((void**)&work, (size_t)t->nwave * 16, s) != hipSuccess) {
    (void)hipGetLastError();
    return hd::set_global_error(HD_ENOMEM, "%s: scratch allocation failed", what);
  }
  double* wf = reinterpret_cast<double*>(work);
  int* wi = reinterpret_cast<int*>(work + (size_t)t->nwave * 8);
  hipLaunchKernelGGL(hd::hd_rfm_wave_bracket_kernel, dim3(hd::nblk(t->nwave, 256)), dim3(256), 0,
                     s, *t, wi, wf);
  hd::RfmGrad prob{*t, wi, wf, conc, pres, temp, gout, nspecies, gconc, gpres, gtemp};
  const int rc = hd::reduce_waves(what, prob, t->nwave, ncl, s);
  (void)hipFreeAsync(work, s);
  return rc;
}

}  // extern "C"
