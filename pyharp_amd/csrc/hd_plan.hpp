// hd_plan.hpp -- the host-side plan of a solve: record sizes, the automatic chunk
// policy and the layout of the context's scratch.  Plain C++17, no HIP header: the
// single statement of the scratch layout, shared by the enqueue functions and
// hd_context_reserve (hd_api.cpp) and checked on the CPU by tests/cpp/plan_check.cpp.
#pragma once

#include <algorithm>
#include <cstddef>

namespace hd {

constexpr int kMaxNN = 16;    // nstr <= 32
constexpr int kMaxRegNN = 8;  // one-lane-per-problem kernels (hd_kernels.hip) up to nstr 16;
                              // 16-lane team kernels (hd_team_mfma.hip) for nstr 18..32

// every group of record elements starts at an even element (RecL / RecB, hd_kernels.hpp)
constexpr int even_up(int n) { return (n + 1) & ~1; }

// register path: records in 16-byte pairs (RecL / RecB), groups padded to even
constexpr size_t reg_pairs_l(int nn) {
  return (size_t)(2 * even_up(nn * (nn + 1) / 2) + 2 * even_up(nn) + 2) / 2;
}
constexpr size_t reg_pairs_b(int nn) {
  return (size_t)(even_up(nn * nn) + 2 * even_up(nn) + 2) / 2;
}

// doubles per (layer, solve) of the layer-operator and back-substitution records
constexpr size_t layer_record_doubles(int nn) {
  if (nn <= kMaxRegNN) return 2 * reg_pairs_l(nn);
  return (size_t)(2 * nn * nn + 2 * nn + 2);  // team layout: full R, T rows (+ pad to even)
}
constexpr size_t bsub_record_doubles(int nn) {
  if (nn <= kMaxRegNN) return 2 * reg_pairs_b(nn);
  return (size_t)((nn * nn + 2 * nn + 2) & ~1);
}
// hd_solve_flx's records (RecBF / the widened team record)
constexpr size_t bsub_flx_record_doubles(int nn) {
  if (nn <= kMaxRegNN) return 2 * reg_pairs_b(nn) + (size_t)even_up(nn) + 2;
  return (size_t)((nn * nn + 3 * nn + 3) & ~1);  // team: the rh row and ch after cs
}

constexpr size_t scratch_doubles_per_solve(int nn, int nlyr, bool planck) {
  // every per-chunk region is double-buffered: chunk k+1's layer kernel (and its
  // tauc/planck prologue) runs beside chunk k's sweep on another stream, and on
  // the register path chunk k's back-substitution beside chunk k+1's layer
  // kernel on a third (see hd_solve)
  const size_t nb = 2;
  return nb * (layer_record_doubles(nn) * nlyr + bsub_record_doubles(nn) * nlyr + 1 +
               (planck ? (size_t)nlyr + 3 : 0) + (size_t)nlyr);
}

// column slots a 64-lane wave of consecutive column-major solves can touch
inline int band_slots(int nwave) { return nwave >= 64 ? 2 : (63 / nwave + 2 < 64 ? 63 / nwave + 2 : 64); }
inline int band_steps(int nwave) {
  int k = 0;
  while ((1 << k) < (nwave < 64 ? nwave : 64)) ++k;
  return k;
}

// ---- chunk policy ------------------------------------------------------------------

constexpr long kRegChunkMax = 40960;  // the register path's largest automatic chunk

// team path: bytes of scratch for the two chunks in flight (the per-solve size counts
// both) within a 16 GB budget
inline long team_chunk_target(int nn, int nlyr, bool planck) {
  const double budget = 16.0 * 1024.0 * 1024.0 * 1024.0;
  const double per = 8.0 * (double)scratch_doubles_per_solve(nn, nlyr, planck);
  return std::min<long>(262144, std::max<long>(16384, (long)(budget / per)));
}

inline long auto_chunk(long nsolve, int nn, int nlyr, bool planck) {
  // NN <= 8: the sweep runs one lane per solve at one wave per SIMD (its register
  // file is full) and cannot share a SIMD with the layer kernel.  Chunks of 32 000-
  // 40 000 solves (500-625 sweep waves) leave 40-50 % of the SIMDs to the next chunk's
  // layer kernel while a sweep runs, instead of the 1 024 waves of a 65 536-solve chunk
  // that take every SIMD: C4 12.80 -> 13.35 M solves/s at 20 chunks of 32 000 (16 of
  // 40 000: 13.27; 24-28 chunks: 12.96-13.03).  With fewer than five chunks the
  // pipeline's fill and drain dominate and the larger chunk wins: the 8-GPU rank shape
  // (80 000) runs 2 x 40 000 at 12.15 M, 3 x 26 667 at 11.78
  // (profiles/r05/chunk_sweep.txt).
  // NN > 8: one 16-lane team per solve; chunks bounded by a scratch budget
  // (the rest of the 288 GB stays the caller's).
  long target;
  if (nn <= kMaxRegNN) {
    target = (nsolve + 32767) / 32768 >= 5 ? 32768 : kRegChunkMax;
  } else {
    target = team_chunk_target(nn, nlyr, planck);
  }
  // (team path: a call that fits one chunk stays one chunk.  Split in two, the 8-GPU
  // C5 rank shape -- 8 000 solves -- ran 1.155 M solves/s against 1.268 M: a 4 000-solve
  // layer kernel takes 2.57 ms alone and 3.63 ms beside the first chunk's sweep,
  // against 4.59 ms for all 8 000, profiles/r05/c5_rank_shape.txt)
  if (nsolve <= target) return nsolve;
  const long n = (nsolve + target - 1) / target;
  return (nsolve + n - 1) / n;
}

// The largest chunk auto_chunk gives any call of at most nsolve solves (the chunk
// size is not monotone in nsolve: 163 840 solves run in chunks of 32 768, 80 000 in
// chunks of 40 000), so hd_context_reserve(nsolve) covers every smaller call too.
inline long max_auto_chunk(long nsolve, int nn, int nlyr, bool planck) {
  const long cap = nn <= kMaxRegNN ? kRegChunkMax : team_chunk_target(nn, nlyr, planck);
  return std::min(nsolve, cap);
}

// hd_solve_band without caller fluxes on the register path, when the call runs as the
// three-stream pipeline of five or more automatic chunks (the 32 768-solve regime): the
// row-major chunks of hd_solve into a per-g flux buffer of the context, then
// hd_band_flux.  C4: 14.80-14.92 M solves/s against 14.33-14.45 M for the column-major
// fused epilogue on one box (profiles/r06/fuse_ab.txt); the 8-GPU rank shape (two
// chunks) is equal and the small shapes keep the fused epilogue.
// (the size predicate; the context's switches are band_rowmajor's in hd_api.cpp)
inline bool band_rowmajor_size(int nn, long nsolve) {
  return nn <= kMaxRegNN && (nsolve + 32767) / 32768 >= 5;
}

// ---- scratch of the flux solves (hd_solve, hd_solve_flx, hd_solve_band) --------------

// what hd_solve_band's fused epilogue keeps in scratch after the chunk regions
enum BandScratch {
  kBandNone,   // no band sum, or the team path summing the caller's flux array
  kBandFused,  // register path: column-major chunks, the surface fluxes of two chunks in
               // flight [2][2][chunk] and one chunk's run partials [wave][nslot][lev][2]
  kBandLocal   // team path without caller fluxes: two chunk flux buffers (the band reduce
               // of chunk k runs on the side stream beside sweep k+1)
};
inline BandScratch band_scratch(int nn, bool band, bool caller_flux) {
  if (!band) return kBandNone;
  if (nn <= kMaxRegNN) return kBandFused;
  return caller_flux ? kBandNone : kBandLocal;
}

enum SolveRegion { kRLayer, kRBsub, kRXsurf, kRPlanck, kRTauc, kRLvl, kRFsurf, kRPart, kRFchunk,
                   kRSph, kNSolveRegions };

// doubles per solve of a pseudo-spherical chunk's prologue region (hd_spher_kernel):
// ch' [nlyr+2] | lambda [nlyr] | ch [nlyr+1] | scaled and unscaled layer depths [2][nlyr]
constexpr size_t spher_doubles(int nlyr) {
  return (size_t)(nlyr + 2) + (size_t)nlyr + (size_t)(nlyr + 1) + 2 * (size_t)nlyr;
}

// Scratch regions, sized for the largest chunk so that no region moves between
// chunks (inside a region the kernels interleave with the chunk's own nsc):
//   layer ops[nb] | bsub[nb] | xsurf[nb] | planck[nb] | tauc[nb] | lvl[nb] (hd_solve_flx:
//   the wider records and the per-level terms [3][nlyr+1]) | band epilogue | sph[nb]
//   (pseudo-spherical plans only: the slant depths and secants, spher_doubles)
// Chunk k uses buffer k & 1 of every per-chunk region (two chunks in flight).
struct SolvePlan {
  size_t off[kNSolveRegions];  // doubles from the base to buffer 0
  size_t len[kNSolveRegions];  // doubles per buffer; 0: the call does not use the region
  int nbuf[kNSolveRegions];
  size_t total;
  int nslot;  // column slots per wave of the fused band epilogue

  SolvePlan(int nn, int nlyr, bool planck, bool flx, BandScratch band, int nwave, long chunk_,
            bool spher = false) {
    const size_t chunk = (size_t)chunk_, nlev2 = 2 * (size_t)(nlyr + 1);
    const size_t ne2 = flx ? bsub_flx_record_doubles(nn) : bsub_record_doubles(nn);
    nslot = band == kBandFused ? band_slots(nwave) : 0;
    for (int r = 0; r < kNSolveRegions; ++r) len[r] = 0, nbuf[r] = 2;
    len[kRLayer] = layer_record_doubles(nn) * nlyr * chunk;
    len[kRBsub] = ne2 * nlyr * chunk;
    len[kRXsurf] = chunk;
    if (planck) len[kRPlanck] = (size_t)(nlyr + 3) * chunk;
    len[kRTauc] = (size_t)nlyr * chunk;
    if (flx) len[kRLvl] = 3 * (size_t)(nlyr + 1) * chunk;
    if (band == kBandFused) {
      len[kRFsurf] = 2 * chunk;
      len[kRPart] = (size_t)((chunk_ + 63) / 64) * nslot * nlev2;
      nbuf[kRPart] = 1;
    } else if (band == kBandLocal) {
      len[kRFchunk] = chunk * nlev2;
    }
    if (spher) len[kRSph] = spher_doubles(nlyr) * chunk;
    size_t q = 0;
    for (int r = 0; r < kNSolveRegions; ++r) off[r] = q, q += nbuf[r] * len[r];
    total = q;
  }
  // buffer `buf` of region r; null where the call does not use the region
  double* at(double* base, SolveRegion r, int buf) const {
    return len[r] ? base + off[r] + (size_t)buf * len[r] : nullptr;
  }
};

// What hd_context_reserve sizes the scratch to for chunks of `chunk` solves: hd_solve,
// and hd_solve_band's epilogue too, at its largest (any nwave) on either route -- so a
// reserved context captures either solve without growing.  (hd_solve_flx's wider
// records are not counted.)
inline size_t solve_reserve_doubles(int nn, int nlyr, bool planck, long chunk) {
  return std::max(SolvePlan(nn, nlyr, planck, false, kBandFused, 1, chunk).total,
                  SolvePlan(nn, nlyr, planck, false, kBandLocal, 1, chunk).total);
}

// ---- scratch of the intensity solves (hd_solve_radiance, hd_solve_rays) ---------------

// rec_sw / rec_rd / rec_bs: doubles per (unit, layer) of the sweep, radiance and
// back-substitution records (hd_rad.hpp); a solve is nm units (azimuthal modes).
// spher (hd_solve_rays_spher only): the prologue's slant depths and secants,
// spher_doubles(nlyr) per solve, after the Planck region
struct RadPlan {
  size_t per_solve;  // modes x (per-unit records + radiance per mode) + prologue
  long chunk;
  size_t sw, rd, bs, lev, cst, radm, taus, tauc, planck, sph;  // offsets (doubles)
  size_t total;

  RadPlan(int nn, int nlyr, bool planck_, int nm, int ntau, int numu, size_t rec_sw,
          size_t rec_rd, size_t rec_bs, long nsolve, long max_chunk, bool spher = false) {
    const size_t u_sw = (size_t)nlyr * rec_sw, u_rd = (size_t)nlyr * rec_rd,
                 u_bs = (size_t)nlyr * rec_bs, u_lev = (size_t)(nlyr + 1) * 2 * nn,
                 u_cst = (size_t)nlyr * 2 * nn, u_radm = (size_t)ntau * numu;
    per_solve = (size_t)nm * (u_sw + u_rd + u_bs + u_lev + u_cst + u_radm) + (size_t)(nlyr + 1) +
                nlyr + (planck_ ? (size_t)nlyr + 3 : 0) + (spher ? spher_doubles(nlyr) : 0);
    // 16 GB of the 288 GB: chunks of ~1e5 units keep every SIMD busy in the per-unit sweep
    const double budget = 16.0 * 1024.0 * 1024.0 * 1024.0 / 8.0;  // doubles
    chunk = std::max<long>(1, std::min<long>(nsolve, (long)(budget / (double)per_solve)));
    chunk = std::min<long>(chunk, 0x7fffffffL / std::max(1, nm));
    if (max_chunk > 0) chunk = std::min(chunk, max_chunk);
    const size_t nuc = (size_t)nm * chunk;  // units of the largest chunk
    size_t q = 0;
    sw = q, q += u_sw * nuc;
    rd = q, q += u_rd * nuc;
    bs = q, q += u_bs * nuc;
    lev = q, q += u_lev * nuc;
    cst = q, q += u_cst * nuc;
    radm = q, q += u_radm * nuc;
    taus = q, q += (size_t)(nlyr + 1) * chunk;
    tauc = q, q += (size_t)nlyr * chunk;
    planck = q, q += (planck_ ? (size_t)nlyr + 3 : 0) * chunk;
    sph = q;
    total = per_solve * (size_t)chunk;
  }
};

// ---- scratch of the Beer-Lambert solves (hd_beer_flux, _flux_band, hd_beer_rays) ------

constexpr long kBeerChunk = 262144;  // solves per automatic chunk

// scratch of one chunk: planck [nlyr+3] | xsurf (rays) | per-wave values (band sum
// without a caller buffer for them; m values per solve)
struct BeerPlan {
  long chunk;
  size_t planck, xsurf, local;  // offsets (doubles)
  size_t total;

  BeerPlan(int nlyr, bool planck_, bool rays, bool caller_out, size_t m, long nsolve,
           long max_chunk) {
    chunk = std::min(nsolve, max_chunk > 0 ? max_chunk : kBeerChunk);
    planck = 0;
    xsurf = planck_ ? (size_t)(nlyr + 3) * chunk : 0;
    local = xsurf + (rays ? (size_t)chunk : 0);
    total = std::max<size_t>(local + (caller_out ? 0 : m * (size_t)chunk), 1);
  }
};

// ---- scratch of the Beer-Lambert gradients (hd_beer_flux_bwd, hd_beer_rays_bwd) --------

// scratch of one chunk: planck [nlyr+3] | gb [nlyr+3], dL/dB per level (both with Planck
// only) | sweep [nlyr][2 nn]: the downward intensities and the upward adjoints entering
// each layer from above, written by the backward kernel's first sweep and read once by
// its second | seed (rays): the sum of the upward rays' adjoints at the surface.
// Every region is laid out [..][chunk], the solve fastest.
struct BeerGradPlan {
  size_t per_solve;
  long chunk;
  size_t planck, gb, sweep, seed;  // offsets (doubles)
  size_t total;

  BeerGradPlan(int nn, int nlyr, bool planck_, bool rays, long nsolve, long max_chunk) {
    const size_t npl = planck_ ? (size_t)nlyr + 3 : 0, nsw = 2 * (size_t)nn * nlyr;
    per_solve = 2 * npl + nsw + (rays ? 1 : 0);
    const double budget = 16.0 * 1024.0 * 1024.0 * 1024.0 / 8.0;  // doubles
    chunk = std::min<long>(kBeerChunk, std::max<long>(1, (long)(budget / (double)per_solve)));
    if (max_chunk > 0) chunk = std::min(chunk, max_chunk);
    chunk = std::max<long>(1, std::min(chunk, nsolve));
    planck = 0;
    gb = npl * chunk;
    sweep = 2 * npl * chunk;
    seed = sweep + nsw * chunk;
    total = per_solve * (size_t)chunk;
  }
};

}  // namespace hd
