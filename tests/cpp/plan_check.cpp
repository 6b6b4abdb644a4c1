// plan_check.cpp -- host-only check of pyharp_amd/csrc/hd_plan.hpp (tests/test_plan_cpu.py
// builds it with g++, under the address and undefined-behaviour sanitizers where their
// runtimes are installed, and runs it): the scratch layout of the flux solves, what
// hd_context_reserve sizes against it, and the automatic chunk policy.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../pyharp_amd/csrc/hd_plan.hpp"

static int g_fail = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      if (++g_fail <= 20) {                       \
        std::printf("FAIL %s: ", #cond);          \
        std::printf(__VA_ARGS__);                 \
        std::printf("\n");                        \
      }                                           \
    }                                             \
  } while (0)

static size_t even(size_t n) { return (n + 1) & ~(size_t)1; }

// The record sizes, written out from the kernels' record layouts (hd_kernels.hpp RecL /
// RecB / RecBF; the team path's rows): not through the header under test.
static size_t ne1_ref(int nn) {
  if (nn <= 8) return 2 * even((size_t)nn * (nn + 1) / 2) + 2 * even(nn) + 2;
  return 2 * (size_t)nn * nn + 2 * nn + 2;
}
static size_t ne2_ref(int nn) {
  if (nn <= 8) return even((size_t)nn * nn) + 2 * even(nn) + 2;
  return ((size_t)nn * nn + 2 * nn + 2) & ~(size_t)1;
}
static size_t ne2f_ref(int nn) {
  if (nn <= 8) return ne2_ref(nn) + even(nn) + 2;
  return ((size_t)nn * nn + 3 * nn + 3) & ~(size_t)1;
}
// the scratch of a call, as hd_solve's enqueue and hd_context_reserve computed it before
// hd_plan.hpp: scratch_doubles_per_solve * chunk + band_extra
static size_t per_solve_ref(int nn, int nlyr, bool planck) {
  return 2 * (ne1_ref(nn) * nlyr + ne2_ref(nn) * nlyr + 1 + (planck ? (size_t)nlyr + 3 : 0) +
              (size_t)nlyr);
}
static size_t band_fused_ref(long chunk, int nwave, int nlyr) {  // register-path band
  return 4 * (size_t)chunk + (size_t)((chunk + 63) / 64) * hd::band_slots(nwave) * 2 * (size_t)(nlyr + 1);
}
static size_t band_local_ref(long chunk, int nlyr) {  // team-path band without caller flux
  return 2 * (size_t)chunk * 2 * (size_t)(nlyr + 1);
}

static void check_plan(int nn, int nlyr, bool planck, bool flx, hd::BandScratch band, int nwave,
                       long chunk) {
  const hd::SolvePlan p(nn, nlyr, planck, flx, band, nwave, chunk);
  const bool used[hd::kNSolveRegions] = {true, true, true, planck, true, flx,
                                         band == hd::kBandFused, band == hd::kBandFused,
                                         band == hd::kBandLocal};
  // the kernels read these in 16-byte pairs (double2): records, and the band buffers
  const bool pairs[hd::kNSolveRegions] = {true, true, false, false, false, false, true, true, true};
  struct Iv { size_t a, b; };
  std::vector<Iv> iv;
  double* const base = reinterpret_cast<double*>(1 << 20);
  for (int r = 0; r < hd::kNSolveRegions; ++r) {
    CHECK((p.len[r] > 0) == used[r], "region %d nn %d nlyr %d chunk %ld", r, nn, nlyr, chunk);
    for (int b = 0; b < p.nbuf[r]; ++b) {
      double* q = p.at(base, (hd::SolveRegion)r, b);
      CHECK((q != nullptr) == used[r], "pointer of region %d", r);
      if (!used[r]) continue;
      const size_t a = (size_t)(q - base);
      CHECK(a == p.off[r] + b * p.len[r], "region %d buffer %d offset", r, b);
      if (pairs[r]) CHECK(a % 2 == 0, "region %d buffer %d at odd double %zu (nn %d chunk %ld)", r, b, a, nn, chunk);
      CHECK(a + p.len[r] <= p.total, "region %d buffer %d ends past the total", r, b);
      iv.push_back({a, a + p.len[r]});
    }
  }
  std::sort(iv.begin(), iv.end(), [](const Iv& x, const Iv& y) { return x.a < y.a; });
  for (size_t i = 1; i < iv.size(); ++i)
    CHECK(iv[i - 1].b <= iv[i].a, "regions overlap (nn %d nlyr %d chunk %ld)", nn, nlyr, chunk);
  size_t want = per_solve_ref(nn, nlyr, planck) * (size_t)chunk;
  if (flx)  // the wider records and the per-level terms [3][nlyr+1], per buffer
    want += 2 * ((ne2f_ref(nn) - ne2_ref(nn)) * nlyr + 3 * (size_t)(nlyr + 1)) * (size_t)chunk;
  if (band == hd::kBandFused) want += band_fused_ref(chunk, nwave, nlyr);
  if (band == hd::kBandLocal) want += band_local_ref(chunk, nlyr);
  CHECK(p.total == want, "total %zu, the formula gives %zu (nn %d nlyr %d planck %d flx %d band %d "
        "nwave %d chunk %ld)", p.total, want, nn, nlyr, planck, flx, (int)band, nwave, chunk);
}

// hd_context_reserve(nsolve) covers every automatically chunked call of at most nsolve
// solves, on either band route at any nwave (the claim of max_auto_chunk's comment)
static void check_reserve(int nn, int nlyr, bool planck, long nsolve) {
  const long cres = std::max<long>(hd::max_auto_chunk(nsolve, nn, nlyr, planck), 1);
  const size_t reserved = hd::solve_reserve_doubles(nn, nlyr, planck, cres);
  const size_t per = per_solve_ref(nn, nlyr, planck);
  CHECK(reserved == per * cres + std::max(band_fused_ref(cres, 1, nlyr), band_local_ref(cres, nlyr)),
        "reserve size nn %d nsolve %ld", nn, nsolve);
  std::vector<char> seen((size_t)cres + 2, 0);
  const int nwaves[] = {1, 2, 3, 16, 63, 64, 65, 1000};
  for (long n = 1; n <= nsolve; ++n) {
    const long c = hd::auto_chunk(n, nn, nlyr, planck);
    CHECK(c >= 1 && c <= cres, "auto_chunk(%ld) = %ld beyond max_auto_chunk(%ld) = %ld", n, c, nsolve, cres);
    if (c < 1 || c > cres || seen[(size_t)c]) continue;
    seen[(size_t)c] = 1;
    for (int caller_flux = 0; caller_flux < 2; ++caller_flux)
      for (int band = 0; band < 2; ++band)
        for (int nwave : nwaves) {
          const hd::SolvePlan p(nn, nlyr, planck, false, hd::band_scratch(nn, band, caller_flux),
                                nwave, c);
          CHECK(p.total <= reserved, "nn %d: a call of %ld solves (chunk %ld, nwave %d) needs %zu > "
                "reserved %zu", nn, n, c, nwave, p.total, reserved);
        }
  }
}

int main() {
  static_assert(hd::layer_record_doubles(8) == 90 && hd::bsub_record_doubles(8) == 82 &&
                hd::bsub_flx_record_doubles(8) == 92, "C4 records: 45, 41 and 46 pairs");
  for (int nn = 1; nn <= hd::kMaxNN; ++nn) {
    CHECK(hd::layer_record_doubles(nn) == ne1_ref(nn), "layer record nn %d", nn);
    CHECK(hd::bsub_record_doubles(nn) == ne2_ref(nn), "bsub record nn %d", nn);
    CHECK(hd::bsub_flx_record_doubles(nn) == ne2f_ref(nn), "flx bsub record nn %d", nn);
    CHECK(hd::layer_record_doubles(nn) % 2 == 0 && hd::bsub_record_doubles(nn) % 2 == 0 &&
          hd::bsub_flx_record_doubles(nn) % 2 == 0, "records in whole pairs nn %d", nn);
  }
  const int nns[] = {1, 2, 4, 8, 9, 12, 16}, nlyrs[] = {1, 7, 80};
  const long chunks[] = {1, 17, 64, 65, 40960};
  const int nwaves[] = {1, 5, 64, 1000};
  for (int nn : nns)
    for (int nlyr : nlyrs)
      for (int planck = 0; planck < 2; ++planck) {
        CHECK(hd::scratch_doubles_per_solve(nn, nlyr, planck) == per_solve_ref(nn, nlyr, planck),
              "per-solve scratch nn %d nlyr %d", nn, nlyr);
        for (int flx = 0; flx < 2; ++flx)
          for (long chunk : chunks) {
            check_plan(nn, nlyr, planck, flx, hd::kBandNone, 1, chunk);
            check_plan(nn, nlyr, planck, flx, hd::kBandLocal, 1, chunk);
            for (int nwave : nwaves) check_plan(nn, nlyr, planck, flx, hd::kBandFused, nwave, chunk);
          }
      }
  // the band mode of a call
  CHECK(hd::band_scratch(8, false, true) == hd::kBandNone && hd::band_scratch(8, true, true) == hd::kBandFused &&
        hd::band_scratch(8, true, false) == hd::kBandFused && hd::band_scratch(9, true, true) == hd::kBandNone &&
        hd::band_scratch(9, true, false) == hd::kBandLocal, "band_scratch");

  for (long nsolve : {16L, 19990L, 65536L, 80000L, 163840L, 640000L})
    for (int planck = 0; planck < 2; ++planck) check_reserve(8, 80, planck, nsolve);
  for (long nsolve : {8000L, 16385L, 64000L})
    for (int planck = 0; planck < 2; ++planck) check_reserve(16, 80, planck, nsolve);

  // tests/test_library.py::test_chunk_plan
  CHECK(hd::auto_chunk(640000, 8, 80, false) == 32000, "C4");
  CHECK(hd::auto_chunk(160000, 8, 80, false) == 32000, "160 000");
  CHECK(hd::auto_chunk(65536, 8, 80, false) == 32768, "65 536");
  CHECK(hd::auto_chunk(80000, 8, 80, false) == 40000, "80 000");
  CHECK(hd::auto_chunk(16, 8, 80, false) == 16, "16");
  CHECK(hd::auto_chunk(64000, 16, 80, false) == 16000, "C5");
  CHECK(hd::auto_chunk(8000, 16, 80, false) == 8000, "C5 rank shape");
  CHECK(hd::auto_chunk(16384, 16, 80, false) == 16384, "16 384");
  CHECK(hd::auto_chunk(16385, 16, 80, false) == 8193, "16 385");
  // the row-major band route starts at (nsolve + 32767) / 32768 >= 5
  CHECK(!hd::band_rowmajor_size(4, 131072) && hd::band_rowmajor_size(4, 131073) &&
        !hd::band_rowmajor_size(9, 640000), "band_rowmajor_size");

  // the intensity and Beer-Lambert layouts: ordered regions inside the total
  for (int planck = 0; planck < 2; ++planck) {
    const hd::RadPlan r(4, 7, planck, 8, 8, 3, 29, 51, 34, 1000, 17);
    CHECK(r.chunk == 17 && r.sw == 0 && r.sw < r.rd && r.rd < r.bs && r.bs < r.lev && r.lev < r.cst &&
          r.cst < r.radm && r.radm < r.taus && r.taus < r.tauc && r.tauc < r.planck &&
          r.planck + (planck ? (size_t)(7 + 3) * 17 : 0) == r.total, "RadPlan");
    const hd::BeerPlan b(7, planck, true, false, 5, 1000, 0);
    CHECK(b.chunk == 1000 && b.planck == 0 && b.xsurf == (planck ? 10u * 1000u : 0u) &&
          b.local == b.xsurf + 1000 && b.total == b.local + 5 * 1000, "BeerPlan");
  }
  CHECK(hd::BeerPlan(7, false, false, true, 16, 1000000, 0).chunk == hd::kBeerChunk &&
        hd::BeerPlan(7, false, false, true, 16, 10, 0).total == 1, "BeerPlan without scratch");

  if (g_fail) {
    std::printf("plan_check: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("plan_check: ok\n");
  return 0;
}
