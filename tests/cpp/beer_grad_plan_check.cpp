// beer_grad_plan_check.cpp -- host-only check of BeerGradPlan (pyharp_amd/csrc/hd_plan.hpp):
// the scratch of the Beer-Lambert gradient calls.  tests/test_beer_grad_plan_cpu.py builds
// it with g++, under the address and undefined-behaviour sanitizers where their runtimes
// are installed, and runs it.  Checked: the regions the kernels index ([..][chunk], the
// solve fastest) are disjoint, in the order the header documents, and fill the total;
// the chunk respects the caller's bound, the automatic bound and the 16 GB budget.
#include <cstdio>

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

int main() {
  const double budget = 16.0 * 1024.0 * 1024.0 * 1024.0;  // bytes
  const long nsolves[] = {1, 16, 67, 201, 19990, 262144, 1000000, 50000000};
  const long bounds[] = {0, 1, 40, 1000, 300000};
  for (int nn = 1; nn <= 16; ++nn)
    for (int nlyr : {1, 3, 17, 40, 200})
      for (int planck = 0; planck < 2; ++planck)
        for (int rays = 0; rays < 2; ++rays)
          for (long nsolve : nsolves)
            for (long bound : bounds) {
              const hd::BeerGradPlan p(nn, nlyr, planck != 0, rays != 0, nsolve, bound);
              // what the kernels index, written out: planckv and gb [nlyr+3][chunk] with
              // Planck, sweep [nlyr][2 nn][chunk], seed [chunk] for rays
              const size_t c = (size_t)p.chunk;
              const size_t npl = planck ? (size_t)(nlyr + 3) * c : 0;
              const size_t nsw = (size_t)nlyr * 2 * nn * c;
              CHECK(p.chunk >= 1 && p.chunk <= nsolve, "chunk %ld of %ld", p.chunk, nsolve);
              CHECK(bound == 0 || p.chunk <= bound, "chunk %ld over the bound %ld", p.chunk, bound);
              CHECK(p.chunk <= hd::kBeerChunk, "chunk %ld over the automatic bound", p.chunk);
              CHECK(p.planck == 0 && p.gb == npl && p.sweep == 2 * npl && p.seed == p.sweep + nsw,
                    "offsets nn=%d nlyr=%d planck=%d", nn, nlyr, planck);
              CHECK(p.total == p.seed + (rays ? c : 0), "total nn=%d nlyr=%d rays=%d", nn, nlyr, rays);
              CHECK(p.total == p.per_solve * c, "per_solve nn=%d nlyr=%d", nn, nlyr);
              CHECK(8.0 * (double)p.total <= budget || p.chunk == 1, "budget: %zu doubles", p.total);
              // a call that fits the automatic bound and the budget is one chunk
              if (bound == 0 && nsolve <= hd::kBeerChunk && 8.0 * (double)(p.per_solve * nsolve) <= budget)
                CHECK(p.chunk == nsolve, "one chunk for %ld solves, got %ld", nsolve, p.chunk);
            }
  // the budget binds before the automatic bound: nstr 32, 400 layers, 13 606 doubles a solve
  {
    const hd::BeerGradPlan p(16, 400, true, false, 10000000, 0);
    CHECK(p.chunk < hd::kBeerChunk && 8.0 * (double)p.total <= budget &&
              8.0 * (double)(p.per_solve * (size_t)(p.chunk + 1)) > budget,
          "budget-bound chunk %ld", p.chunk);
  }
  if (g_fail) {
    std::printf("beer_grad_plan_check: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("beer_grad_plan_check: ok\n");
  return 0;
}
