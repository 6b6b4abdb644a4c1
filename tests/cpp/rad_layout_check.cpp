// CPU check of pyharp_amd/csrc/hd_rad_layout.hpp (plain C++, no HIP), nn = 1..16:
//  - every record layout lists its fields in the documented order, contiguous and
//    non-overlapping, and its size equals the count written out here;
//  - the user-angle maps fit inside the records they overwrite;
//  - both addressings reach every (layer, unit, element) of a buffer exactly once;
//  - fill_rad_tables at the double-Gauss nodes: lam[0][l][i] = P_l(mu_i) (Bonnet's
//    recurrence in long double), the addition theorem
//      sum_{m<=l} (2 - delta_m0) Y_l^m(x) Y_l^m(y) cos(m phi)
//        = P_l(x y + sqrt(1-x^2) sqrt(1-y^2) cos phi)
//    at node pairs of either sign (Y_l^m(-mu) = (-1)^(l+m) Y_l^m(mu)) and four phi for
//    l < 2 nn, and the device recurrence from seed / ra / rb gives the table back.
// Absolute tolerance 5e-13: the recurrence in double deviates by at most 1.0e-14 (m = 0)
// and 4.1e-14 (addition theorem) from numpy's Legendre polynomials over nn = 1..16.
#include <cmath>
#include <cstdio>
#include <utility>
#include <vector>

#include "hd_rad_layout.hpp"

namespace {

int g_fail = 0;
#define CHECK(c, ...)                          \
  do {                                         \
    if (!(c)) {                                \
      ++g_fail;                                \
      std::printf("FAIL %s: ", #c);            \
      std::printf(__VA_ARGS__);                \
      std::printf("\n");                       \
    }                                          \
  } while (0)

struct Field {
  const char* name;
  int off, len;
};

// fields in order: the first at 0, each next where the previous ends, size at the end
void check_fields(const char* rec, int nn, const std::vector<Field>& f, int size, int expect) {
  int at = 0;
  for (const Field& x : f) {
    CHECK(x.off == at, "%s nn %d field %s at %d, expected %d", rec, nn, x.name, x.off, at);
    CHECK(x.len > 0, "%s nn %d field %s is empty", rec, nn, x.name);
    at = x.off + x.len;
  }
  CHECK(size == at, "%s nn %d size %d, fields end at %d", rec, nn, size, at);
  CHECK(size == expect, "%s nn %d size %d, expected %d", rec, nn, size, expect);
}

template <class At>
void check_addressing(const char* name, int size, bool unit_fastest) {
  const int nl = 3, nu = 5;
  std::vector<int> hits((size_t)nl * nu * size, 0);
  int* base = hits.data();
  for (int lc = 0; lc < nl; ++lc)
    for (int u = 0; u < nu; ++u)
      for (int e = 0; e < size; ++e) {
        const size_t o = (size_t)(At::rec(base, size, lc, (size_t)nu, u) - base) + e * At::stride(nu);
        CHECK(o < hits.size(), "%s out of the buffer", name);
        if (o < hits.size()) ++hits[o];
        const size_t want = unit_fastest ? ((size_t)lc * size + e) * nu + u
                                         : ((size_t)lc * nu + u) * size + e;
        CHECK(o == want, "%s (lc %d, u %d, e %d) at %zu, expected %zu", name, lc, u, e, o, want);
      }
  for (int h : hits) CHECK(h == 1, "%s reaches an element %d times", name, h);
}

template <int NN>
void check_layouts() {
  using namespace hd;
  const int nsym = NN * (NN + 1) / 2;
  using O = RadOps<NN>;
  check_fields("RadOps", NN,
               {{"R", O::R, nsym}, {"T", O::T, nsym}, {"Sp", O::Sp, NN}, {"Sm", O::Sm, NN},
                {"Tau", O::Tau, 1}},
               O::size, NN * (NN + 1) + 2 * NN + 1);
  CHECK(O::size == rad_layer_record_doubles(NN), "rad_layer_record_doubles(%d)", NN);
  using R = RadRec<NN>;
  check_fields("RadRec", NN,
               {{"L", R::L, nsym}, {"V", R::V, NN * NN}, {"K", R::K, NN}, {"Zp", R::Zp, NN},
                {"Zm", R::Zm, NN}, {"H", R::H, NN}, {"Bt", R::Bt, 1}, {"Sl", R::Sl, 1},
                {"Tp", R::Tp, 1}, {"Om", R::Om, 1}, {"Ek", R::Ek, NN}, {"E0", R::E0, 1}},
               R::size, nsym + NN * NN + 5 * NN + 5);
  CHECK(R::size == rad_rec_doubles(NN), "rad_rec_doubles(%d)", NN);
  using B = RadBsub<NN>;
  check_fields("RadBsub", NN,
               {{"Z", B::Z, NN * NN}, {"Tv", B::Tv, NN}, {"Ra", B::Ra, nsym}, {"Sd", B::Sd, NN}},
               B::size, NN * NN + 2 * NN + nsym);
  CHECK(B::size == rad_bsub_doubles(NN), "rad_bsub_doubles(%d)", NN);
  using M = RadMap<NN>;
  check_fields("RadMap (rsw)", NN,
               {{"Me", M::Me, NN * NN}, {"Abe", M::Abe, NN}, {"Abo", M::Abo, NN},
                {"Tve", M::Tve, NN}},
               M::ops_size, NN * NN + 3 * NN);
  check_fields("RadMap (bsub)", NN, {{"Mo", M::Mo, NN * NN}, {"Tvo", M::Tvo, NN}}, M::bsub_size,
               NN * NN + NN);
  CHECK(M::ops_size <= O::size, "nn %d: the rsw maps do not fit", NN);
  CHECK(M::bsub_size <= B::size, "nn %d: the bsub maps do not fit", NN);
  check_fields("RadLev", NN, {{"Ip", RadLev<NN>::Ip, NN}, {"Im", RadLev<NN>::Im, NN}},
               RadLev<NN>::size, 2 * NN);
  check_fields("RadCst", NN, {{"Cp", RadCst<NN>::Cp, NN}, {"Cm", RadCst<NN>::Cm, NN}},
               RadCst<NN>::size, 2 * NN);
  // unit fastest up to kMaxRegNN, unit-contiguous above; lev and cst unit fastest always
  check_addressing<RadAt<NN>>("RadAt", R::size, NN <= 8);
  check_addressing<RadElemMajor>("RadElemMajor", RadLev<NN>::size, true);
}

template <int... I>
void check_all_layouts(std::integer_sequence<int, I...>) {
  (check_layouts<I + 1>(), ...);
}

// P_0..P_{n-1} at x by Bonnet's recurrence
void legendre(int n, long double x, long double* p) {
  for (int l = 0; l < n; ++l)
    p[l] = l == 0 ? 1.0L : (l == 1 ? x : ((2 * l - 1) * x * p[l - 1] - (l - 1) * p[l - 2]) / l);
}

// double-Gauss nodes: the Gauss-Legendre nodes of order nn mapped to (0, 1)
std::vector<double> double_gauss(int nn) {
  const long double pi = 3.141592653589793238462643383279502884L;
  std::vector<double> mu(nn);
  std::vector<long double> p(nn + 1);
  for (int i = 0; i < nn; ++i) {
    long double x = std::cos(pi * (i + 0.75L) / (nn + 0.5L));
    for (int it = 0; it < 100; ++it) {
      legendre(nn + 1, x, p.data());
      const long double dp = nn * (x * p[nn] - p[nn - 1]) / (x * x - 1.0L);
      const long double dx = p[nn] / dp;
      x -= dx;
      if (std::fabs(dx) < 1e-19L) break;
    }
    mu[i] = (double)(0.5L * (x + 1.0L));
  }
  return mu;
}

void check_tables(int nn, double& worst0, double& worst_add, double& worst_rec) {
  const double tol = 5e-13;
  const int n2 = 2 * nn;
  const std::vector<double> mu = double_gauss(nn);
  std::vector<double> lam((size_t)n2 * n2 * nn, -7.0);
  static hd::RadCoef coef;
  hd::fill_rad_tables(nn, mu.data(), lam.data());
  hd::fill_rad_coef(coef);
  auto y = [&](int m, int l, int i) { return lam[((size_t)m * n2 + l) * nn + i]; };
  std::vector<long double> p(n2);
  for (int i = 0; i < nn; ++i) {
    CHECK(mu[i] > 0.0 && mu[i] < 1.0, "nn %d node %d = %g", nn, i, mu[i]);
    legendre(n2, mu[i], p.data());
    for (int l = 0; l < n2; ++l) {
      const double d = (double)std::fabs((long double)y(0, l, i) - p[l]);
      if (d > worst0) worst0 = d;
      CHECK(d <= tol, "nn %d: lam[0][%d][%d] off P_l by %.3e", nn, l, i, d);
    }
    // the device recurrence (ylm_row) from the coefficients
    for (int m = 0; m < n2; ++m) {
      double seed = coef.seed[m];
      const double s = std::sqrt(std::fmax(0.0, 1.0 - mu[i] * mu[i]));
      for (int a = 0; a < m; ++a) seed *= s;
      double y1 = 0.0, y2 = 0.0;
      for (int l = 0; l < n2; ++l) {
        const double v = l < m ? 0.0
                               : (l == m ? seed
                                         : coef.ra[m][l] * mu[i] * y1 - coef.rb[m][l] * y2);
        const double d = std::fabs(v - y(m, l, i));
        if (d > worst_rec) worst_rec = d;
        CHECK(d <= tol, "nn %d: recurrence at m %d l %d node %d off the table by %.3e", nn, m, l,
              i, d);
        y2 = y1;
        y1 = v;
      }
    }
  }
  const double phis[4] = {0.0, 0.7, 2.1, 3.141592653589793};
  const int signs[3][2] = {{1, 1}, {1, -1}, {-1, -1}};
  for (int i = 0; i < nn; ++i)
    for (int j = 0; j < nn; ++j)
      for (const auto& sg : signs)
        for (double phi : phis) {
          const long double x = sg[0] * (long double)mu[i], z = sg[1] * (long double)mu[j];
          const long double ct = x * z + std::sqrt(1.0L - x * x) * std::sqrt(1.0L - z * z) *
                                             std::cos((long double)phi);
          legendre(n2, ct, p.data());
          for (int l = 0; l < n2; ++l) {
            long double acc = 0.0L;
            for (int m = 0; m <= l; ++m) {
              // Y_l^m(-mu) = (-1)^(l+m) Y_l^m(mu)
              const long double yi = (sg[0] < 0 && ((l + m) & 1)) ? -y(m, l, i) : y(m, l, i);
              const long double yj = (sg[1] < 0 && ((l + m) & 1)) ? -y(m, l, j) : y(m, l, j);
              acc += (m == 0 ? 1.0L : 2.0L) * yi * yj * std::cos(m * (long double)phi);
            }
            const double d = (double)std::fabs(acc - p[l]);
            if (d > worst_add) worst_add = d;
            CHECK(d <= tol, "nn %d: addition theorem l %d nodes %d %d off by %.3e", nn, l, i, j, d);
          }
        }
}

}  // namespace

int main() {
  static_assert(hd::kMaxNN == 16 && hd::kMaxRegNN == 8, "the cases below are for nn 1..16");
  check_all_layouts(std::make_integer_sequence<int, 16>{});
  double w0 = 0.0, wa = 0.0, wr = 0.0;
  for (int nn = 1; nn <= 16; ++nn) check_tables(nn, w0, wa, wr);
  std::printf("largest deviation: lam[0] vs P_l %.3e, addition theorem %.3e, recurrence %.3e\n",
              w0, wa, wr);
  if (g_fail) {
    std::printf("rad_layout_check: %d failures\n", g_fail);
    return 1;
  }
  std::printf("rad_layout_check: ok\n");
  return 0;
}
