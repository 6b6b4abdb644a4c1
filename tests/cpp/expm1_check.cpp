// hd_m_expm1_neg (pyharp_amd/csrc/hd_device.hpp, its host build) against expm1 of long
// double: 1 - exp(-x) at x = 0, denormal x, 1e-300, 2000 points log-spaced in
// [1e-12, 800], the points -1, 0, +1 ulp around n ln2 for n = 1 .. 64, 745, 1e4, +inf.
// Bound: 4 ulp of the result.  Prints the measured maximum.
#define HD_DEVICE_HOST_MATH
#include "../../pyharp_amd/csrc/hd_device.hpp"

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

static double ulp_of(double v) {  // spacing of the doubles at |v|
  const double a = std::fabs(v);
  if (a < DBL_MIN) return std::numeric_limits<double>::denorm_min();
  return std::nextafter(a, INFINITY) - a;
}

int main() {
  std::vector<double> xs = {0.0, std::numeric_limits<double>::denorm_min(), 1.0e-310, 1.0e-300,
                            745.0, 1.0e4, INFINITY};
  for (int i = 0; i < 2000; ++i)
    xs.push_back(std::pow(10.0, -12.0 + (std::log10(800.0) + 12.0) * i / 1999.0));
  const long double ln2l = 0.693147180559945309417232121458176568L;
  for (int n = 1; n <= 64; ++n) {
    const double c = (double)(n * ln2l);
    xs.push_back(std::nextafter(c, 0.0));
    xs.push_back(c);
    xs.push_back(std::nextafter(c, INFINITY));
  }
  // the rounding boundaries of n = rint(x log2 e): odd multiples of ln2 / 2
  for (int n = 0; n < 64; ++n) {
    const double c = (double)((n + 0.5L) * ln2l);
    xs.push_back(std::nextafter(c, 0.0));
    xs.push_back(c);
    xs.push_back(std::nextafter(c, INFINITY));
  }
  double worst = 0.0, worst_x = 0.0;
  int bad = 0;
  for (double x : xs) {
    const double got = hd::hd_m_expm1_neg(x);
    const long double ref = -expm1l(-(long double)x);
    const double refd = (double)ref;
    const double err = (double)(fabsl((long double)got - ref) / (long double)ulp_of(refd));
    if (!(err <= worst)) worst = err, worst_x = x;  // a NaN lands here too
    if (!(err <= 4.0) || !(got >= 0.0) || !(got <= 1.0)) {
      std::printf("FAIL x=%.17g got=%.17g ref=%.17Lg err=%.3f ulp\n", x, got, ref, err);
      ++bad;
    }
  }
  if (hd::hd_m_expm1_neg(0.0) != 0.0 || hd::hd_m_expm1_neg(INFINITY) != 1.0 ||
      hd::hd_m_expm1_neg(1.0e4) != 1.0 || hd::hd_m_expm1_neg(745.0) != 1.0) {
    std::printf("FAIL end values\n");
    ++bad;
  }
  // the lockstep form gives the scalar form's bits
  {
    const double x8[8] = {0.0, 1.0e-9, 0.1, 0.3465735902799727, 1.0, 20.0, 700.0, 1.0e4};
    double m8[8];
    hd::hd_m_expm1_neg_n<8>(x8, m8);
    for (int j = 0; j < 8; ++j)
      if (m8[j] != hd::hd_m_expm1_neg(x8[j])) {
        std::printf("FAIL lockstep j=%d\n", j);
        ++bad;
      }
  }
  std::printf("expm1_check: %zu points, max error %.3f ulp at x = %.17g\n", xs.size(), worst,
              worst_x);
  if (bad) return 1;
  std::printf("expm1_check: ok\n");
  return 0;
}
