// hd_rad_layout.hpp -- the single statement of the intensity path's layouts: the
// per-(unit, layer) records its kernels hand to each other (hd_rad.hip, hd_rad_lane.hpp,
// hd_rad_wide.hip, hd_team_mfma.hip), where a record sits in its buffer, and the host
// side of the Y_l^m tables.  Plain C++17, no HIP header (as hd_plan.hpp); checked on
// the CPU by tests/cpp/rad_layout_check.cpp.  A change to a record is made here.
#pragma once

#include <cmath>
#include <cstddef>
#include <type_traits>

#include "hd_plan.hpp"  // kMaxNN, kMaxRegNN

namespace hd {

constexpr int kRadMaxNN = kMaxNN;  // nstr <= 32

// record sizes in doubles (RadOps / RadRec / RadBsub below), for a run-time nn
constexpr int rad_layer_record_doubles(int nn) { return nn * (nn + 1) + 2 * nn + 1; }
constexpr int rad_rec_doubles(int nn) { return nn * (nn + 1) / 2 + nn * nn + 5 * nn + 5; }
constexpr int rad_bsub_doubles(int nn) { return nn * nn + 2 * nn + nn * (nn + 1) / 2; }

// rsw: the layer operators of one (unit, layer), written by the layer kernels for the
// sweeps -- R~ (packed upper, row-major) | T~ (packed upper) | S~+ | S~- | tau'
template <int NN>
struct RadOps {
  static constexpr int nsym = NN * (NN + 1) / 2;
  static constexpr int R = 0, T = R + nsym, Sp = T + nsym, Sm = Sp + NN, Tau = Sm + NN;
  static constexpr int size = Tau + 1;
  static_assert(size == rad_layer_record_doubles(NN), "RadOps");
};

// rrd: the radiance record of one (unit, layer), written by the layer kernels for the
// const, flux and user-angle kernels -- L (packed lower, row-major) | V (row-major) | k |
// Z+ | Z- | h | B_top | dB/dtau' | tau' | omega' | exp(-k tau') | exp(-tau'/mu0)
template <int NN>
struct RadRec {
  static constexpr int nsym = NN * (NN + 1) / 2;
  static constexpr int L = 0, V = L + nsym, K = V + NN * NN, Zp = K + NN, Zm = Zp + NN;
  static constexpr int H = Zm + NN, Bt = H + NN, Sl = Bt + 1, Tp = Sl + 1, Om = Tp + 1;
  static constexpr int Ek = Om + 1, E0 = Ek + NN;
  static constexpr int size = E0 + 1;
  static_assert(size == rad_rec_doubles(NN), "RadRec");
};

// bsub: the sweep's record of one (unit, layer) for the back-substitution --
// ZT (row-major) | t | R_above (packed upper) | S_down
template <int NN>
struct RadBsub {
  static constexpr int nsym = NN * (NN + 1) / 2;
  static constexpr int Z = 0, Tv = Z + NN * NN, Ra = Tv + NN, Sd = Ra + nsym;
  static constexpr int size = Sd + NN;
  static_assert(size == rad_bsub_doubles(NN), "RadBsub");
};

// nstr <= 16 with radiances: the angle-independent maps of one (unit, layer), which the
// const kernel writes over the rsw and bsub records (dead after the sweep) and
// hd_rad_user_map_kernel reads.  rsw: Me (row-major) | abe | abo | tve; bsub: Mo | tvo
template <int NN>
struct RadMap {
  static constexpr int Me = 0, Abe = Me + NN * NN, Abo = Abe + NN, Tve = Abo + NN;
  static constexpr int ops_size = Tve + NN;
  static constexpr int Mo = 0, Tvo = Mo + NN * NN;
  static constexpr int bsub_size = Tvo + NN;
  static_assert(ops_size <= RadOps<NN>::size && bsub_size <= RadBsub<NN>::size,
                "map does not fit");
};

// nstr 18..32 with the team user-angle kernels: the whole-layer source term of user angle
// iu, which hd_rad_team_user_kernel writes over the rsw record (dead after the sweep) at
// element iu and the scan kernel reads -- hence numu <= RadOps<NN>::size on that route
template <int NN>
struct RadLay {
  static constexpr int Lay = 0, capacity = RadOps<NN>::size;
};

// lev: I+ | I- of one (unit, level), solver order; cst: C+ | C- of one (unit, layer)
template <int NN>
struct RadLev {
  static constexpr int Ip = 0, Im = Ip + NN, size = Im + NN;
};
template <int NN>
struct RadCst {
  static constexpr int Cp = 0, Cm = Cp + NN, size = Cm + NN;
};

// Where the record of unit u in layer lc starts in a buffer of nu units, and the
// distance between its elements: element e is rec(...)[e * stride(nu)].
// RadElemMajor: [layer][element][unit], the unit fastest -- the one-lane kernels'
// coalesced layout; lev and cst at every nstr, rsw / rrd / bsub at nstr <= 16.
// RadUnitMajor: [layer][unit][element] -- rsw / rrd / bsub at nstr 18..32, where the
// team kernels write and read them (a team's accesses to one unit's record share lines).
struct RadElemMajor {
  template <class T>
  static constexpr T* rec(T* base, size_t size, size_t lc, size_t nu, size_t u) {
    return base + lc * size * nu + u;
  }
  static constexpr size_t stride(size_t nu) { return nu; }
};
struct RadUnitMajor {
  template <class T>
  static constexpr T* rec(T* base, size_t size, size_t lc, size_t nu, size_t u) {
    return base + (lc * nu + u) * size;
  }
  static constexpr size_t stride(size_t) { return 1; }
};
template <int NN>  // rsw / rrd / bsub
using RadAt = std::conditional_t<(NN <= kMaxRegNN), RadElemMajor, RadUnitMajor>;

// ---- host: the Y_l^m tables ---------------------------------------------------------

template <int NN>
struct RadTab {
  double lam[2 * NN][2 * NN][NN];  // Y_l^m(mu_i): [m][l][i]
};

// the coefficients of the device recurrence (ylm_row, the layer kernels):
// Y_m^m(x) = seed[m] (1 - x^2)^(m/2), Y_l^m = ra[m][l] x Y_{l-1}^m - rb[m][l] Y_{l-2}^m
struct RadCoef {
  double seed[2 * kRadMaxNN];               // prod_{a<=m} sqrt((2a-1)/(2a))
  double ra[2 * kRadMaxNN][2 * kRadMaxNN];  // [m][l] (2l-1)/sqrt(l^2-m^2), l > m
  double rb[2 * kRadMaxNN][2 * kRadMaxNN];  // [m][l] sqrt((l-1)^2-m^2)/sqrt(l^2-m^2)
};

// lam[m][l][i] = Y_l^m(mu[i]) for m, l < 2 nn and the nn nodes mu (lam holds
// 2nn * 2nn * nn doubles)
inline void fill_rad_tables(int nn, const double* mu, double* lam) {
  const int n2 = 2 * nn;
  for (int m = 0; m < n2; ++m)
    for (int i = 0; i < nn; ++i) {
      const double x = mu[i];
      double seed = 1.0;
      for (int a = 1; a <= m; ++a) seed *= std::sqrt((2.0 * a - 1) / (2.0 * a));
      seed *= std::pow(std::sqrt(std::fmax(0.0, 1.0 - x * x)), m);
      double y1 = 0.0, y2 = 0.0;
      for (int l = 0; l < n2; ++l) {
        double v = 0.0;
        if (l == m) v = seed;
        else if (l > m)
          v = ((2.0 * l - 1) * x * y1 - std::sqrt((double)(l - 1) * (l - 1) - (double)m * m) * y2) /
              std::sqrt((double)l * l - (double)m * m);
        lam[((size_t)m * n2 + l) * nn + i] = v;
        y2 = y1;
        y1 = v;
      }
    }
}

inline void fill_rad_coef(RadCoef& coef) {
  for (int m = 0; m < 2 * kRadMaxNN; ++m) {
    double sd = 1.0;
    for (int a = 1; a <= m; ++a) sd *= std::sqrt((2.0 * a - 1) / (2.0 * a));
    coef.seed[m] = sd;
    for (int l = 0; l < 2 * kRadMaxNN; ++l) {
      if (l > m) {
        const double den = std::sqrt((double)l * l - (double)m * m);
        coef.ra[m][l] = (2.0 * l - 1) / den;
        coef.rb[m][l] = std::sqrt((double)(l - 1) * (l - 1) - (double)m * m) / den;
      } else {
        coef.ra[m][l] = coef.rb[m][l] = 0.0;
      }
    }
  }
}

}  // namespace hd
