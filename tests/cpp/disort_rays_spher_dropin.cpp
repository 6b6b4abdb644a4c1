// Drop-in check of the pseudo-spherical ray radiances at the C++ level: harp_amd::
// DisortImpl::forward_rays and forward_rays_band with the zd argument and
// options.radius(...) on a small fixed batch (2 waves x 2 columns x 5 layers, nstr 8, the
// intensity correction on, a Mars-sized body with levels every 20 km, mu0 = 0.5 and 0.1,
// three shared rays).  Prints one line per value,
//   rad <wave> <col> <depth> <ray> <value>       (depth 0 = top, the user's order)
//   band <col> <depth> <ray> <value>             (weights 0.7, 0.4)
// which tests/test_gpu_rays_spher.py::test_cpp_dropin compares with the Python call's.
#include <harp_amd/disort.hpp>

#include <cmath>
#include <cstdio>

int main() {
  const int nwave = 2, ncol = 2, nlyr = 5, nstr = 8, nray = 3;
  harp_amd::DisortOptions op;
  op.flags("lamber,quiet,intensity_correction,old_intensity_correction");
  op.nwave(nwave).ncol(ncol).radius(3.39e6);
  op.ds().nlyr = nlyr;
  op.ds().nstr = nstr;
  op.ds().nmom = nstr;
  harp_amd::Disort disort(op);

  auto dev = torch::Device(torch::kCUDA, 0);
  auto prop = torch::zeros({nwave, ncol, nlyr, 2 + nstr}, torch::kFloat64);
  for (int w = 0; w < nwave; ++w)
    for (int c = 0; c < ncol; ++c)
      for (int l = 0; l < nlyr; ++l) {
        prop[w][c][l][harp_amd::index::IEX] = 0.1 + 0.05 * l + 0.02 * w;
        prop[w][c][l][harp_amd::index::ISS] = 0.5 + 0.08 * l - 0.1 * c;
        for (int k = 1; k <= nstr; ++k)
          prop[w][c][l][harp_amd::index::IPM + k - 1] = std::pow(0.6 + 0.05 * c, k);
      }
  std::map<std::string, torch::Tensor> bc;
  bc["fbeam"] = torch::full({nwave, ncol}, 1.5, torch::kFloat64).to(dev);
  bc["umu0"] = torch::tensor({0.5, 0.1}, torch::kFloat64).expand({nwave, ncol}).to(dev);
  bc["albedo"] = torch::full({nwave, ncol}, 0.3, torch::kFloat64).to(dev);
  bc["phi0"] = torch::full({nwave, ncol}, 20.0, torch::kFloat64).to(dev);
  auto zd = torch::arange(nlyr + 1, torch::kFloat64) * 2.0e4;  // a CPU tensor: staged like umu
  auto umu = torch::tensor({0.7, -0.02, -1.0}, torch::kFloat64).to(dev);
  auto phi = torch::tensor({10.0, 130.0, 250.0}, torch::kFloat64).to(dev);
  auto rad = disort->forward_rays(prop.to(dev), &bc, torch::Tensor(), umu, phi, zd).cpu();
  if (rad.size(2) != nlyr + 1 || rad.size(3) != nray) return 1;
  auto acc = rad.accessor<double, 4>();
  for (int w = 0; w < nwave; ++w)
    for (int c = 0; c < ncol; ++c)
      for (int l = 0; l <= nlyr; ++l)
        for (int r = 0; r < nray; ++r)
          std::printf("rad %d %d %d %d %.17g\n", w, c, l, r, acc[w][c][l][r]);
  auto wts = torch::tensor({0.7, 0.4}, torch::kFloat64).to(dev);
  auto band = disort->forward_rays_band(prop.to(dev), &bc, torch::Tensor(), umu, phi, wts, nullptr,
                                        zd).cpu();
  if (band.size(0) != ncol || band.size(1) != nlyr + 1 || band.size(2) != nray) return 1;
  auto bacc = band.accessor<double, 3>();
  for (int c = 0; c < ncol; ++c)
    for (int l = 0; l <= nlyr; ++l)
      for (int r = 0; r < nray; ++r) std::printf("band %d %d %d %.17g\n", c, l, r, bacc[c][l][r]);
  return 0;
}
