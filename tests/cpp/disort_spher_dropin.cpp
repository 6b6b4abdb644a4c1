// Drop-in check of the pseudo-spherical flux solve at the C++ level: one call of
// harp_amd::DisortImpl::forward with the 'spher' flag, options.radius(...) and the zd
// argument on a small fixed batch (2 waves x 2 columns x 5 layers, nstr 8, a Mars-sized
// body with levels every 20 km, mu0 = 0.5 and 0.1).  Prints one line per value,
//   flux <wave> <col> <level> <dir> <value>        (level 0 = surface)
// which tests/test_gpu_spher.py::test_cpp_dropin compares with the Python call's.
#include <harp_amd/disort.hpp>

#include <cmath>
#include <cstdio>

int main() {
  const int nwave = 2, ncol = 2, nlyr = 5, nstr = 8;
  harp_amd::DisortOptions op;
  op.flags("lamber,quiet,onlyfl,spher");
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
  auto zd = (torch::arange(nlyr + 1, torch::kFloat64) * 2.0e4).to(dev);
  auto flux = disort->forward(prop.to(dev), &bc, torch::Tensor(), zd).cpu();
  if (flux.size(2) != nlyr + 1 || flux.size(3) != 2) return 1;
  auto acc = flux.accessor<double, 4>();
  for (int w = 0; w < nwave; ++w)
    for (int c = 0; c < ncol; ++c)
      for (int l = 0; l <= nlyr; ++l)
        for (int k = 0; k < 2; ++k)
          std::printf("flux %d %d %d %d %.17g\n", w, c, l, k, acc[w][c][l][k]);
  return 0;
}
