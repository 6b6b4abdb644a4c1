// harp_amd::BeerLambert (include/harp_amd/beer_lambert.hpp) on a small thermal problem:
// four waves, two columns, five layers of extinction alone (nprop = 1), a grey surface.
// Prints, for column 1, "flux <i> <value>" (forward, i over [wave][level][dir]),
// "bflux <i> <value>" (forward_band, weights 0.1 .. 0.4), "rad <i> <value>"
// (forward_rays with alpha = 1.3, i over [wave][ray], rays 1, 0.5, -0.5) and
// "brad <i> <value>" (forward_rays_band); tests/test_gpu_beer.py::test_cpp_beer_dropin
// checks the lines against the Python module on the same inputs.  CPU tensors in, CPU
// tensors out; forward goes through torch::nn::AnyModule as radiation_band.cpp calls it.
#include <harp_amd/beer_lambert.hpp>

#include <cstdio>

int main() {
  const int nwave = 4, ncol = 2, nlyr = 5;
  std::vector<double> lo, hi;
  for (int w = 0; w < nwave; ++w) {
    lo.push_back(100.0 + 200.0 * w);
    hi.push_back(300.0 + 200.0 * w);
  }
  harp_amd::BeerLambertOptions op;
  op.nstr(8).nwave(nwave).ncol(ncol).nlyr(nlyr).planck(true).wave_lower(lo).wave_upper(hi);
  harp_amd::BeerLambert beer(op);
  harp_amd::BeerLambert beer_alpha(harp_amd::BeerLambertOptions(op).alpha(1.3));

  auto prop = torch::zeros({nwave, ncol, nlyr, 1}, torch::kDouble);
  for (int w = 0; w < nwave; ++w)
    for (int c = 0; c < ncol; ++c)
      for (int l = 0; l < nlyr; ++l) prop[w][c][l][0] = 0.05 * (1 + w) * (1 + l) / (1 + c);
  std::map<std::string, torch::Tensor> bc;
  bc["albedo"] = torch::full({nwave, ncol}, 0.3, torch::kDouble);
  bc["btemp"] = torch::full({nwave, ncol}, 290.0, torch::kDouble);
  auto temf = torch::linspace(280.0, 200.0, nlyr + 1, torch::kDouble).repeat({ncol, 1});
  auto w = torch::tensor(std::vector<double>{0.1, 0.2, 0.3, 0.4}, torch::kDouble);
  auto umu = torch::tensor(std::vector<double>{1.0, 0.5, -0.5}, torch::kDouble);

  auto dump = [](const char* tag, torch::Tensor t) {
    t = t.contiguous().reshape({-1});
    for (int64_t i = 0; i < t.size(0); ++i) std::printf("%s %d %.16e\n", tag, (int)i, t[i].item<double>());
  };
  torch::nn::AnyModule any(beer);
  dump("flux", any.forward(prop, &bc, temf).select(1, 1));
  dump("bflux", beer->forward_band(prop, &bc, temf, w)[1]);
  dump("rad", beer_alpha->forward_rays(prop, &bc, temf, umu).select(1, 1));
  dump("brad", beer_alpha->forward_rays_band(prop, &bc, temf, umu, w)[1]);
  return 0;
}
