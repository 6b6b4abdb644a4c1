// DISOTEST problem 1a (the configuration of tests/cpp/disort_rad_dropin.cpp) along
// outgoing rays: harp's `outdirs` string parsed by harp_amd::parse_radiation_directions
// and evaluated by harp_amd::DisortImpl::forward_rays -- the six published user
// cosines (-1, -0.5, -0.1, 0.1, 0.5, 1) as zenith angles at azimuth 0.  Prints
// "ray <r> <value>" with r = lu * 6 + iu (user depth lu, ray iu), then "band <r>
// <value>" from forward_rays_band with weights 0.1 over the ten identical waves;
// tests/test_gpu_rays.py::test_cpp_disort_rays checks them against DISOTEST's uu.
#include <harp_amd/disort.hpp>

#include <cmath>
#include <cstdio>

int main() {
  harp_amd::DisortOptions op;
  op.header("running disort rays example");
  op.flags("usrtau,lamber,quiet,intensity_correction,old_intensity_correction");
  op.nwave(10);
  op.ds().nlyr = 1;
  op.ds().nstr = 16;
  op.ds().nmom = 16;
  op.user_tau({0, 0.03125});
  harp_amd::Disort disort(op);

  auto prop = torch::zeros({disort->options.nwave(), disort->options.ncol(),
                            disort->ds().nlyr, 2 + disort->ds().nstr},
                           torch::kDouble);
  prop.select(3, harp_amd::index::IEX) = disort->ds().utau[1];
  prop.select(3, harp_amd::index::ISS) = 0.2;
  prop.narrow(3, harp_amd::index::IPM, disort->ds().nstr) = harp_amd::scattering_moments(
      disort->ds().nstr, harp_amd::PhaseMomentOptions().type(harp_amd::kIsotropic));

  std::map<std::string, torch::Tensor> bc;
  bc["umu0"] = 0.1 * torch::ones({disort->options.nwave(), disort->options.ncol()}, torch::kDouble);
  bc["fbeam"] = M_PI / bc["umu0"];

  // zenith = acos(mu) in degrees for mu = -1, -0.5, -0.1, 0.1, 0.5, 1
  auto [umu, phi] = harp_amd::parse_radiation_directions(
      "(180,0) (120,0) (95.73917047726678,0) (84.26082952273322,0) (60,0) (0,0)");
  auto rad = disort->forward_rays(prop, &bc, torch::Tensor(), umu, phi);
  for (int lu = 0; lu < 2; ++lu)
    for (int iu = 0; iu < 6; ++iu)
      std::printf("ray %d %.9e\n", lu * 6 + iu, rad[9][0][lu][iu].item<double>());
  auto w = torch::full({10}, 0.1, torch::kDouble);
  auto brad = disort->forward_rays_band(prop, &bc, torch::Tensor(), umu, phi, w);
  for (int lu = 0; lu < 2; ++lu)
    for (int iu = 0; iu < 6; ++iu)
      std::printf("band %d %.9e\n", lu * 6 + iu, brad[0][lu][iu].item<double>());
  return 0;
}
