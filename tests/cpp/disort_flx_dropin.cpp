// Drop-in check of the full flux record at the C++ level: DISOTEST problem 1a
// (isotropic scattering, one layer of tau = 0.03125, ssalb = 0.2, umu0 = 0.1, beam
// pi / umu0, black surface, nstr 16 -- tests/golden/disotest1.json) through
// harp_amd::DisortImpl::forward_flx.  Prints one line per level and component,
//   flx <level> <name> <value>        (level 0 = surface)
// which tests/test_gpu_flx.py::test_cpp_dropin_disotest_1a compares with the CPU
// reference (the driver's published dfdt is 25.4067 at the top, 18.6531 at the bottom).
#include <harp_amd/disort.hpp>

#include <cmath>
#include <cstdio>

int main() {
  const int nwave = 1, ncol = 1, nlyr = 1, nstr = 16;
  harp_amd::DisortOptions op;
  op.flags("lamber,quiet,onlyfl");
  op.nwave(nwave).ncol(ncol);
  op.ds().nlyr = nlyr;
  op.ds().nstr = nstr;
  op.ds().nmom = nstr;
  harp_amd::Disort disort(op);

  auto prop = torch::zeros({nwave, ncol, nlyr, 2 + nstr}, torch::kFloat64);  // isotropic
  prop[0][0][0][harp_amd::index::IEX] = 0.03125;
  prop[0][0][0][harp_amd::index::ISS] = 0.2;
  const double umu0 = 0.1, pi = 3.14159265358979323846;
  std::map<std::string, torch::Tensor> bc;
  bc["fbeam"] = torch::full({nwave, ncol}, pi / umu0, torch::kFloat64);
  bc["umu0"] = torch::full({nwave, ncol}, umu0, torch::kFloat64);
  bc["albedo"] = torch::zeros({nwave, ncol}, torch::kFloat64);
  auto flx = disort->forward_flx(prop, &bc);  // CPU tensors in, a CPU tensor out
  if (flx.is_cuda() || flx.size(3) != harp_amd::index::NFLX) return 1;
  static const char* names[harp_amd::index::NFLX] = {"rfldir", "rfldn",  "flup",   "dfdt",
                                                     "uavg",   "uavgdn", "uavgup", "uavgso"};
  auto acc = flx.accessor<double, 4>();
  for (int l = 0; l <= nlyr; ++l)
    for (int k = 0; k < harp_amd::index::NFLX; ++k)
      std::printf("flx %d %s %.17g\n", l, names[k], acc[0][0][l][k]);
  return 0;
}
