// harp_amd/beer_lambert.hpp -- libtorch module for the reference's second RT solver,
// `BeerLambert` (src/rtsolver/rtsolver.hpp:34-64: BeerLambertOptions with the one option
// `alpha`, BeerLambertImpl::forward(prop, bc, temf)), backed by the MI355X kernels of
// libhdisort.so (C-ABI: include/hdbeer.h).
//
//     harp_amd::BeerLambertOptions op;
//     op.nstr(8).nwave(nwave).ncol(ncol).nlyr(nlyr);
//     op.planck(true).wave_lower(lo).wave_upper(hi);
//     harp_amd::BeerLambert solver(op);
//     auto flux = solver->forward(prop, &bc, temf);                  // (nwave, ncol, nlyr+1, 2)
//     auto toa = solver->forward_rays(prop, &bc, temf, umu);         // (nwave, ncol, nray)
//     auto btoa = solver->forward_rays_band(prop, &bc, temf, umu, w);  // (ncol, nray)
//
// Only prop[..., 0], the layer's optical thickness, is read: extinction is treated as
// absorption.  At ssa = 0 the results are those of harp_amd::Disort, without its linear
// algebra.  nstr is the order of the double-Gauss quadrature of the fluxes.  A ray's
// radiance emerges at the top for umu > 0 (with the alpha term) and at the surface for
// umu < 0.  Tensors may live on the CPU (staged with torch copies, results returned on
// the CPU) or on a ROCm device (torch's current stream).  Errors are raised with
// TORCH_CHECK.
#pragma once

#include <ATen/hip/HIPContext.h>
#include <torch/nn/cloneable.h>
#include <torch/nn/module.h>
#include <torch/nn/modules/container/any.h>
#include <torch/torch.h>

#include <cmath>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../hdbeer.h"

namespace harp_amd {

#define HARP_AMD_BEER_ARG(T, name)                                    \
 public:                                                             \
  inline auto name(const T& v) -> decltype(*this) {                  \
    this->name##_ = v;                                               \
    return *this;                                                    \
  }                                                                  \
  inline const T& name() const noexcept { return this->name##_; }    \
  inline T& name() noexcept { return this->name##_; }                \
                                                                     \
 private:                                                            \
  T name##_

struct BeerLambertOptions {
  BeerLambertOptions() = default;
  //! rays only: the source below the lower boundary grows as (tau / tau_s)^alpha; 0 = off
  HARP_AMD_BEER_ARG(double, alpha) = 0.0;
  HARP_AMD_BEER_ARG(int, nstr) = 8;
  HARP_AMD_BEER_ARG(int, nwave) = 1;
  HARP_AMD_BEER_ARG(int, ncol) = 1;
  HARP_AMD_BEER_ARG(int, nlyr) = 1;
  HARP_AMD_BEER_ARG(bool, planck) = false;
  HARP_AMD_BEER_ARG(std::vector<double>, wave_lower) = {};
  HARP_AMD_BEER_ARG(std::vector<double>, wave_upper) = {};
  HARP_AMD_BEER_ARG(int, device) = 0;
};

class BeerLambertImpl : public torch::nn::Cloneable<BeerLambertImpl> {
 public:
  BeerLambertOptions options;

  BeerLambertImpl() = default;
  explicit BeerLambertImpl(BeerLambertOptions const& op) : options(op) { reset(); }

  void reset() override {
    TORCH_CHECK(options.nstr() >= 2 && options.nstr() % 2 == 0 && options.nstr() <= 32,
                "BeerLambert: nstr must be even and in [2, 32]");
    TORCH_CHECK(options.nlyr() >= 1, "BeerLambert: nlyr must be >= 1");
    TORCH_CHECK(std::isfinite(options.alpha()) && options.alpha() >= 0.0,
                "BeerLambert: alpha must be finite and >= 0");
    if (options.planck())
      TORCH_CHECK((int)options.wave_lower().size() == options.nwave() &&
                      (int)options.wave_upper().size() == options.nwave(),
                  "BeerLambert: planck needs wave_lower/wave_upper of size nwave");
  }

  //! flux (nwave, ncol, nlyr+1, 2); level 0 = surface; [..,0] up, [..,1] down
  torch::Tensor forward(torch::Tensor prop, std::map<std::string, torch::Tensor>* bc,
                        torch::Tensor temf = torch::Tensor()) {
    Batch x = prepare("BeerLambert.forward", prop, bc, temf, /*rays=*/false);
    auto flux = torch::empty({x.nwave, x.ncol, x.nlyr + 1, 2}, x.f64);
    const int rc = hd_beer_flux(context(x.dev.index()), &x.cfg, &x.in, flux.data_ptr<double>(),
                                nullptr, x.stream());
    return finish(x, rc, flux);
  }

  //! band flux (ncol, nlyr+1, 2) = sum_w weights[w] flux[w], one fma per wave in wave
  //! order (bitwise hd_band_sum of forward's result); per-wave fluxes are not stored
  torch::Tensor forward_band(torch::Tensor prop, std::map<std::string, torch::Tensor>* bc,
                             torch::Tensor temf, torch::Tensor weights) {
    Batch x = prepare("BeerLambert.forward_band", prop, bc, temf, /*rays=*/false);
    auto w = band_weights("BeerLambert.forward_band", x, weights);
    auto bflux = torch::empty({x.ncol, x.nlyr + 1, 2}, x.f64);
    hd_band band{w.data_ptr<double>(), bflux.data_ptr<double>()};
    const int rc = hd_beer_flux_band(context(x.dev.index()), &x.cfg, &x.in, &band, nullptr,
                                     nullptr, x.stream());
    return finish(x, rc, bflux);
  }

  //! emergent radiances (nwave, ncol, nray): umu float64 (nray) -- shared -- or
  //! (ncol, nray); at the top for umu > 0, at the surface for umu < 0
  torch::Tensor forward_rays(torch::Tensor prop, std::map<std::string, torch::Tensor>* bc,
                             torch::Tensor temf, torch::Tensor umu) {
    return solve_rays("BeerLambert.forward_rays", prop, bc, temf, umu, torch::Tensor());
  }

  //! band radiance (ncol, nray) = sum_w weights[w] rad[w] (the legacy
  //! btoa(n) += wght[b] * toa(b, n)); per-wave radiances are not stored
  torch::Tensor forward_rays_band(torch::Tensor prop, std::map<std::string, torch::Tensor>* bc,
                                  torch::Tensor temf, torch::Tensor umu, torch::Tensor weights) {
    TORCH_CHECK(weights.defined(), "BeerLambert.forward_rays_band: weights are required");
    return solve_rays("BeerLambert.forward_rays_band", prop, bc, temf, umu, weights);
  }

 protected:
  FORWARD_HAS_DEFAULT_ARGS({2, torch::nn::AnyValue(torch::Tensor())})

 private:
  struct Batch {
    torch::Device dev = torch::kCPU, in_dev = torch::kCPU;
    torch::TensorOptions f64;
    int nwave = 0, ncol = 0, nlyr = 0, nprop = 0;
    torch::Tensor p, tf, wl, wu;
    std::map<std::string, torch::Tensor> b;
    hd_config cfg{};
    hd_inputs in{};
    const double* bp(const char* k) const {
      auto it = b.find(k);
      return it == b.end() ? nullptr : it->second.data_ptr<double>();
    }
    void* stream() const {
      return reinterpret_cast<void*>(at::hip::getCurrentHIPStream(dev.index()).stream());
    }
  };

  torch::Tensor finish(const Batch& x, int rc, torch::Tensor res) {
    TORCH_CHECK(rc == HD_OK, "BeerLambert: ", hd_last_error(context(x.dev.index())));
    return x.in_dev.is_cuda() ? res : res.to(x.in_dev);
  }

  torch::Tensor band_weights(const char* who, const Batch& x, torch::Tensor weights) {
    auto w = weights.to(x.f64).reshape({-1}).contiguous();
    TORCH_CHECK(w.size(0) == x.nwave, who, ": ", w.size(0), " weights for ", x.nwave, " waves");
    return w;
  }

  torch::Tensor solve_rays(const char* who, torch::Tensor prop,
                           std::map<std::string, torch::Tensor>* bc, torch::Tensor temf,
                           torch::Tensor umu, torch::Tensor weights) {
    TORCH_CHECK(prop.dim() == 4, who, ": prop must be (nwave, ncol, nlyr, nprop)");
    TORCH_CHECK(umu.defined() && umu.scalar_type() == torch::kFloat64, who,
                ": umu must be a float64 tensor");
    TORCH_CHECK((umu.dim() == 1 || (umu.dim() == 2 && umu.size(0) == prop.size(1))) &&
                    umu.size(-1) >= 1,
                who, ": umu must be (nray) or (ncol, nray)");
    Batch x = prepare(who, prop, bc, temf, /*rays=*/true);
    const bool band = weights.defined();
    const int nray = (int)umu.size(-1);
    auto mu = umu.to(x.f64).contiguous();
    torch::Tensor w, res;
    if (band) w = band_weights(who, x, weights);
    res = band ? torch::empty({x.ncol, nray}, x.f64) : torch::empty({x.nwave, x.ncol, nray}, x.f64);
    struct hd_beer_rays rays{nray, umu.dim() == 2 ? 1 : 0, mu.data_ptr<double>(), options.alpha(),
                             band ? w.data_ptr<double>() : nullptr,
                             band ? res.data_ptr<double>() : nullptr};
    const int rc = hd_beer_rays(context(x.dev.index()), &x.cfg, &x.in, &rays,
                                band ? nullptr : res.data_ptr<double>(), nullptr, x.stream());
    return finish(x, rc, res);
  }

  Batch prepare(const char* who, torch::Tensor prop, std::map<std::string, torch::Tensor>* bc,
                torch::Tensor temf, bool rays) {
    TORCH_CHECK(prop.dim() == 4, who, ": prop must be (nwave, ncol, nlyr, nprop)");
    Batch x;
    x.nwave = prop.size(0);
    x.ncol = prop.size(1);
    x.nlyr = prop.size(2);
    x.nprop = prop.size(3);
    const int nwave = x.nwave, ncol = x.ncol, nlyr = x.nlyr;
    TORCH_CHECK(nlyr == options.nlyr(), who, ": prop has ", nlyr, " layers, options.nlyr() = ",
                options.nlyr());
    TORCH_CHECK(x.nprop >= 1, who, ": prop needs at least the optical thickness");
    TORCH_CHECK(rays || options.alpha() == 0.0, who, ": alpha = ", options.alpha(),
                " applies to ray radiances only; the flux calls need alpha = 0");
    const bool planck = options.planck();
    TORCH_CHECK(!planck || temf.defined(), who, ": planck set but temf not given");
    TORCH_CHECK(!planck || ((int)options.wave_lower().size() == nwave &&
                            (int)options.wave_upper().size() == nwave),
                who, ": planck: prop has ", nwave, " waves but wave_lower/wave_upper hold ",
                options.wave_lower().size(), "/", options.wave_upper().size());
    x.in_dev = prop.device();
    x.dev = x.in_dev.is_cuda() ? x.in_dev : torch::Device(torch::kCUDA, options.device());
    x.f64 = torch::TensorOptions().dtype(torch::kFloat64).device(x.dev);
    auto to_dev = [&](torch::Tensor t) { return t.to(x.f64).contiguous(); };
    x.p = to_dev(prop);
    static const char* keys[] = {"fbeam", "umu0", "albedo", "btemp", "ttemp", "temis", "fisot"};
    if (bc) {
      for (auto const& [k, v] : *bc) {
        bool ok = k == "phi0";  // the beam's azimuth: no meaning without scattering
        for (auto key : keys) ok = ok || k == key;
        TORCH_CHECK(ok, who, ": unknown boundary condition '", k, "'");
        x.b[k] = to_dev(v.expand({nwave, ncol}));
      }
    }
    if (planck) {
      x.tf = to_dev(temf);
      TORCH_CHECK(x.tf.dim() == 2 && x.tf.size(0) == ncol && x.tf.size(1) == nlyr + 1, who,
                  ": temf must be (ncol, nlyr+1)");
      x.wl = torch::tensor(options.wave_lower(), x.f64);
      x.wu = torch::tensor(options.wave_upper(), x.f64);
    }
    auto ptr = [](const torch::Tensor& t) -> const double* {
      return t.defined() ? t.data_ptr<double>() : nullptr;
    };
    x.cfg = hd_config{options.nstr(), 0, nlyr, x.nprop,
                      HD_FLAG_LAMBER | HD_FLAG_ONLYFL | (planck ? HD_FLAG_PLANCK : 0u)};
    x.in = hd_inputs{nwave,         ncol,           ptr(x.p),      x.bp("fbeam"),
                     x.bp("umu0"),  x.bp("albedo"), x.bp("btemp"), x.bp("ttemp"),
                     x.bp("temis"), x.bp("fisot"),  ptr(x.tf),     ptr(x.wl),
                     ptr(x.wu)};
    return x;
  }

  // one hd_context per (device, host thread), as harp_amd::Disort keeps its own
  static hd_context* context(int device) {
    thread_local std::map<int, std::unique_ptr<hd_context, int (*)(hd_context*)>> ctxs;
    auto it = ctxs.find(device);
    if (it != ctxs.end()) return it->second.get();
    hd_context* c = nullptr;
    int rc = hd_context_create(&c, device);
    TORCH_CHECK(rc == HD_OK, "BeerLambert: ", hd_last_error(nullptr));
    ctxs.emplace(device, std::unique_ptr<hd_context, int (*)(hd_context*)>(c, hd_context_destroy));
    return c;
  }
};
TORCH_MODULE(BeerLambert);

#undef HARP_AMD_BEER_ARG

}  // namespace harp_amd
