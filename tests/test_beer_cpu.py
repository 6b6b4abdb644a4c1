"""The Beer-Lambert solver without a GPU: its numpy restatement (tests/beer_ref.py)
against the project's DISORT oracles at ssa = 0 -- where the discrete-ordinate equations
decouple and the two must agree -- the alpha identity against quadrature, and the
module's host-side argument checks, which fire before a device or the library is touched.

Bounds: two different algorithms in FP64.  The restatement agrees with
oracle.disort_np.disort_forward to 1.2e-10 (nstr 2, the rel_err metric of
tests/helpers.py; the oracle's banded solve carries the error) and with
oracle.disort_rad_np.disort_rad_forward to 1.4e-12 (plain relative): the asserted
bounds are 1e-9 and 1e-10.
"""

import math

import numpy as np
import pytest
import torch

import beer_ref
from helpers import rel_err
from oracle.disort_np import disort_forward, layer2level
from oracle.disort_rad_np import disort_rad_forward


def _case(seed, nstr, nwave=3, ncol=2, nlyr=6, nprop=None):
    rng = np.random.default_rng(seed)
    nprop = 2 + nstr if nprop is None else nprop
    prop = np.zeros((nwave, ncol, nlyr, nprop))
    prop[..., 0] = 10.0 ** rng.uniform(-5, 1, (nwave, ncol, nlyr))
    bc = {"fbeam": rng.uniform(0.5, 2, (nwave, ncol)), "umu0": rng.uniform(0.1, 1, (nwave, ncol)),
          "albedo": rng.uniform(0, 1, (nwave, ncol)), "fisot": rng.uniform(0, 0.1, (nwave, ncol)),
          "btemp": rng.uniform(250, 300, (nwave, ncol)),
          "ttemp": rng.uniform(100, 200, (nwave, ncol)),
          "temis": rng.uniform(0.1, 0.9, (nwave, ncol))}
    bc["albedo"][0, 0], bc["albedo"][-1, -1] = 0.0, 1.0
    kw = {"temf": layer2level(np.linspace(290, 180, nlyr)[None, :] + rng.uniform(-5, 5, (ncol, nlyr))),
          "wave_lower": np.sort(rng.uniform(100, 1500, nwave))}
    kw["wave_upper"] = kw["wave_lower"] + rng.uniform(10, 300, nwave)
    return prop, bc, kw


@pytest.mark.parametrize("nstr", [2, 4, 8, 16])
def test_flux_restatement_vs_disort_oracle(nstr):
    prop, bc, kw = _case(100 + nstr, nstr)
    got = beer_ref.beer_flux(prop, bc, kw["temf"], nstr=nstr, planck=True,
                             wave_lower=kw["wave_lower"], wave_upper=kw["wave_upper"])
    ref = disort_forward(prop, bc, kw["temf"], nstr=nstr, planck=True,
                         wave_lower=kw["wave_lower"], wave_upper=kw["wave_upper"])
    err = rel_err(got, ref).max()
    print("beer_ref flux vs disort_np", nstr, err)
    assert err < 1e-9, err


@pytest.mark.parametrize("corint", [False, True])
@pytest.mark.parametrize("nstr", [4, 8, 16])
def test_ray_restatement_vs_radiance_oracle(nstr, corint):
    prop, bc, kw = _case(200 + nstr, nstr)
    umu = np.array([-1.0, -0.3, 0.05, 0.37, 1.0])
    got = beer_ref.beer_rays(prop, bc, kw["temf"], nstr=nstr, umu=umu, planck=True,
                             wave_lower=kw["wave_lower"], wave_upper=kw["wave_upper"])
    _, uu = disort_rad_forward(prop, bc, kw["temf"], nstr=nstr, umu=umu, phi=[0.0], planck=True,
                               wave_lower=kw["wave_lower"], wave_upper=kw["wave_upper"],
                               corint=corint)
    # levels top -> bottom: upward rays emerge at the top, downward ones at the surface
    ref = np.where(umu > 0, uu[:, :, 0, 0, :], uu[:, :, 0, -1, :])
    err = (np.abs(got - ref) / np.abs(ref)).max()
    print("beer_ref rays vs disort_rad_np", nstr, corint, err)
    assert err < 1e-10, err


@pytest.mark.parametrize("alpha,x", [(0.5, 0.3), (1.3, 5.0), (0.25, 1e-3), (2.0, 40.0)])
def test_alpha_identity(alpha, x):
    """alpha Gamma(alpha, x) x^-alpha = int_x^inf (t/x)^alpha e^-t dt - e^-x"""
    from scipy.integrate import quad
    val, _ = quad(lambda t: (t / x) ** alpha * math.exp(-t), x, np.inf, epsabs=0, epsrel=1e-13)
    ref = val - math.exp(-x)
    got = float(beer_ref.alpha_term(alpha, x))
    assert abs(got - ref) <= 1e-11 * abs(ref), (got, ref)


def test_coef_limits():
    t, w1, cin = beer_ref.coef(np.array([0.0, 1e-12, 1e-3, 0.5, 800.0]))
    assert t[0] == 1.0 and w1[0] == 0.0 and cin[0] == 0.0
    assert np.all(w1 >= 0) and np.all(cin >= 0) and np.all(t >= 0)
    np.testing.assert_allclose(w1[1:3], [5e-13, 1e-3 / 2 - 1e-6 / 6 + 1e-9 / 24 - 1e-12 / 120],
                               rtol=1e-12)
    np.testing.assert_allclose(t + w1 + cin, 1.0, rtol=0, atol=2e-16)


# --- the module's host-side checks ---------------------------------------------------
def _module(**kw):
    from pyharp_amd import BeerLambert, BeerLambertOptions
    op = BeerLambertOptions().nstr(4).nwave(2).ncol(3).nlyr(3)
    for k, v in kw.items():
        getattr(op, k)(v)
    return BeerLambert(op)


def test_options_arg_idiom_and_defaults():
    from pyharp_amd import BeerLambertOptions
    op = BeerLambertOptions()
    assert op.nstr() == 8 and op.alpha() == 0.0 and op.planck() is False
    assert op.alpha(1.3).nstr(16) is op and op.alpha() == 1.3 and op.nstr() == 16


def test_option_errors():
    for bad in (dict(nstr=3), dict(nstr=34), dict(nstr=0), dict(nlyr=0), dict(alpha=-1.0),
                dict(alpha=float("nan")), dict(planck=True)):  # planck without wave bounds
        with pytest.raises(RuntimeError, match="BeerLambert"):
            _module(**bad)


def test_forward_errors_before_any_device(monkeypatch):
    """every check below fires although no device may be asked for"""
    def boom(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    f64 = torch.float64
    b = _module()
    prop = torch.zeros((2, 3, 3, 1), dtype=f64)
    mu = torch.tensor([0.5, -0.5], dtype=f64)
    with pytest.raises(RuntimeError, match="prop must be"):
        b.forward(prop[0])
    with pytest.raises(RuntimeError, match="layers"):
        b.forward(torch.zeros((2, 3, 4, 1), dtype=f64))
    with pytest.raises(RuntimeError, match="unknown boundary condition"):
        b.forward(prop, {"nope": mu})
    with pytest.raises(RuntimeError, match=r"bc\['albedo'\]"):
        b.forward(prop, {"albedo": torch.zeros((2, 2), dtype=f64)})
    with pytest.raises(RuntimeError, match="weights for 2 waves"):
        b.forward_band(prop, weights=torch.ones(3, dtype=f64))
    with pytest.raises(RuntimeError, match="float64"):
        b.forward_rays(prop, umu=mu.float())
    with pytest.raises(RuntimeError, match="float64"):
        b.forward_rays(prop, umu=[0.5])
    with pytest.raises(RuntimeError, match="umu must be"):
        b.forward_rays(prop, umu=mu.expand(2, 2).contiguous())  # (ncol, nray) with ncol 3
    with pytest.raises(RuntimeError, match="umu must be"):
        b.forward_rays(prop, umu=mu[:0])
    with pytest.raises(RuntimeError, match="weights for 2 waves"):
        b.forward_rays_band(prop, umu=mu, weights=torch.ones(5, dtype=f64))
    pl = _module(planck=True, wave_lower=[100.0, 200.0], wave_upper=[200.0, 300.0])
    with pytest.raises(RuntimeError, match="temf not given"):
        pl.forward(prop)
    with pytest.raises(RuntimeError, match="temf must be"):
        pl.forward(prop, None, torch.zeros((3, 3), dtype=f64))
    with pytest.raises(RuntimeError, match="hold 2/2"):
        pl.forward(torch.zeros((4, 3, 3, 1), dtype=f64), None, torch.zeros((3, 4), dtype=f64))
    al = _module(alpha=1.3)
    with pytest.raises(RuntimeError, match="alpha"):
        al.forward(prop)
    with pytest.raises(RuntimeError, match="alpha"):
        al.forward_band(prop, weights=torch.ones(2, dtype=f64))


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_no_device_raises():
    with pytest.raises(RuntimeError, match="no HIP device"):
        _module().forward(torch.zeros((2, 3, 3, 1), dtype=torch.float64))
