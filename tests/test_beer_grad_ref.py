"""The reference of the Beer-Lambert gradients (tests/beer_grad_ref.py) without a GPU:
its forward against the numpy restatement it restates, its autograd gradients against
central differences of that restatement, the thin-layer series of dw1/dx against mpmath,
and the module's host-side refusals, which fire before a device is touched.

Bounds.  Forward: the same formulas in the same precision, 1e-13 relative.  Gradients of
everything but temperatures: 1e-6 of the tensor's largest component (central differences
at the steps of STEP carry about 1e-9).  Temperature gradients are DEFINED by the
Leibniz derivative of the exact band integral, while the differences see PLKAVG's own
approximation (a Simpson rule stopped at 1e-6, series truncated by a table: not smooth
in T): the worst difference measured in this test, Richardson-extrapolated differences at
2 K and 1 K, is T_MEASURED; ten times that is asserted.
"""

import math

import numpy as np
import pytest
import torch

import beer_grad_ref
import beer_ref
from test_gpu_beer import _case, _ref_kw

T_MEASURED = 7.1e-5  # worst temperature-gradient difference relative to the largest component
# relative steps of the central differences (of max(|x|, 1)): the results are linear in
# albedo, fbeam, fisot and temis, so a step of 1e-2 is exact up to rounding 1e-16 / 1e-2
STEP = {"tau": 1e-6, "umu0": 1e-5}
UMU = np.array([[-1.0, -0.3, 0.05, 0.37, 1.0], [0.9, -0.02, 0.02, -1.0, 0.5]])


@pytest.mark.parametrize("planck", [False, True])
@pytest.mark.parametrize("nstr,nlyr", [(2, 1), (8, 3), (16, 17)])
def test_forward_equals_the_restatement(nstr, nlyr, planck):
    rng = np.random.default_rng(9000 + 100 * nstr + nlyr + 7 * planck)
    prop, bc, kw = _case(rng, 5, 2, nlyr, 3, planck)
    ref = beer_ref.beer_flux(prop, bc, kw.get("temf"), nstr=nstr, **_ref_kw(kw))
    got = beer_grad_ref.beer_flux(prop, bc, kw.get("temf"), nstr=nstr, **_ref_kw(kw)).numpy()
    err = (np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)).max()
    rref = beer_ref.beer_rays(prop, bc, kw.get("temf"), nstr=nstr, umu=UMU, alpha=0.7,
                              **_ref_kw(kw))
    rgot = beer_grad_ref.beer_rays(prop, bc, kw.get("temf"), nstr=nstr, umu=UMU, alpha=0.7,
                                   **_ref_kw(kw)).numpy()
    rerr = (np.abs(rgot - rref) / np.maximum(np.abs(rref), 1e-300)).max()
    print("beer_grad_ref forward vs beer_ref", nstr, nlyr, planck, err, rerr)
    assert max(err, rerr) < 1e-13


def _fd_case():
    """2 x 2 solves, 4 layers on both sides of the series switch with an empty and a thick
    one, albedo 0 / 1 / inside (the beam stays on: at fbeam = 0 the solver's switch
    fbeam > 0 makes the differences one-sided)"""
    rng = np.random.default_rng(4242)
    prop, bc, kw = _case(rng, 2, 2, 4, 2, True)
    prop[0, 0, :, 0] = [0.3, 0.0, 50.0, 1e-3]
    bc["albedo"][0, 0], bc["albedo"][1, 1] = 0.0, 1.0
    return prop, bc, kw


def _loss_np(fn, cot, prop, bc, temf, **kw):
    return float((cot * fn(prop, bc, temf, **kw)).sum())


@pytest.mark.parametrize("call", ["flux", "rays"])
def test_gradients_against_central_differences(call):
    prop, bc, kw = _fd_case()
    nstr = 4
    opts = dict(nstr=nstr, **_ref_kw(kw))
    if call == "rays":
        opts.update(umu=UMU, alpha=0.7)
    fn_t = beer_grad_ref.beer_flux if call == "flux" else beer_grad_ref.beer_rays
    fn_n = beer_ref.beer_flux if call == "flux" else beer_ref.beer_rays
    tau = torch.tensor(prop[..., 0], requires_grad=True)
    temf = torch.tensor(kw["temf"], requires_grad=True)
    bct = {k: torch.tensor(v, requires_grad=True) for k, v in bc.items()}
    pt = torch.stack([tau, torch.as_tensor(prop[..., 1])], dim=-1)
    out = fn_t(pt, bct, temf, **opts)
    cot = np.random.default_rng(7).uniform(-1, 1, tuple(out.shape))
    (torch.as_tensor(cot) * out).sum().backward()

    def fd(name, h, richardson=False):
        """central differences of beer_ref in one input, component by component"""
        base = {"tau": prop[..., 0], "temf": kw["temf"]}.get(name, bc.get(name))
        g = np.zeros_like(base)

        def loss(x):
            p, b, tf = prop.copy(), dict(bc), kw["temf"]
            if name == "tau":
                p[..., 0] = x
            elif name == "temf":
                tf = x
            else:
                b[name] = x
            return _loss_np(fn_n, cot, p, b, tf, **opts)

        def diff(idx, step):
            xp, xm = base.copy(), base.copy()
            xp[idx] += step
            xm[idx] -= step
            return (loss(xp) - loss(xm)) / (2.0 * step)

        for idx in np.ndindex(base.shape):
            step = h * max(abs(base[idx]), 1.0) if not richardson else h
            g[idx] = diff(idx, step) if not richardson else \
                (4.0 * diff(idx, step / 2) - diff(idx, step)) / 3.0
        return g

    worst_t = 0.0
    for name, got in [("tau", tau.grad), ("temf", temf.grad)] + [(k, v.grad) for k, v in bct.items()]:
        got = got.numpy()
        temp = name in ("temf", "btemp", "ttemp")
        ref = fd(name, 2.0, richardson=True) if temp else fd(name, STEP.get(name, 1e-2))
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"beer_grad_ref {call} d/d{name}: {err:.3e} of the largest component "
              f"{np.abs(ref).max():.3e}")
        if temp:
            worst_t = max(worst_t, err)
        else:
            assert err < 1e-6, (name, err)
    print(f"worst temperature gradient difference ({call}): {worst_t:.3e}")
    assert worst_t < 10.0 * T_MEASURED


def test_thin_layer_series_against_mpmath():
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 700  # (1 - e^-x) - x e^-x cancels to x^2 / 2: 600 digits at x = 1e-300

    def exact(x):
        if x == 0.0:
            return mpmath.mpf(1) / 2
        x = mpmath.mpf(x)
        return ((1 - mpmath.exp(-x)) - x * mpmath.exp(-x)) / x ** 2

    assert beer_grad_ref.w1p_series(0.0) == 0.5
    for x in [0.0, 1e-300, 1e-8, 1e-3, 0.1249, 0.125, 1.0, 50.0]:
        ref = exact(x)
        got = float(beer_grad_ref.w1p(x))
        ulps = abs(mpmath.mpf(got) - ref) / mpmath.mpf(math.ulp(float(ref)))
        print(f"w1p({x:g}) = {got!r}: {float(ulps):.2f} ulp")
        if x < 0.125:  # the series
            assert ulps <= 4
        else:          # ((1 - w1) - t) / x: w1's rounding over a difference >= 0.057
            assert abs(got - float(ref)) <= 1e-13 * float(ref)
    # the series itself up to the switch
    got = float(beer_grad_ref.w1p_series(0.125))
    assert abs(mpmath.mpf(got) - exact(0.125)) <= 4 * math.ulp(got)


# --- host-side refusals: before a device or the library is touched ---------------------
def _solver(planck=False):
    from pyharp_amd import BeerLambert, BeerLambertOptions
    op = BeerLambertOptions().nstr(4).nlyr(3).nwave(2).ncol(2)
    if planck:
        op.planck(True).wave_lower([100.0, 200.0]).wave_upper([150.0, 260.0])
    return BeerLambert(op)


def _prop(requires_grad=True):
    return torch.full((2, 2, 3, 1), 0.1, dtype=torch.float64, requires_grad=requires_grad)


def test_out_with_an_input_that_requires_grad_is_refused():
    b = _solver()
    w = torch.ones(2, dtype=torch.float64)
    umu = torch.tensor([0.5], dtype=torch.float64)
    with pytest.raises(RuntimeError, match="out=.*requires grad"):
        b.forward(_prop(), out=torch.empty(2, 2, 4, 2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="requires grad"):
        b.forward_band(_prop(), weights=w, flux=torch.empty(2, 2, 4, 2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="requires grad"):
        b.forward_band(_prop(False), {"albedo": torch.tensor(0.3, dtype=torch.float64,
                                                             requires_grad=True)},
                       weights=w, out=torch.empty(2, 4, 2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="requires grad"):
        b.forward_rays_band(_prop(), umu=umu, weights=w,
                            rad=torch.empty(2, 2, 1, dtype=torch.float64))
    temf = torch.full((2, 4), 250.0, dtype=torch.float64, requires_grad=True)
    with pytest.raises(RuntimeError, match="requires grad"):
        _solver(True).forward(_prop(False), None, temf,
                              out=torch.empty(2, 2, 4, 2, dtype=torch.float64))


def test_umu_and_weights_requiring_grad_are_refused():
    b = _solver()
    umu = torch.tensor([0.5], dtype=torch.float64, requires_grad=True)
    with pytest.raises(RuntimeError, match="umu requires grad"):
        b.forward_rays(_prop(False), umu=umu)
    w = torch.ones(2, dtype=torch.float64, requires_grad=True)
    with pytest.raises(RuntimeError, match="weights requires grad"):
        b.forward_band(_prop(False), weights=w)
    with pytest.raises(RuntimeError, match="weights requires grad"):
        b.forward_rays_band(_prop(), umu=umu.detach(), weights=w)


def test_no_grad_and_plain_inputs_take_the_plain_path(monkeypatch):
    """nothing to differentiate: the call reaches today's device check, not a refusal"""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    b = _solver()
    out = torch.empty(2, 2, 4, 2, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no HIP device"):
        b.forward(_prop(False), out=out)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no HIP device"):
        b.forward(_prop(), out=out)
