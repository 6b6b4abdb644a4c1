"""The pseudo-spherical ray-radiance reference (tests/rays_spher_ref.py) against its two
exact limits, the flux reference, the discrete-ordinate field and an integration that does
not use the eigen-solution; and the argument checks of ``forward_rays(zd=)`` that run
before any device is touched (DESIGN.md sections 3b and 3e).  No GPU needed."""

import numpy as np
import pytest

import rays_spher_ref as RS
import spher_ref as S
from oracle.disort_np import double_gauss
from oracle.disort_rad_np import disort_rad_column

R_MARS = S.RADIUS
ZD = S.ZD
LIMIT_TOL = 1e-9   # test_spher_ref.py's bound for the same two limits of the flux reference
ODE_TOL = 1e-8     # test_spher_ref.py's bound for the flux reference against its propagator


def _hg(nlyr, nmom, g):
    pm = np.ones((nlyr, nmom + 1))
    for l in range(1, nmom + 1):
        pm[:, l] = np.asarray(g) ** l
    return pm


def _column(nstr, seed, planck=False):
    rng = np.random.default_rng(seed)
    nlyr = 5
    dtau = 10.0 ** rng.uniform(-2, 0.3, nlyr)
    ssa = rng.uniform(0.2, 0.98, nlyr)
    pm = _hg(nlyr, nstr, rng.uniform(0.2, 0.8, nlyr))  # nmom = nstr: delta-M active
    kw = dict(fbeam=1.3, albedo=0.3, phi0=rng.uniform(0, 360), fisot=0.01)
    if planck:
        kw.update(planck=True, temper=np.sort(rng.uniform(200, 300, nlyr + 1)), btemp=305.0,
                  ttemp=150.0, temis=0.5, wvnmlo=300.0, wvnmhi=800.0)
    tot = dtau.sum()
    utau = np.array([0.0, 0.37 * tot, dtau[0] + 0.5 * dtau[1], tot])
    return dtau, ssa, pm, kw, utau


def _rays(nstr, rng):
    mu_q, _ = double_gauss(nstr // 2)
    umu = np.array([0.6, -0.45, 0.02, -0.02, 1.0, -1.0, mu_q[0], -mu_q[-1]])
    return umu, rng.uniform(0.0, 360.0, umu.size)


def _plain_rays(dtau, ssa, pm, nstr, umu, phi, utau, corint, **kw):
    """disort_rad_column per ray: the diagonal of the umu x phi grid"""
    r = disort_rad_column(dtau, ssa, pm, nstr, umu=umu, phi=phi, utau=utau, corint=corint, **kw)
    i = np.arange(umu.size)
    return r["uu"][i, :, i].T, r


# ---------------------------------------------------------------- 1. the two exact limits
@pytest.mark.parametrize("nstr", [4, 8])
@pytest.mark.parametrize("corint", [False, True])
@pytest.mark.parametrize("planck", [False, True])
def test_large_radius_is_disort_rad_np(nstr, corint, planck):
    dtau, ssa, pm, kw, utau = _column(nstr, 40 + nstr + planck, planck)
    umu, phi = _rays(nstr, np.random.default_rng(nstr))
    umu0 = 0.23
    ref, full = _plain_rays(dtau, ssa, pm, nstr, umu, phi, utau, corint, umu0=umu0, **kw)
    r = RS.rays_spher_column(dtau, ssa, pm, nstr, zd=ZD, radius=1e12 * ZD[-1], umu=umu, phi=phi,
                             utau=utau, umu0=umu0, corint=corint, **kw)
    err = np.abs(r["rad"] - ref).max() / np.abs(ref).max()
    ferr = max(np.abs(r["flup"] - full["flup"]).max(), np.abs(r["fdn"] - full["fdn"]).max()) / \
        np.abs(full["fdn"]).max()
    print("R -> inf", nstr, corint, planck, err, ferr)
    assert err < LIMIT_TOL and ferr < LIMIT_TOL
    if corint:
        assert np.abs(r["mubar"] / umu0 - 1.0).max() < 1e-9


@pytest.mark.parametrize("nstr", [4, 8])
@pytest.mark.parametrize("corint", [False, True])
def test_overhead_sun_is_disort_rad_np(nstr, corint):
    dtau, ssa, pm, kw, utau = _column(nstr, 60 + nstr)
    umu, phi = _rays(nstr, np.random.default_rng(nstr + 1))
    ref, _ = _plain_rays(dtau, ssa, pm, nstr, umu, phi, utau, corint, umu0=1.0, **kw)
    r = RS.rays_spher_column(dtau, ssa, pm, nstr, zd=ZD, radius=R_MARS, umu=umu, phi=phi,
                             utau=utau, umu0=1.0, corint=corint, **kw)
    err = np.abs(r["rad"] - ref).max() / np.abs(ref).max()
    print("mu0 = 1", nstr, corint, err)
    assert err < LIMIT_TOL


# ---------------------------------------------------------------- 2. the flux reference
@pytest.mark.parametrize("profile", list(S.TAU_PROFILES))
@pytest.mark.parametrize("umu0", [0.5, 0.1, 0.02])
def test_level_fluxes_are_spher_column(profile, umu0):
    nstr, nlyr = 8, 5
    rng = np.random.default_rng(7)
    dtau = np.asarray(S.TAU_PROFILES[profile])[::-1].copy()
    dtau[2] = 0.0  # a layer of zero depth: the level below it has its own ch'
    ssa = rng.uniform(0.3, 0.95, nlyr)
    pm = _hg(nlyr, nstr, rng.uniform(0.3, 0.8, nlyr))
    kw = dict(umu0=umu0, fbeam=1.4, albedo=0.3, planck=True, temper=np.linspace(200, 300, nlyr + 1),
              btemp=305.0, ttemp=150.0, temis=0.5, wvnmlo=300.0, wvnmhi=800.0)
    ref = S.spher_column(dtau, ssa, pm, nstr, zd=ZD, radius=R_MARS, **kw)
    r = RS.rays_spher_column(dtau, ssa, pm, nstr, zd=ZD, radius=R_MARS, umu=[0.5], phi=[0.0],
                             **kw)
    scale = max(np.abs(ref["flup"]).max(), np.abs(ref["fdn"]).max())
    err = max(np.abs(r["flup"] - ref["flup"]).max(), np.abs(r["fdn"] - ref["fdn"]).max()) / scale
    print("level fluxes", profile, umu0, err)
    assert err < LIMIT_TOL


# ---------------------------------------------------------------- 3. quadrature nodes
@pytest.mark.parametrize("nstr", [4, 8])
def test_ray_at_a_node_is_the_discrete_ordinate_intensity(nstr):
    """A ray at +-mu_i equals the level's discrete-ordinate intensity, summed over the
    modes at the ray's phi (the source-function integration reproduces the solution it
    integrates)."""
    nn = nstr // 2
    dtau, ssa, pm, kw, _ = _column(nstr, 80 + nstr)
    mu_q, _ = double_gauss(nn)
    umu = np.concatenate([mu_q, -mu_q])
    phi = np.random.default_rng(3).uniform(0, 360, nstr)
    r = RS.rays_spher_column(dtau, ssa, pm, nstr, zd=ZD, radius=R_MARS, umu=umu, phi=phi,
                             umu0=0.1, **kw)
    nlyr = dtau.size
    exp = np.zeros((nlyr + 1, nstr))
    for m, sol in enumerate(r["sol"]):
        for lv in range(nlyr + 1):
            lc = min(lv, nlyr - 1)
            exp[lv] += sol["quad_field"](lc, r["taucpr"][lv]) * \
                np.cos(m * np.radians(phi - kw["phi0"]))
    err = np.abs(r["rad"] - exp).max() / np.abs(exp).max()
    print("nodes", nstr, err)
    assert err < 1e-10


# ---------------------------------------------------------------- 4. no eigen-solution
_ODE_CASES = {
    "uniform": S.TAU_PROFILES["uniform"],
    "thin_bottom": S.TAU_PROFILES["thin_bottom"],
}


@pytest.mark.parametrize("nstr", [4, 8])
@pytest.mark.parametrize("name", list(_ODE_CASES))
def test_matches_integration_of_the_true_source(name, nstr):
    """Rays of rays_spher_column against the eigen-free integration (ode_rays_column) at
    the top, the bottom and inside a layer, |mu| = 0.02 and mu = +-1 among the rays, mu0 =
    0.1 on a Mars-sized body; thin_bottom has two negative secants.  The quadrature order
    is such that doubling it moves the result by less than 1e-10 of its scale."""
    umu0, f0, albedo, phi0 = 0.1, 1.0, 0.3, 33.0
    dtau = np.asarray(_ODE_CASES[name])[::-1].copy()
    nlyr = dtau.size
    rng = np.random.default_rng(5)
    ssa = rng.uniform(0.3, 0.95, nlyr)
    pm = _hg(nlyr, nstr, rng.uniform(0.3, 0.8, nlyr))
    umu = np.array([0.02, -0.02, 1.0, -1.0, 0.55, -0.3])
    phi = np.array([10.0, 200.0, 0.0, 0.0, 75.0, 310.0])
    nsub, order = 4, 24
    tauc = np.concatenate([[0.0], np.cumsum(dtau)])
    pick = [0, 2 * nsub + nsub // 2, nlyr * nsub]  # top, the middle of layer 2, bottom
    utau = np.array([0.0, tauc[2] + 0.5 * dtau[2], tauc[-1]])
    r = RS.rays_spher_column(dtau, ssa, pm, nstr, zd=ZD, radius=R_MARS, umu=umu, phi=phi,
                             utau=utau, umu0=umu0, phi0=phi0, fbeam=f0, albedo=albedo)
    if name == "thin_bottom":
        assert r["lam"][-1] < 0.0 and r["lam"][-2] < 0.0
    kw = dict(zd=ZD, radius=R_MARS, umu=umu, phi=phi, umu0=umu0, phi0=phi0, fbeam=f0,
              albedo=albedo, nsub=nsub)
    ode, tsub = RS.ode_rays_column(dtau, ssa, pm, nstr, order=order, **kw)
    ode2, _ = RS.ode_rays_column(dtau, ssa, pm, nstr, order=2 * order, **kw)
    assert np.abs(tsub[pick] - r["utaupr"]).max() <= 1e-14
    scale = np.abs(ode[pick]).max()
    conv = np.abs(ode2[pick] - ode[pick]).max() / scale
    err = np.abs(r["rad"] - ode[pick]).max() / scale
    print(name, nstr, "order doubling moves", conv, " reference vs ODE", err)
    assert conv < 1e-10
    assert err < ODE_TOL


# ---------------------------------------------------------------- 5. argument checks
def _module(nstr=8, radius=None, flags="lamber,quiet"):
    from pyharp_amd import Disort, DisortOptions
    op = DisortOptions().flags(flags).nwave(1).ncol(2)
    op.ds().nlyr, op.ds().nstr, op.ds().nmom = 4, nstr, nstr
    if radius is not None:
        op.radius(radius)
    return Disort(op)


def test_forward_rays_zd_argument_errors():
    import torch
    f64 = torch.float64
    no_gpu = not torch.cuda.is_available()  # with one, a good call goes on to the device
    prop = torch.zeros((1, 2, 4, 10), dtype=f64)
    umu = torch.tensor([0.5, -0.5], dtype=f64)
    phi = torch.zeros(2, dtype=f64)
    zd = torch.arange(5, dtype=f64)
    w = torch.ones(1, dtype=f64)
    calls = (lambda m, **k: m.forward_rays(prop, {}, umu=umu, phi=phi, **k),
             lambda m, **k: m.forward_rays_band(prop, {}, umu=umu, phi=phi, weights=w, **k))
    for call in calls:
        # no radius (0 by default), and bad ones
        with pytest.raises(RuntimeError, match="needs DisortOptions.radius"):
            call(_module(), zd=zd)
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(RuntimeError, match="needs DisortOptions.radius"):
                call(_module(radius=bad), zd=zd)
        m = _module(radius=R_MARS)
        # shape and dtype
        for z in (torch.arange(4, dtype=f64), torch.zeros((3, 5), dtype=f64),
                  torch.zeros((1, 2, 5), dtype=f64)):
            with pytest.raises(RuntimeError, match=r"zd must be \(nlyr\+1,\) or \(ncol, nlyr\+1\)"):
                call(m, zd=z)
        with pytest.raises(RuntimeError, match="zd must be a float64 tensor"):
            call(m, zd=zd.to(torch.float32))
        with pytest.raises(RuntimeError, match="zd must be a float64 tensor"):
            call(m, zd=[0.0, 1.0, 2.0, 3.0, 4.0])
        # nstr 18
        with pytest.raises(RuntimeError, match="nstr <= 16"):
            call(_module(nstr=18, radius=R_MARS), zd=zd)
        # a good zd passes these checks and stops where the plain call does: at the device
        if no_gpu:
            with pytest.raises(RuntimeError, match="no HIP device"):
                call(m, zd=zd)
            with pytest.raises(RuntimeError, match="no HIP device"):
                call(m, zd=torch.zeros((2, 5), dtype=f64))
            # zd=None: the plain route's checks, radius or not, nstr 18 included
            with pytest.raises(RuntimeError, match="no HIP device"):
                call(_module(nstr=18), zd=None)
        with pytest.raises(RuntimeError, match="phi .* must have umu's shape"):
            m.forward_rays(prop, {}, umu=umu, phi=torch.zeros(3, dtype=f64), zd=None)
    # the spher flag keeps its meaning: not on a module with radiances
    with pytest.raises(RuntimeError, match="pseudo-spherical radiances are not implemented"):
        _module(radius=R_MARS, flags="lamber,quiet,spher")
