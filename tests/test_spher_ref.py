"""The pseudo-spherical CPU reference (tests/spher_ref.py) against identities, limits,
closed forms and an integration that does not use the eigen-solution; and the binding's
flag semantics for ``spher`` (DESIGN.md sections 1 and 3e).  No GPU needed."""

import math

import numpy as np
import pytest

import spher_ref as S
from oracle.disort_np import disort_column, double_gauss

R_MARS, R_EARTH = 3.39e6, 6.4e6
ZD = S.ZD


def _hg(nlyr, nstr, g):
    pm = np.ones((nlyr, nstr + 1))
    for l in range(1, nstr + 1):
        pm[:, l] = np.asarray(g) ** l
    return pm


# ---------------------------------------------------------------- 1. Chapman identities
@pytest.mark.parametrize("radius", [R_MARS, R_EARTH])
def test_overhead_sun_gives_the_vertical_depth(radius):
    dtau = np.array([0.3, 1e-3, 0.7, 0.05, 1.2])
    ch = S.chapman(ZD, radius, 1.0, dtau)
    cum = np.concatenate([np.cumsum(dtau[::-1])[::-1], [0.0]])
    assert np.abs(ch - cum).max() <= 1e-14 * max(1.0, cum.max())
    assert ch[-1] == 0.0


@pytest.mark.parametrize("umu0", [1.0, 0.5, 0.1, 0.02])
def test_splitting_layers_keeps_the_slant_depth(umu0):
    """Every layer cut in two at equal extinction per unit height: ch at the original
    levels is unchanged (the shells' extinction is uniform in altitude)."""
    dtau = np.array([0.3, 1e-3, 0.7, 0.05, 1.2])
    zmid = 0.5 * (ZD[:-1] + ZD[1:]) + 0.17 * (ZD[1:] - ZD[:-1])  # not the midpoints
    z2 = np.sort(np.concatenate([ZD, zmid]))
    frac = (zmid - ZD[:-1]) / (ZD[1:] - ZD[:-1])
    dt2 = np.stack([dtau * frac, dtau * (1.0 - frac)], axis=1).ravel()
    ch = S.chapman(ZD, R_MARS, umu0, dtau)
    ch2 = S.chapman(z2, R_MARS, umu0, dt2)[::2]
    assert np.abs(ch2 - ch).max() <= 1e-13 * max(1.0, ch.max())


def test_large_radius_is_plane_parallel():
    dtau = np.array([0.3, 1e-3, 0.7, 0.05, 1.2])
    umu0 = 0.2
    ch = S.chapman(ZD, 1e12 * ZD[-1], umu0, dtau)
    cum = np.concatenate([np.cumsum(dtau[::-1])[::-1], [0.0]]) / umu0
    rel = np.abs(ch[:-1] - cum[:-1]) / cum[:-1]
    print("R = 1e12 z_top: max rel dev of ch from tau/mu0", rel.max())
    assert rel.max() < 1e-10
    g = S.geometric_factors(ZD, 1e12 * ZD[-1], umu0)
    assert np.abs(g[np.triu_indices(5)[0], np.triu_indices(5)[1]] * umu0 - 1.0).max() < 1e-10


# ---------------------------------------------------------------- 2. plane-parallel limit
@pytest.mark.parametrize("nstr", [4, 8, 16])
@pytest.mark.parametrize("planck", [False, True])
@pytest.mark.parametrize("albedo", [0.0, 0.3])
def test_plane_parallel_limit_matches_disort_np(nstr, planck, albedo):
    rng = np.random.default_rng(nstr + 10 * planck)
    nlyr = 5
    dtau = 10.0 ** rng.uniform(-2, 0.3, nlyr)
    ssa = rng.uniform(0.2, 0.98, nlyr)
    pm = _hg(nlyr, nstr, rng.uniform(0.2, 0.8, nlyr))
    kw = dict(umu0=rng.uniform(0.2, 1.0), fbeam=1.3, albedo=albedo)
    if planck:
        kw.update(planck=True, temper=np.sort(rng.uniform(200, 300, nlyr + 1)), btemp=305.0,
                  ttemp=150.0, temis=0.5, wvnmlo=300.0, wvnmhi=800.0)
    ref = disort_column(dtau, ssa, pm, nstr, **kw)
    r = S.spher_column(dtau, ssa, pm, nstr, zd=ZD, radius=1e12 * ZD[-1], **kw)
    scale = max(np.abs(ref["flup"]).max(), np.abs(ref["fdn"]).max())
    for k in ("flup", "fdn", "rfldir"):
        err = np.abs(r[k] - ref[k]).max() / scale
        assert err < 1e-9, (k, err)


# ---------------------------------------------------------------- 3. closed forms, omega = 0
@pytest.mark.parametrize("umu0", [1.0, 0.5, 0.1, 0.02])
@pytest.mark.parametrize("albedo", [0.0, 0.3])
def test_closed_forms_without_scattering(umu0, albedo):
    nstr, nlyr = 8, 5
    dtau = np.array([0.5, 0.5, 0.5, 1e-3, 1e-3])[::-1].copy()  # top -> bottom
    f0 = 1.7
    r = S.spher_column(dtau, np.zeros(nlyr), _hg(nlyr, nstr, 0.0), nstr, zd=ZD, radius=R_MARS,
                       umu0=umu0, fbeam=f0, albedo=albedo)
    ch = S.chapman(ZD, R_MARS, umu0, dtau[::-1])[::-1]  # top -> bottom
    assert np.abs(r["rfldir"] - umu0 * f0 * np.exp(-ch)).max() <= 1e-12 * umu0 * f0
    mu, w = double_gauss(nstr // 2)
    tau = np.concatenate([[0.0], np.cumsum(dtau)])
    up = 2.0 * albedo * umu0 * f0 * math.exp(-ch[-1]) * \
        (w * mu * np.exp(-(tau[-1] - tau)[:, None] / mu)).sum(axis=1)
    assert np.abs(r["flup"] - up).max() <= 1e-12 * umu0 * f0
    assert np.abs(r["rfldn"]).max() <= 1e-12 * umu0 * f0


# ---------------------------------------------------------------- 4. no eigen-solution
_ODE_CASES = {
    "three_layers": (ZD[[0, 1, 3, 5]], (0.4, 0.6, 0.5)),
    "thin_bottom": (ZD, S.TAU_PROFILES["thin_bottom"]),
}


@pytest.mark.parametrize("name", list(_ODE_CASES))
def test_matches_integration_of_the_true_source(name):
    """Level fluxes of spher_column against the matrix-exponential propagation of the
    2N-stream equation with the source x0(mu0) F0 e^{-ch'(tau)} (spher_ref.
    propagator_column): exact to rounding (it stands in for an integrator asked for
    1e-10), asserted at 1e-8 of the incident flux.  mu0 = 0.1 on a Mars-sized body."""
    zd, dt_bt = _ODE_CASES[name]
    nstr, umu0, f0, albedo = 4, 0.1, 1.0, 0.3
    dtau = np.asarray(dt_bt)[::-1].copy()
    nlyr = dtau.size
    rng = np.random.default_rng(5)
    ssa = rng.uniform(0.3, 0.95, nlyr)
    pm = _hg(nlyr, nstr, rng.uniform(0.3, 0.8, nlyr))
    r = S.spher_column(dtau, ssa, pm, nstr, zd=zd, radius=R_MARS, umu0=umu0, fbeam=f0,
                       albedo=albedo)
    flup, fdn, chp, lam = S.propagator_column(dtau, ssa, pm, nstr, zd=zd, radius=R_MARS,
                                              umu0=umu0, fbeam=f0, albedo=albedo)
    if name == "thin_bottom":
        print("secants top -> bottom:", lam)
        assert lam[-1] < 0.0 and lam[-2] < 0.0  # the beam grows downward through them
        assert (lam[:3] > 1.0).all()
    err = max(np.abs(r["flup"] - flup).max(), np.abs(r["fdn"] - fdn).max()) / (umu0 * f0)
    print(name, "max |dF| / (mu0 F0) =", err)
    assert err < 1e-8


def test_issue_secants():
    """The secants quoted in DESIGN.md section 3e (unscaled depths, mu0 = 0.1)."""
    _, lam = S.layer_secants(ZD, R_MARS, 0.1, np.array([0.5, 0.5, 0.5, 1e-3, 1e-3]))
    assert np.allclose(lam[::-1], [-1020, -1806, 5.1, 6.1, 8.1], rtol=0.01)
    _, lam = S.layer_secants(ZD, R_MARS, 0.1, np.full(5, 0.3))
    assert np.allclose(lam[::-1], [4.0, 4.5, 5.1, 6.1, 8.1], rtol=0.02)


# ---------------------------------------------------------------- 5. flag semantics
def _options(flags, radius=None):
    from pyharp_amd import DisortOptions
    op = DisortOptions().flags(flags).nwave(1).ncol(1)
    op.ds().nlyr, op.ds().nstr, op.ds().nmom = 4, 8, 8
    if radius is not None:
        op.radius(radius)
    return op


def test_spher_flag_semantics():
    import torch
    from pyharp_amd import Disort
    with pytest.raises(RuntimeError, match="pseudo-spherical geometry needs DisortOptions.radius"):
        Disort(_options("lamber,onlyfl,spher"))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="pseudo-spherical"):
            Disort(_options("lamber,onlyfl,spher", bad))
    d = Disort(_options("lamber,onlyfl,spher", R_MARS))
    assert d.spher
    with pytest.raises(RuntimeError, match="pseudo-spherical radiances are not implemented"):
        Disort(_options("lamber,spher", R_MARS))
    op = _options("lamber,onlyfl,usrtau,spher", R_MARS)
    op.user_tau([0.0, 0.1])
    with pytest.raises(RuntimeError, match="pseudo-spherical radiances are not implemented"):
        Disort(op)
    # radius without spher: accepted and unused
    plain = Disort(_options("lamber,onlyfl", R_MARS))
    assert not plain.spher
    prop = torch.zeros((1, 1, 4, 10), dtype=torch.float64)
    zd = torch.arange(5, dtype=torch.float64)
    w = torch.ones(1, dtype=torch.float64)
    # spher without zd / zd without spher: never ignored
    for call in (lambda m, **k: m.forward(prop, {}, **k), lambda m, **k: m.forward_flx(prop, {}, **k),
                 lambda m, **k: m.forward_band(prop, {}, weights=w, **k)):
        with pytest.raises(RuntimeError, match="zd"):
            call(d)
        with pytest.raises(RuntimeError, match="zd"):
            call(plain, zd=zd)
    # CPU tensors with spher
    with pytest.raises(RuntimeError, match="device"):
        d.forward(prop, {}, zd=zd)
