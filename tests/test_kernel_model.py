"""The kernels' formulation (tests/kernel_model.py) against the oracle, on CPU.

Separates a formulation error (symmetric eigenproblem, flux-weighted layer
operators, adding sweep) from a HIP coding error.
"""

import numpy as np
import pytest

from kernel_model import solve_column
from oracle.disort_np import disort_column


@pytest.mark.parametrize("seed", range(6))
def test_model_matches_oracle(seed):
    rng = np.random.default_rng(100 + seed)
    nstr = [4, 8, 16][seed % 3]
    L = int(rng.integers(1, 15))
    tau = 10 ** rng.uniform(-5, 1.5, L)
    ssa = rng.uniform(0, 0.9999, L)
    g = rng.uniform(0, 0.9, L)
    chis = [[gg ** l for l in range(1, nstr + 1)] for gg in g]
    pmom = np.array([[1.0] + c for c in chis])
    planck = seed % 2 == 1
    kw = dict(planck=planck, temper=np.linspace(150, 300, L + 1), btemp=300.0,
              wvnmlo=100.0, wvnmhi=900.0) if planck else {}
    mu0, A = rng.uniform(0.05, 1), rng.uniform(0, 1)
    r = disort_column(tau, ssa, pmom, nstr, umu0=mu0, fbeam=1.0, albedo=A, **kw)
    fu, fd = solve_column(tau, ssa, chis, nstr, umu0=mu0, fbeam=1.0, albedo=A, **kw)
    scale = max(np.abs(r["flup"]).max(), np.abs(r["fdn"]).max())
    for a, b in ((fu, r["flup"]), (fd, r["fdn"])):
        err = np.abs(a - b) / np.maximum(np.abs(b), 1e-6 * scale)
        assert err.max() < 1e-8


def test_model_exact_conservative_without_dither():
    """The symmetric formulation needs no dither: k -> 0 is regular."""
    import kernel_model
    saved = kernel_model.DITHER
    try:
        kernel_model.DITHER = 0.0
        tau = [0.5, 3.0]
        chis = [[0.5 ** l for l in range(1, 9)]] * 2
        fu, fd = solve_column(tau, [1.0, 1.0], chis, 8, umu0=0.7, fbeam=1.0, albedo=1.0)
    finally:
        kernel_model.DITHER = saved
    assert np.all(np.isfinite(fu)) and np.abs(fd - fu).max() < 1e-12


@pytest.mark.parametrize("seed", range(4))
def test_radiance_model_matches_oracle(seed):
    """tests/kernel_model_rad.py (the radiance kernels' formulation) vs the
    radiance oracle, every azimuthal mode, user depths inside layers."""
    import kernel_model_rad as km
    from oracle.disort_np import plkavg
    from oracle.disort_rad_np import disort_rad_column
    rng = np.random.default_rng(300 + seed)
    nstr = [4, 8, 16, 6][seed]
    L = int(rng.integers(1, 7))
    tau = 10 ** rng.uniform(-3, 0.7, L)
    ssa = rng.uniform(0, 0.99, L)
    g = rng.uniform(0, 0.8, L)
    chis = [[gg ** l for l in range(1, nstr + 1)] for gg in g]
    pmom = np.array([[1.0] + c for c in chis])
    planck = seed % 2 == 1
    umu0, fbeam, alb, fisot = rng.uniform(0.1, 1), 1.7, rng.uniform(0, 1), 0.03
    kw = {}
    pk, bsurf, btop = None, 0.0, 0.0
    if planck:
        temper = np.linspace(180, 290, L + 1)
        kw = dict(planck=True, temper=temper, btemp=295.0, ttemp=160.0, temis=0.4,
                  wvnmlo=300.0, wvnmhi=1000.0)
        pk = np.array([plkavg(300.0, 1000.0, t) for t in temper])
        bsurf, btop = plkavg(300.0, 1000.0, 295.0), 0.4 * plkavg(300.0, 1000.0, 160.0)
    taus = np.concatenate([[0.0], np.cumsum(tau)])
    ut = np.sort(np.concatenate([[0.0, taus[-1]], rng.uniform(0, taus[-1], 3)]))
    umu = np.array([-0.9, -0.35, 0.2, 0.65, 1.0])
    r = disort_rad_column(tau, ssa, pmom, nstr, umu=umu, phi=[0.0], utau=ut, umu0=umu0,
                          fbeam=fbeam, albedo=alb, fisot=fisot, **kw)
    for m in range(nstr):
        ops, ip, im, cp, cm = km.solve_mode(tau, ssa, chis, nstr, m, umu0=umu0, fbeam=fbeam,
                                            albedo=alb, fisot=fisot, pk=pk, bsurf=bsurf,
                                            btop=btop)
        ref = r["uum"][m]
        scale = np.abs(r["uum"][0]).max()
        for iu, mu in enumerate(umu):
            got = km.user_radiance(ops, ip, im, cp, cm, nstr, m, mu, ut, umu0=umu0, fbeam=fbeam,
                                   albedo=alb, fisot=fisot, bsurf=bsurf, btop=btop)
            err = np.abs(got - ref[:, iu]).max() / scale
            assert err < 1e-9, (m, mu, got, ref[:, iu])


# --------------------------------------------------------------------------- #
# the hard-regime fixture (tests/hard_cases.py, mp reference): where a formulation
# defect of the kernels shows without a GPU
# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def hard_fixture():
    import hard_cases
    from helpers import GOLDEN
    return hard_cases.load(GOLDEN)


def _model_batch(b):
    """The model's (1, C, L+1, 2) fluxes of a fixture batch, harp layout."""
    import hard_cases
    nlyr, nstr = b["nlyr"], b["nstr"]
    out = np.zeros((1, b["prop"].shape[1], nlyr + 1, 2))
    for c in range(out.shape[1]):
        p = b["prop"][0, c, ::-1]
        kw = {k: float(v[0, c]) for k, v in b["bc"].items()}
        if b["planck"]:
            kw.update(planck=True, temper=b["temf"][c, ::-1], wvnmlo=hard_cases.WAVE[0],
                      wvnmhi=hard_cases.WAVE[1])
        fu, fd = solve_column(p[:, 0], p[:, 1], [list(r[2:2 + b["nmom"]]) for r in p], nstr, **kw)
        out[0, c, :, 0], out[0, c, :, 1] = fu[::-1], fd[::-1]
    return out


@pytest.mark.parametrize("nstr", [2, 4, 8, 16])
@pytest.mark.parametrize("family", ["phase", "conservative", "depth", "thin_thermal",
                                    "resonance"])
def test_model_on_hard_fixture(hard_fixture, family, nstr):
    """Every fixture column with nstr <= 16 at TOL against the mp reference."""
    from helpers import TOL, rel_err
    from oracle.disort_mp import flux_of_record
    worst = 0.0
    for b in hard_fixture[family, nstr]:
        err = rel_err(_model_batch(b), flux_of_record(b["ref"])).max(axis=(0, 2, 3))
        print(f"  {family} n{nstr} {b['name']}: worst {err.max():.3e} (column {err.argmax()})")
        worst = max(worst, err.max())
    assert worst < TOL


def test_model_shows_what_the_two_rules_replace(hard_fixture):
    """With the earlier rules (one denominator clamped at 1e-9 / mu0^2, dB / tau' formed at
    any tau' > 0) the same columns miss TOL by orders of magnitude: the fixture sees both."""
    import kernel_model
    from helpers import TOL, rel_err
    from oracle.disort_mp import flux_of_record
    saved = kernel_model.RES_CLAMP, kernel_model.THIN_TAU
    try:
        kernel_model.RES_CLAMP, kernel_model.THIN_TAU = 1.0e-9, 0.0
        res = [b for b in hard_fixture["resonance", 8] if b["name"] == "scat"][0]
        thin = [b for b in hard_fixture["thin_thermal", 8] if b["name"] == "top2"][0]
        e_res = rel_err(_model_batch(res), flux_of_record(res["ref"])).max()
        e_thin = rel_err(_model_batch(thin), flux_of_record(thin["ref"])).max()
    finally:
        kernel_model.RES_CLAMP, kernel_model.THIN_TAU = saved
    print(f"  clamp: {e_res:.3e}   dB/tau': {e_thin:.3e}")
    assert e_res > 1e3 * TOL and e_thin > 1e3 * TOL


# --------------------------------------------------------------------------- #
# the pseudo-spherical hard-regime fixture (tests/spher_hard_cases.py)
# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def spher_fixture():
    import spher_hard_cases
    from helpers import GOLDEN
    return spher_hard_cases.load(GOLDEN)


def _spher_model_batch(b):
    import spher_hard_cases
    out = np.zeros((1, b["prop"].shape[1], b["nlyr"] + 1, 2))
    for c in range(out.shape[1]):
        (tau, ssa, pm, nstr), kw = spher_hard_cases.column_kwargs(b, c)
        fu, fd = solve_column(tau, ssa, [list(r[1:]) for r in pm], nstr, **kw)
        out[0, c, :, 0], out[0, c, :, 1] = fu[::-1], fd[::-1]
    return out


@pytest.mark.parametrize("nstr", [2, 4, 8, 16])
@pytest.mark.parametrize("family", ["resonance", "low_sun", "depth", "conservative",
                                    "thin_thermal", "phase"])
def test_model_on_spher_hard_fixture(spher_fixture, family, nstr):
    """Every pseudo-spherical fixture column with nstr <= 16 at TOL against the mp
    reference."""
    from helpers import TOL, rel_err
    from oracle.disort_mp import flux_of_record
    worst = 0.0
    for b in spher_fixture[family, nstr]:
        err = rel_err(_spher_model_batch(b), flux_of_record(b["ref"])).max(axis=(0, 2, 3))
        print(f"  {family} n{nstr} {b['name']}: worst {err.max():.3e} (column {err.argmax()})")
        worst = max(worst, err.max())
    assert worst < TOL


def test_model_shows_what_the_spher_move_replaces(spher_fixture):
    """The clamp the SPHER layer kernels carried (one denominator at 1e-9 lambda^2) misses
    TOL by orders of magnitude on the layer secant's resonance; the plain path's move
    carried over without lambda's sign misses it where lambda < 0."""
    import kernel_model
    from helpers import TOL, rel_err
    from oracle.disort_mp import flux_of_record
    res = {b["name"]: b for b in spher_fixture["resonance", 8]}
    saved = kernel_model.RES_CLAMP, kernel_model.KEEP_SIGN
    try:
        kernel_model.RES_CLAMP = 1.0e-9
        e_clamp = rel_err(_spher_model_batch(res["scat"]), flux_of_record(res["scat"]["ref"])).max()
        kernel_model.RES_CLAMP, kernel_model.KEEP_SIGN = None, False
        e_sign = rel_err(_spher_model_batch(res["negative"]),
                         flux_of_record(res["negative"]["ref"])).max()
    finally:
        kernel_model.RES_CLAMP, kernel_model.KEEP_SIGN = saved
    print(f"  clamp: {e_clamp:.3e}   move without the sign: {e_sign:.3e}")
    assert e_clamp > 1e3 * TOL and e_sign > TOL
