"""oracle/disort_mp.py, the arbitrary-precision pin of the flux solve, on the CPU.

* against both double oracles on benign columns (where all three must agree to rounding),
* against the published DISOTEST-1 fluxes and the closed forms of tests/test_oracle.py,
* against itself at 50 and 90 digits on the inputs the double oracles fail on,
* against the stored fixture tests/golden/flux_hard.npz (a stale file fails).
"""

import math

import numpy as np
import pytest
from mpmath import mp

import hard_cases
from flx_ref import flx_ref_column
from helpers import GOLDEN, disotest, rel_err
from oracle import disort_mp, disort_np


@pytest.fixture(scope="module")
def fixture():
    return hard_cases.load(GOLDEN)


@pytest.mark.parametrize("nstr", [2, 4, 8, 16])
def test_matches_both_oracles_on_benign_columns(nstr, oracle_c):
    """tau in [0.05, 3], ssa <= 0.95, g = 0.7, a 20 K step per layer: the inputs every
    double solver here resolves to rounding.  1e-12 in the project's metric."""
    rng = np.random.default_rng(7100 + nstr)
    W, C, L = 1, 2, 3
    prop = np.zeros((W, C, L, 2 + nstr))
    prop[..., 0] = rng.uniform(0.05, 3.0, (W, C, L))
    prop[..., 1] = rng.uniform(0.1, 0.95, (W, C, L))
    for l in range(nstr):
        prop[..., 2 + l] = 0.7 ** (l + 1)
    bc = {"fbeam": np.full((W, C), 1.3), "umu0": rng.uniform(0.2, 1.0, (W, C)),
          "albedo": rng.uniform(0.0, 1.0, (W, C)), "btemp": np.full((W, C), 285.0),
          "ttemp": np.full((W, C), 150.0), "temis": np.full((W, C), 0.5),
          "fisot": np.full((W, C), 0.1)}
    temf = np.linspace(280.0, 220.0, L + 1)[None, :].repeat(C, 0)
    for planck in (False, True):
        kw = dict(nstr=nstr, planck=planck, wave_lower=[500.0], wave_upper=[800.0])
        m = disort_mp.disort_forward(prop, bc, temf, **kw)
        a = disort_np.disort_forward(prop, bc, temf, **kw)
        b = oracle_c.forward(prop, bc, temf, **kw)
        ea, eb = rel_err(a, m).max(), rel_err(b, m).max()
        print(f"  nstr {nstr} planck {planck}: numpy {ea:.2e}  C {eb:.2e}")
        assert ea < 1e-12 and eb < 1e-12


def test_record_matches_flx_ref():
    """The eight-entry record and dfdt's scale, against tests/flx_ref.py (the NumPy
    intensity oracle's field at the nodes) on a benign column."""
    nstr = 8
    pm = np.array([[0.75 ** l for l in range(nstr + 1)]] * 3)
    kw = dict(umu0=0.55, fbeam=1.2, albedo=0.4, fisot=0.05, planck=True,
              temper=[210.0, 230.0, 250.0, 270.0], btemp=275.0, ttemp=140.0, temis=0.6,
              wvnmlo=500.0, wvnmhi=800.0)
    r = disort_mp.disort_column([0.2, 1.0, 0.6], [0.9, 0.5, 0.7], pm, nstr, **kw)
    f, s, _ = flx_ref_column([0.2, 1.0, 0.6], [0.9, 0.5, 0.7], pm, nstr, **kw)
    for k in range(8):
        assert rel_err(f[None, :, k:k + 1], r["flx"][None, :, k:k + 1]).max() < 1e-11, k
    np.testing.assert_allclose(r["scale"], s, rtol=1e-12)
    np.testing.assert_allclose(r["fdn"], r["rfldir"] + r["rfldn"], rtol=1e-15)


@pytest.mark.parametrize("case", ["1a", "1b", "1d"])
def test_disotest1(case):
    c = disotest()["cases"][case]
    pm = np.array([[1.0] + [0.0] * 16])
    r = disort_mp.disort_column([c["tau"]], [c["ssalb"]], pm, 16, umu0=0.1, fbeam=math.pi / 0.1)
    for key in ("rfldir", "rfldn", "flup"):
        got, exp = np.asarray(r[key]), np.asarray(c[key])
        assert np.all(np.abs(got - exp) <= 5e-6 * np.abs(exp) + 1e-6), (key, got, exp)


@pytest.mark.parametrize("nstr", [4, 8, 16])
def test_omega0_beam_closed_form(nstr):
    """omega = 0: the diffuse field is only the Lambert-reflected beam."""
    tau = np.array([0.1, 0.5, 0.3])
    mu0, f0, alb = 0.6, 2.0, 0.4
    r = disort_mp.disort_column(tau, np.zeros(3), np.ones((3, 1)), nstr, umu0=mu0, fbeam=f0,
                                albedo=alb)
    tc = np.concatenate([[0.0], np.cumsum(tau)])
    np.testing.assert_allclose(r["fdn"], mu0 * f0 * np.exp(-tc / mu0), rtol=1e-14)
    mu, w = disort_np.double_gauss(nstr // 2)
    iup = alb * mu0 * f0 * math.exp(-tc[-1] / mu0) / math.pi
    flup = [2 * math.pi * np.sum(w * mu * iup * np.exp(-(tc[-1] - t) / mu)) for t in tc]
    np.testing.assert_allclose(r["flup"], flup, rtol=1e-13)


@pytest.mark.parametrize("nstr", [2, 8, 16])
def test_isothermal_nonscattering_slab(nstr):
    """omega = 0, isothermal over a black surface at the same T: I+ = B everywhere,
    I- = B (1 - exp(-tau_above / mu))."""
    tau = np.array([0.2, 1.0, 0.05, 2.0])
    t, lo, hi = 250.0, 400.0, 900.0
    r = disort_mp.disort_column(tau, np.zeros(4), np.ones((4, 1)), nstr, planck=True,
                                temper=np.full(5, t), btemp=t, wvnmlo=lo, wvnmhi=hi)
    b = disort_np.plkavg(lo, hi, t)
    mu, w = disort_np.double_gauss(nstr // 2)
    tc = np.concatenate([[0.0], np.cumsum(tau)])
    np.testing.assert_allclose(r["flup"], math.pi * b, rtol=1e-14)
    fdn = [2 * math.pi * np.sum(w * mu * b * (1 - np.exp(-x / mu))) for x in tc]
    np.testing.assert_allclose(r["fdn"], fdn, rtol=1e-13, atol=1e-15 * b)
    np.testing.assert_allclose(r["uavgup"], 0.5 * b, rtol=1e-14)


def test_conservative_scattering_flux_constant():
    """ssa = 1 - 1e-12 (not dithered) over albedo 1: the net flux is what 1e-12 absorbs."""
    tau = np.array([0.3, 2.0, 5.0, 0.7])
    pm = np.array([[0.7 ** l for l in range(9)]] * 4)
    r = disort_mp.disort_column(tau, np.full(4, 1.0 - 1e-12), pm, 8, umu0=0.5, fbeam=1.0,
                                albedo=1.0)
    assert np.abs(r["fdn"] - r["flup"]).max() < 1e-9


def test_gauss_nodes_at_working_precision():
    with mp.workdps(60):
        xs, ws = disort_mp.double_gauss(16)
        assert abs(sum(ws) - 1) < mp.mpf(10) ** -57
        # exact for polynomials up to degree 31 on (0, 1): int x^31 = 1/32
        assert abs(sum(w * x ** 31 for x, w in zip(xs, ws)) - mp.mpf(1) / 32) < mp.mpf(10) ** -57
    mu, w = disort_np.double_gauss(16)
    np.testing.assert_allclose([float(x) for x in xs], mu, rtol=1e-14)


def _column_kwargs(b, c):
    """Column c of a one-wave batch in cdisort's order (top -> bottom)."""
    p = b["prop"][0, c, ::-1]
    pm = np.concatenate([np.ones((b["nlyr"], 1)), p[:, 2:2 + b["nmom"]]], axis=1)
    kw = {k: float(v[0, c]) for k, v in b["bc"].items()}
    if b["planck"]:
        kw.update(planck=True, temper=b["temf"][c, ::-1], wvnmlo=hard_cases.WAVE[0],
                  wvnmhi=hard_cases.WAVE[1])
    return (p[:, 0], p[:, 1], pm, b["nstr"]), kw


@pytest.mark.parametrize("family,name,col", [("thin_thermal", "top2", 6),   # tau 1e-12
                                             ("resonance", "scat", 0),      # delta 0
                                             ("conservative", "beam", 13)])  # 1 - ssa 1e-12
def test_50_and_90_digits_agree(family, name, col):
    """The reference does not depend on its working precision: 1e-30 relative to the
    column's largest flux between 50 and 90 digits, on the inputs that cost the double
    solvers their digits (10 to 17 of them)."""
    b = [x for x in hard_cases.batches(family, 8) if x["name"] == name][0]
    args, kw = _column_kwargs(b, col)
    a = disort_mp.disort_column(*args, dps=50, return_mp=True, **kw)["mp"]
    c = disort_mp.disort_column(*args, dps=90, return_mp=True, **kw)["mp"]
    with mp.workdps(90):
        for k in range(8):
            scale = max(abs(r[k]) for r in c)
            if scale == 0:
                assert all(r[k] == 0 for r in a)
                continue
            err = max(abs(x[k] - y[k]) for x, y in zip(a, c)) / scale
            print(f"  component {k}: {mp.nstr(err, 3)}")
            assert err < mp.mpf(10) ** -30


def _sample():
    out = []
    for nstr in (2, 4, 8):
        for family in hard_cases.FAMILIES:
            out.append((family, nstr))
    return out


@pytest.mark.parametrize("family,nstr", _sample())
def test_fixture_is_current(fixture, family, nstr):
    """Inputs of every batch are what tests/hard_cases.py builds, bitwise, and the stored
    record of two columns per batch is what the solver returns now."""
    stored = {b["name"]: b for b in fixture[family, nstr]}
    built = hard_cases.batches(family, nstr)
    assert sorted(stored) == sorted(b["name"] for b in built)
    for b in built:
        s = stored[b["name"]]
        assert np.array_equal(s["prop"], b["prop"]) and s["nmom"] == b["nmom"]
        assert sorted(s["bc"]) == sorted(b["bc"])
        for k in b["bc"]:
            assert np.array_equal(s["bc"][k], b["bc"][k]), k
        assert (s["temf"] is None) == (b["temf"] is None)
        if b["temf"] is not None:
            assert np.array_equal(s["temf"], b["temf"])
        ncol = b["prop"].shape[1]
        cols = sorted({0, ncol - 1}) if nstr == 8 else [ncol // 2]
        ref, scale = hard_cases.reference(b, cols)
        assert np.array_equal(s["ref"][:, cols], ref)
        # dfdt's scale is rebuilt from the stored record and the inputs
        np.testing.assert_allclose(s["scale"][:, cols], scale, rtol=1e-13, atol=0.0)


def test_fixture_is_current_nstr16(fixture):
    b = [x for x in hard_cases.batches("resonance", 16) if x["name"] == "scat"][0]
    s = [x for x in fixture["resonance", 16] if x["name"] == "scat"][0]
    assert np.array_equal(s["prop"], b["prop"])
    assert np.array_equal(s["bc"]["umu0"], b["bc"]["umu0"])
    ref, _ = hard_cases.reference(b, [2])
    assert np.array_equal(s["ref"][:, [2]], ref)


def test_fixture_covers_every_family_and_nstr(fixture):
    assert sorted(fixture) == sorted((f, n) for f in hard_cases.FAMILIES for n in hard_cases.NSTR)
    for bs in fixture.values():
        for b in bs:
            assert np.all(np.isfinite(b["ref"])) and np.all(np.isfinite(b["scale"]))


def test_resonance_umu0_sits_on_the_eigenvalue():
    """delta = 0: the stored umu0 is the double nearest 1/k_j of the middle layer."""
    b = hard_cases.batches("resonance", 8)[0]
    ssa, k = hard_cases.resonance_k(8, True)
    assert ssa == 0.9
    with mp.workdps(50):
        assert abs(mp.mpf(float(b["bc"]["umu0"][0, 0])) * k - 1) < mp.mpf(2) ** -52
        d = [float(mp.mpf(float(u)) * k - 1) for u in b["bc"]["umu0"][0]]
    np.testing.assert_allclose(d[1:], hard_cases.DELTAS[1:], rtol=2e-3)
