"""oracle/disort_mp.py, the arbitrary-precision pin of the flux solve, on the CPU.

* against both double oracles on benign columns (where all three must agree to rounding),
* against the published DISOTEST-1 fluxes and the closed forms of tests/test_oracle.py,
* against itself at 50 and 90 digits on the inputs the double oracles fail on,
* against the stored fixture tests/golden/flux_hard.npz (a stale file fails),
* with zd / radius (the pseudo-spherical beam): against tests/spher_ref.py on benign
  columns, against its own plane-parallel solve in the two limits, against an eigen-free
  integration on a resonance, and against tests/golden/spher_hard.npz.
"""

import math

import numpy as np
import pytest
from mpmath import mp

import hard_cases
import spher_hard_cases
import spher_ref
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


# --------------------------------------------------------------------------- #
# zd / radius: the pseudo-spherical beam
# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def spher_fixture():
    return spher_hard_cases.load(GOLDEN)


@pytest.mark.parametrize("planck", [False, True], ids=["beam", "beam_planck"])
@pytest.mark.parametrize("nstr", [2, 4, 8, 16])
def test_spher_matches_spher_ref_on_benign_columns(nstr, planck):
    """The batch of tests/test_gpu_spher.py (mu0 from 1 to 0.02, a layer of tau = 0, delta-M
    active), per-column altitudes at nstr 8: the double restatement resolves these to
    rounding.  The full record, 1e-12 in the project's metric."""
    prop, bc, temf, zd = spher_ref.batch_inputs(nstr, "thin_bottom", planck, nstr == 8)
    prop, bc = prop[:1], {k: v[:1] for k, v in bc.items()}
    kw = dict(nstr=nstr, planck=planck, wave_lower=[spher_ref.WAVES[0][0]],
              wave_upper=[spher_ref.WAVES[0][1]], zd=zd, radius=spher_ref.RADIUS)
    flx, scale = disort_mp.flx_forward(prop, bc, temf, **kw)
    flux, dflx, dscale = spher_ref.spher_forward(prop, bc, temf, **kw)
    assert np.array_equal(disort_mp.disort_forward(prop, bc, temf, **kw),
                          disort_mp.flux_of_record(flx))
    e = rel_err(flux, disort_mp.flux_of_record(flx)).max()
    print(f"  nstr {nstr} planck {planck}: fluxes {e:.2e}")
    assert e < 1e-12
    # the other entries are sums and differences of numbers no larger than the column's
    # largest (rfldn at the top is rfldir - rfldir): 1e-12 of that, entry by entry
    big = np.abs(flx).max(axis=(2, 3), keepdims=True)
    assert (np.abs(dflx - flx) <= 1e-12 * big).all()
    np.testing.assert_allclose(dscale, scale, rtol=1e-12)


def _benign_column(nstr):
    pm = np.array([[g ** l for l in range(nstr + 1)] for g in (0.5, 0.7, 0.6)])
    return ([0.4, 1.0, 0.8], [0.6, 0.9, 0.7], pm, nstr), dict(
        fbeam=1.3, albedo=0.3, planck=True, temper=[210.0, 230.0, 250.0, 270.0], btemp=275.0,
        ttemp=140.0, temis=0.6, wvnmlo=500.0, wvnmhi=800.0)


def test_spher_overhead_sun_is_plane_parallel():
    """g = 1 identically at mu0 = 1, so ch' = tau', lambda = 1: the same numbers."""
    args, kw = _benign_column(8)
    a = disort_mp.disort_column(*args, umu0=1.0, zd=spher_hard_cases.ZD3, radius=3.39e6, **kw)
    b = disort_mp.disort_column(*args, umu0=1.0, **kw)
    assert np.abs(a["flx"] - b["flx"]).max() <= 1e-15 * np.abs(b["flx"]).max()


def test_spher_large_radius_tends_to_plane_parallel():
    """g - 1/mu0 = O(z / R): at R = 1e30 the difference is far below double rounding, at
    R = 1e9 (z / R = 4.5e-5) it is that order."""
    args, kw = _benign_column(8)
    b = disort_mp.disort_column(*args, umu0=0.3, **kw)
    far = disort_mp.disort_column(*args, umu0=0.3, zd=spher_hard_cases.ZD3, radius=1e30, **kw)
    near = disort_mp.disort_column(*args, umu0=0.3, zd=spher_hard_cases.ZD3, radius=1e9, **kw)
    scale = np.abs(b["flx"]).max()
    assert np.abs(far["flx"] - b["flx"]).max() <= 1e-15 * scale
    d = np.abs(near["flx"] - b["flx"]).max() / scale
    assert 1e-7 < d < 1e-3, d


@pytest.mark.parametrize("name,col", [("scat", 0), ("negative", 0), ("top", 0)])
def test_spher_50_and_90_digits_agree_on_a_resonance(name, col):
    _digits_agree([x for x in spher_hard_cases.batches("resonance", 8) if x["name"] == name][0],
                  col)


def test_spher_50_and_90_digits_agree_on_a_thin_layer():
    """tau' 1e-12 under a thick layer (lambda about -5e12), mu0 = 1e-3."""
    _digits_agree([x for x in spher_hard_cases.batches("low_sun", 8)
                   if x["name"] == "thin_under_thick_planck"][0], 3)


def _digits_agree(b, col):
    args, kw = spher_hard_cases.column_kwargs(b, col)
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


def test_spher_resonance_against_the_propagator():
    """nstr 2, the three-layer resonance column at delta = 0: spher_ref.propagator_column
    integrates the 2N-stream equation by matrix exponentials, has no eigen-solution and is
    regular where lambda = k_j -- an independent pin exactly where spher_ref.spher_column
    is wrong by O(1).  (Not above nstr 2 on these depths: an initial-value integration.)"""
    b = [x for x in spher_hard_cases.batches("resonance", 2) if x["name"] == "scat"][0]
    c = int(np.flatnonzero(b["delta"] == 0.0)[0])
    args, kw = spher_hard_cases.column_kwargs(b, c)
    r = disort_mp.disort_column(*args, return_mp=True, **kw)
    with mp.workdps(50):
        assert abs(r["lam"][1] / r["kk"][1][0] - 1) < mp.mpf(10) ** -12
    fu, fd, _, _ = spher_ref.propagator_column(*args, zd=kw["zd"], radius=kw["radius"],
                                               umu0=kw["umu0"], fbeam=kw["fbeam"],
                                               albedo=kw["albedo"])
    e = rel_err(np.stack([fu, fd], -1)[None], np.stack([r["flup"], r["fdn"]], -1)[None]).max()
    print(f"  propagator vs mp: {e:.2e}")
    assert e < 1e-12
    d = spher_ref.spher_column(*args, **kw)
    e_ref = rel_err(np.stack([d["flup"], d["fdn"]], -1)[None],
                    np.stack([r["flup"], r["fdn"]], -1)[None]).max()
    print(f"  spher_ref.spher_column vs mp: {e_ref:.2e}")


@pytest.mark.parametrize("family,nstr", [(f, n) for n in (2, 4, 8)
                                         for f in spher_hard_cases.FAMILIES])
def test_spher_fixture_is_current(spher_fixture, family, nstr):
    """Inputs of every batch are what tests/spher_hard_cases.py builds, bitwise, and the
    stored record of two columns per batch (one at nstr 2 and 4) is what the solver returns
    now, to 1e-13."""
    stored = {b["name"]: b for b in spher_fixture[family, nstr]}
    built = spher_hard_cases.batches(family, nstr)
    assert sorted(stored) == sorted(b["name"] for b in built)
    for b in built:
        s = stored[b["name"]]
        assert np.array_equal(s["prop"], b["prop"]) and s["nmom"] == b["nmom"]
        assert np.array_equal(s["zd"], b["zd"]) and s["radius"] == b["radius"]
        assert sorted(s["bc"]) == sorted(b["bc"])
        for k in b["bc"]:
            assert np.array_equal(s["bc"][k], b["bc"][k]), k
        assert (s["temf"] is None) == (b["temf"] is None)
        if b["temf"] is not None:
            assert np.array_equal(s["temf"], b["temf"])
        if "delta" in b:
            assert np.array_equal(s["delta"], b["delta"])
            assert np.abs(s["delta_realised"] - b["delta"]).max() <= spher_hard_cases.DELTA_TOL
        ncol = b["prop"].shape[1]
        cols = sorted({0, ncol - 1}) if nstr == 8 else [ncol // 2]
        ref, scale = spher_hard_cases.reference(b, cols)
        assert rel_err(disort_mp.flux_of_record(s["ref"][:, cols]),
                       disort_mp.flux_of_record(ref)).max() <= 1e-13
        np.testing.assert_allclose(s["ref"][:, cols], ref, rtol=1e-13, atol=1e-13 * np.abs(ref).max())
        np.testing.assert_allclose(s["scale"][:, cols], scale, rtol=1e-13, atol=0.0)


def test_spher_fixture_covers_every_family_and_nstr(spher_fixture):
    assert sorted(spher_fixture) == sorted((f, n) for f in spher_hard_cases.FAMILIES
                                           for n in spher_hard_cases.NSTR)
    shared = {f: False for f in spher_hard_cases.FAMILIES}
    own = dict(shared)
    for (family, _), bs in spher_fixture.items():
        for b in bs:
            assert np.all(np.isfinite(b["ref"])) and np.all(np.isfinite(b["scale"]))
            assert b["nlyr"] <= 5 and b["prop"].shape[1] <= 24
            shared[family] |= b["zd"].ndim == 1
            own[family] |= b["zd"].ndim == 2
    assert all(shared.values()) and all(own.values())  # both prologue addressings
