"""Pseudo-spherical ray radiances on the device (hd_solve_rays_spher through
``Disort.forward_rays(..., zd=)`` / ``forward_rays_band``) against tests/rays_spher_ref.py:
parity at nstr 4, 8, 16 with and without the intensity correction, the two exact limits,
the flux output, chunked calls, the fused band sum, status flags and the C++ drop-in
(DESIGN.md sections 3b and 3e).

The batch is spher_ref.batch_inputs: nwave 2 x ncol 4 x nlyr 5, mu0 = 1, 0.5, 0.1, 0.02 by
column, a layer of dtau = 0 in column 1, albedo 0.3, delta-M active; phi0 is random.  Six
rays per column: mu = +-0.02, +-1, a quadrature node, and (-mu0, phi0), looking into the
sun.  Error metric and bound: test_gpu_rays.py's ``_col_err`` and helpers.TOL through
``margin()``.
"""

import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import rays_spher_ref as RS
import spher_ref as S
from helpers import TOL, margin
from oracle.disort_np import double_gauss
from test_gpu_rays import _col_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
WL = [w[0] for w in S.WAVES]
WU = [w[1] for w in S.WAVES]
CORINT = ",intensity_correction,old_intensity_correction"
BAD_INPUT, RESONANCE, ERROR_MASK = 0x01, 0x10, 0x0F
UTAU = (0.0, 0.2, 0.55, 0.9, 1.002)  # 1.002: the thinnest column's total depth
NRAY = 6


def _t(x):
    return None if x is None else torch.tensor(np.array(x), dtype=torch.float64, device=DEV)


def _bc(bc):
    return {k: _t(v) for k, v in bc.items()}


def _disort(nstr, nlyr, nwave, ncol, *, planck=False, corint=False, utau=None, radius=S.RADIUS,
            flags="lamber,quiet"):
    from pyharp_amd import Disort, DisortOptions
    op = DisortOptions().flags(flags + (",planck" if planck else "") +
                               (",usrtau" if utau is not None else "") +
                               (CORINT if corint else ""))
    op.nwave(nwave).ncol(ncol).radius(radius)
    if planck:
        op.wave_lower(list(map(float, WL))).wave_upper(list(map(float, WU)))
    if utau is not None:
        op.user_tau(list(utau))
    op.ds().nlyr, op.ds().nstr, op.ds().nmom = nlyr, nstr, nstr
    return Disort(op)


def _with_chunk(chunk, fn):
    from pyharp_amd.disort import _context
    ctx = _context(0)
    ctx.set_chunk(chunk)
    try:
        return fn()
    finally:
        ctx.set_chunk(0)


@functools.lru_cache(maxsize=None)
def _inputs(nstr, profile, planck, per_zd, per_rays):
    """spher_ref.batch_inputs with a random phi0 and the six rays, shared or per column."""
    prop, bc, temf, zd = S.batch_inputs(nstr, profile, planck, per_zd)
    nwave, ncol = prop.shape[:2]
    rng = np.random.default_rng(977 + nstr)
    bc = dict(bc, phi0=rng.uniform(0.0, 360.0, (nwave, ncol)))
    mu_q, _ = double_gauss(nstr // 2)
    umu = np.zeros((ncol, NRAY))
    phi = rng.uniform(0.0, 360.0, (ncol, NRAY))
    umu[:, :5] = [0.02, -0.02, 1.0, -1.0, mu_q[nstr // 4]]
    umu[:, 5] = -bc["umu0"][0]       # into the sun of wave 0
    phi[:, 5] = bc["phi0"][0]
    if not per_rays:
        umu, phi = umu[1].copy(), phi[1].copy()  # column 1's rays for every column
    for a in (prop, temf, zd, umu, phi, *bc.values()):
        if a is not None:
            a.setflags(write=False)
    return prop, bc, temf, zd, umu, phi


@functools.lru_cache(maxsize=None)
def _reference(nstr, profile, planck, per_zd, per_rays, interior):
    """(rad without, rad with the intensity correction, flux), computed once."""
    prop, bc, temf, zd, umu, phi = _inputs(nstr, profile, planck, per_zd, per_rays)
    kw = dict(zd=zd, radius=S.RADIUS, nstr=nstr, umu=umu, phi=phi,
              utau=np.asarray(UTAU) if interior else None, planck=planck, wave_lower=WL,
              wave_upper=WU)
    plain, flux = RS.rays_spher_forward(prop, bc, temf, **kw)
    cor, _ = RS.rays_spher_forward(prop, bc, temf, corint=True, **kw)
    for a in (plain, cor, flux):
        a.setflags(write=False)
    return plain, cor, flux


def _call(d, prop, bc, temf, zd, umu, phi, **kw):
    return d.forward_rays(_t(prop), _bc(bc), _t(temf), umu=_t(umu), phi=_t(phi), zd=_t(zd), **kw)


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("corint", [False, True], ids=["plain", "corint"])
@pytest.mark.parametrize("interior", [False, True], ids=["levels", "user_tau"])
@pytest.mark.parametrize("per_rays", [False, True], ids=["shared_rays", "column_rays"])
@pytest.mark.parametrize("per_zd", [False, True], ids=["shared_zd", "column_zd"])
@pytest.mark.parametrize("planck", [False, True], ids=["beam", "beam_planck"])
@pytest.mark.parametrize("profile", list(S.TAU_PROFILES))
@pytest.mark.parametrize("nstr", [4, 8, 16])
def test_parity_with_reference(nstr, profile, planck, per_zd, per_rays, interior, corint):
    prop, bc, temf, zd, umu, phi = _inputs(nstr, profile, planck, per_zd, per_rays)
    ref = _reference(nstr, profile, planck, per_zd, per_rays, interior)
    nwave, ncol, nlyr = prop.shape[:3]
    d = _disort(nstr, nlyr, nwave, ncol, planck=planck, corint=corint,
                utau=UTAU if interior else None)
    st = torch.zeros(nwave * ncol, dtype=torch.int32, device=DEV)
    flux = torch.empty((nwave, ncol, d.ds().ntau, 2), dtype=torch.float64, device=DEV)
    rad = _call(d, prop, bc, temf, zd, umu, phi, status=st, flux=flux).cpu().numpy()
    assert not (st.cpu().numpy() & ERROR_MASK).any()
    err = _col_err(rad, ref[1] if corint else ref[0])
    ferr = _col_err(flux.cpu().numpy(), ref[2])
    print(f"nstr {nstr} {profile} planck={planck} zd/col={per_zd} rays/col={per_rays} "
          f"interior={interior} corint={corint}: rad {err:.3e} flux {ferr:.3e}")
    assert margin(err) < TOL
    assert margin(ferr) < TOL


# ------------------------------------------------------------------ 2. limits
@pytest.mark.parametrize("corint", [False, True], ids=["plain", "corint"])
@pytest.mark.parametrize("nstr", [8, 16])
def test_large_radius_equals_plane_parallel(nstr, corint):
    prop, bc, temf, zd, umu, phi = _inputs(nstr, "thin_bottom", False, False, True)
    nwave, ncol, nlyr = prop.shape[:3]
    a = _call(_disort(nstr, nlyr, nwave, ncol, corint=corint, radius=1e12 * zd[-1], utau=UTAU),
              prop, bc, temf, zd, umu, phi).cpu().numpy()
    b = _disort(nstr, nlyr, nwave, ncol, corint=corint, utau=UTAU).forward_rays(
        _t(prop), _bc(bc), umu=_t(umu), phi=_t(phi)).cpu().numpy()
    err = _col_err(a, b)
    print("R = 1e12 z_top vs plain", nstr, corint, err)
    assert margin(err) < TOL


@pytest.mark.parametrize("corint", [False, True], ids=["plain", "corint"])
@pytest.mark.parametrize("nstr", [8, 16])
def test_overhead_sun_equals_plane_parallel(nstr, corint):
    """column 0 (mu0 = 1) at Mars radius: every g = 1"""
    prop, bc, temf, zd, umu, phi = _inputs(nstr, "uniform", False, True, True)
    nwave, ncol, nlyr = prop.shape[:3]
    a = _call(_disort(nstr, nlyr, nwave, ncol, corint=corint, utau=UTAU), prop, bc, temf, zd,
              umu, phi).cpu().numpy()
    b = _disort(nstr, nlyr, nwave, ncol, corint=corint, utau=UTAU).forward_rays(
        _t(prop), _bc(bc), umu=_t(umu), phi=_t(phi)).cpu().numpy()
    assert bc["umu0"][0, 0] == 1.0
    err = _col_err(a[:, :1], b[:, :1])
    print("mu0 = 1 vs plain", nstr, corint, err)
    assert margin(err) < TOL
    assert _col_err(a[:, 3:], b[:, 3:]) > 1e-3  # mu0 = 0.02: the geometries disagree


# ------------------------------------------------------------------ 3. fluxes
@pytest.mark.parametrize("nstr", [8])
def test_flux_along_rays_matches_forward_spher(nstr):
    """``flux=`` at the layer boundaries against ``forward(zd=)`` of an 'onlyfl,spher'
    module on the same inputs, at test_gpu_rays.py::test_flux_along_rays_matches_forward's
    tolerance, which is equality: the level fluxes of the ray call are the flux solve's own
    (hd_solve_rays_spher runs it first), so the two outputs of one model are one set of
    numbers.  (Taken from the intensity path's level field instead they differed by 4.0e-15
    of the column maximum: two algorithms, equal to rounding only.)  Also with chunks that
    cut waves, and with a status buffer that then carries both solves' bits."""
    prop, bc, temf, zd, umu, phi = _inputs(nstr, "thin_bottom", False, True, True)
    nwave, ncol, nlyr = prop.shape[:3]
    flux = torch.empty((nwave, ncol, nlyr + 1, 2), dtype=torch.float64, device=DEV)
    _call(_disort(nstr, nlyr, nwave, ncol), prop, bc, temf, zd, umu, phi, flux=flux)
    f = _disort(nstr, nlyr, nwave, ncol, flags="lamber,quiet,onlyfl,spher")
    bcf = {k: v for k, v in bc.items() if k != "phi0"}
    ref = f.forward(_t(prop), _bc(bcf), zd=_t(zd)).cpu().numpy()
    got = flux.cpu().numpy()
    print("flux along rays vs forward(zd=): max |d| / column max", _col_err(got, ref))
    assert np.array_equal(got, ref)
    st = torch.zeros(nwave * ncol, dtype=torch.int32, device=DEV)
    cut = torch.empty_like(flux)
    rad = _call(_disort(nstr, nlyr, nwave, ncol), prop, bc, temf, zd, umu, phi)
    rcut = _with_chunk(3, lambda: _call(_disort(nstr, nlyr, nwave, ncol), prop, bc, temf, zd, umu,
                                        phi, flux=cut, status=st))
    assert np.array_equal(cut.cpu().numpy(), ref) and torch.equal(rcut, rad)
    assert not (st.cpu().numpy() & ERROR_MASK).any()


# ------------------------------------------------------------------ 4. chunks, band sum
@pytest.mark.parametrize("nstr,planck,corint", [(8, False, True), (16, True, False)])
def test_chunks_and_band(nstr, planck, corint):
    from pyharp_amd.spectral import band_rad
    prop, bc, temf, zd, umu, phi = _inputs(nstr, "thin_bottom", planck, True, True)
    nwave, ncol, nlyr = prop.shape[:3]
    d = _disort(nstr, nlyr, nwave, ncol, planck=planck, corint=corint, utau=UTAU)
    one = _call(d, prop, bc, temf, zd, umu, phi)
    w = _t([0.7, 0.4])
    bunf = band_rad(one, w)
    args = (_t(prop), _bc(bc), _t(temf))
    kw = dict(umu=_t(umu), phi=_t(phi), zd=_t(zd))
    for chunk in (3, 5):  # chunks that cut waves (ncol 4)
        cut = _with_chunk(chunk, lambda: d.forward_rays(*args, **kw))
        assert torch.equal(cut, one)
        band = _with_chunk(chunk, lambda: d.forward_rays_band(*args, weights=w, **kw))
        assert torch.equal(band, bunf)
    stored = torch.empty_like(one)
    band = d.forward_rays_band(*args, weights=w, rad=stored, **kw)
    assert torch.equal(band, bunf) and torch.equal(stored, one)


# ------------------------------------------------------------------ 5. status
@pytest.mark.parametrize("corint", [False, True], ids=["plain", "corint"])
def test_bad_zd_flags_its_column(corint):
    nstr = 8
    prop, bc, temf, zd, umu, phi = _inputs(nstr, "uniform", True, True, True)
    nwave, ncol, nlyr = prop.shape[:3]
    d = _disort(nstr, nlyr, nwave, ncol, planck=True, corint=corint, utau=UTAU)
    clean = _call(d, prop, bc, temf, zd, umu, phi)
    z = np.array(zd)
    z[2, 3] = z[2, 2]
    st = torch.zeros(nwave * ncol, dtype=torch.int32, device=DEV)
    got = _call(d, prop, bc, temf, z, umu, phi, status=st)
    st = st.cpu().numpy().reshape(nwave, ncol)
    assert ((st & BAD_INPUT) != 0).tolist() == [[False, False, True, False]] * nwave
    keep = [0, 1, 3]
    assert torch.equal(got[:, keep], clean[:, keep])
    fb = np.array(bc["fbeam"])
    fb[:, 2] = 0.0
    off = _call(d, prop, dict(bc, fbeam=fb), temf, zd, umu, phi)
    assert torch.isfinite(got).all() and got[:, 2].abs().max().item() > 0.0  # the Planck source
    assert (got[:, 2] - off[:, 2]).abs().max().item() <= 1e-13 * off[:, 2].abs().max().item()


def test_resonance_is_a_warning():
    """The top layer's secant lam = g(j, j) bisected (spher_hard_cases' helpers) onto one of
    the layer's mode-0 eigenvalues: the warning bit, no error bit, finite output.  No
    accuracy is asserted at a resonance."""
    from spher_hard_cases import _tune_mu0, scaled_depths
    nstr = 8
    prop, bc, temf, zd, umu, phi = _inputs(nstr, "uniform", False, False, False)
    nwave, ncol, nlyr = prop.shape[:3]
    p = prop[0, 0, ::-1]
    pm = np.concatenate([np.ones((nlyr, 1)), p[:, 2:]], axis=1)
    r = RS.rays_spher_column(p[:, 0], p[:, 1], pm, nstr, zd=zd, radius=S.RADIUS, umu=[0.5],
                             phi=[0.0], umu0=0.5, fbeam=1.0)
    kk = r["sol"][0]["kk"][0]
    k = kk[np.argmin(np.abs(kk - 3.0))]
    tp = scaled_depths(p[:, 0], p[:, 1], [list(row[1:]) for row in pm], nstr)
    mu0 = _tune_mu0(zd, tp, 0, k)
    lam = S.layer_secants(zd, S.RADIUS, mu0, tp)[1][0]
    assert abs(lam / k - 1.0) < 1e-12
    bc = dict(bc, umu0=np.full((nwave, ncol), 0.5))
    bc["umu0"][0, 0] = mu0
    umu = np.array(umu)
    umu[5] = -0.5
    st = torch.zeros(nwave * ncol, dtype=torch.int32, device=DEV)
    rad = _call(_disort(nstr, nlyr, nwave, ncol), prop, bc, temf, zd, umu, phi, status=st)
    st = st.cpu().numpy()
    print("resonance status", st)
    assert st[0] & RESONANCE
    assert not (st & ERROR_MASK).any()
    assert torch.isfinite(rad).all()


def test_nstr_18_is_refused():
    from pyharp_amd import _lib
    from pyharp_amd.disort import _context
    prop, bc, temf, zd, umu, phi = _inputs(16, "uniform", False, False, False)
    nwave, ncol, nlyr = prop.shape[:3]
    d = _disort(16, nlyr, nwave, ncol)
    cfg, inp, keep = d._stage(_t(prop), _bc({k: v for k, v in bc.items() if k != "phi0"}), None,
                              DEV)
    cfg.nstr = 18
    mu, ph, z = _t(umu), _t(phi), _t(zd)
    out = torch.empty((nwave, ncol, nlyr + 1, NRAY), dtype=torch.float64, device=DEV)
    rays = _lib.HdRays(nray=NRAY, per_column=0, umu=mu.data_ptr(), phi=ph.data_ptr(), ntau=0,
                       utau=None, phi0=None, corint=0, weight=None, brad=None)
    sph = _lib.HdSphere(radius=S.RADIUS, zd=z.data_ptr(), per_column=0)
    with pytest.raises(RuntimeError, match="invalid argument"):
        _context(0).solve_rays_spher(cfg, inp, sph, rays, None, out.data_ptr(), None, None)
    for radius, zp in ((0.0, z.data_ptr()), (float("nan"), z.data_ptr()), (S.RADIUS, None)):
        cfg.nstr = 16
        bad = _lib.HdSphere(radius=radius, zd=zp, per_column=0)
        with pytest.raises(RuntimeError, match="invalid argument"):
            _context(0).solve_rays_spher(cfg, inp, bad, rays, None, out.data_ptr(), None, None)
    from pyharp_amd import Disort, DisortOptions
    op = DisortOptions().flags("lamber,quiet").nwave(nwave).ncol(ncol).radius(S.RADIUS)
    op.ds().nlyr, op.ds().nstr, op.ds().nmom = nlyr, 18, 18
    with pytest.raises(RuntimeError, match="nstr <= 16"):
        Disort(op).forward_rays(_t(np.zeros((nwave, ncol, nlyr, 20))), {}, umu=mu, phi=ph, zd=z)


# ------------------------------------------------------------------ 6. C++ drop-in
def test_cpp_dropin():
    """harp_amd::DisortImpl::forward_rays / forward_rays_band with zd (tests/cpp/
    disort_rays_spher_dropin.cpp, built by tests/cpp/build_rays_spher.sh) against the
    Python call on the same batch."""
    exe = os.path.join(ROOT, "tests", "cpp", "disort_rays_spher_dropin")
    if not os.path.exists(exe):
        subprocess.run([os.path.join(ROOT, "tests", "cpp", "build_rays_spher.sh")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    nwave, ncol, nlyr, nstr, nray = 2, 2, 5, 8, 3
    got = np.full((nwave, ncol, nlyr + 1, nray), np.nan)
    band = np.full((ncol, nlyr + 1, nray), np.nan)
    for line in out.strip().splitlines():
        f = line.split()
        if f[0] == "rad":
            got[int(f[1]), int(f[2]), int(f[3]), int(f[4])] = float(f[5])
        else:
            assert f[0] == "band"
            band[int(f[1]), int(f[2]), int(f[3])] = float(f[4])
    prop = np.zeros((nwave, ncol, nlyr, 2 + nstr))
    for w in range(nwave):
        for c in range(ncol):
            for l in range(nlyr):
                prop[w, c, l, 0] = 0.1 + 0.05 * l + 0.02 * w
                prop[w, c, l, 1] = 0.5 + 0.08 * l - 0.1 * c
                prop[w, c, l, 2:] = (0.6 + 0.05 * c) ** np.arange(1, nstr + 1)
    bc = {"fbeam": np.full((nwave, ncol), 1.5),
          "umu0": np.broadcast_to(np.array([0.5, 0.1]), (nwave, ncol)).copy(),
          "albedo": np.full((nwave, ncol), 0.3), "phi0": np.full((nwave, ncol), 20.0)}
    zd = 2.0e4 * np.arange(nlyr + 1.0)
    umu, phi = np.array([0.7, -0.02, -1.0]), np.array([10.0, 130.0, 250.0])
    d = _disort(nstr, nlyr, nwave, ncol, corint=True)
    py = _call(d, prop, bc, None, zd, umu, phi).cpu().numpy()
    # the C++ program fills prop with std::pow, this test with numpy's power: one ulp apart
    assert np.abs(got - py).max() <= 1e-12 * np.abs(py).max()
    assert np.abs(band - (0.7 * py[0] + 0.4 * py[1])).max() <= 1e-12 * np.abs(py).max()
    ref, _ = RS.rays_spher_forward(prop, bc, zd=zd, radius=S.RADIUS, nstr=nstr, umu=umu, phi=phi,
                                   corint=True)
    assert margin(_col_err(got, ref)) < TOL
