"""HIP ray radiances (hd_solve_rays through Disort.forward_rays / forward_rays_band):
paired outgoing directions, shared or per column, with the band sum fused into the
solve -- against the radiance oracle (oracle/disort_rad_np.py, called once per column
with that column's own umu / phi lists; a ray is the diagonal entry uref[w, 0, r, lu, r]
of its grid), the grid path's own diagonal and DISOTEST-1's published radiances.

Tolerance: the project's TOL = 1e-6 relative to the column's largest radiance, as in
tests/test_gpu_radiance.py, whose input distributions these cases share.
"""

import functools
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from helpers import TOL, disotest, margin
from oracle.disort_rad_np import disort_rad_forward

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORINT = ",intensity_correction,old_intensity_correction"


def _disort(nstr, nlyr, nwave, ncol, *, flags, utau=None, planck=False, wl=None, wu=None,
            nmom=None, umu=None, phi=None):
    from pyharp_amd import Disort, DisortOptions
    op = DisortOptions().flags(flags + (",planck" if planck else "")).nwave(nwave).ncol(ncol)
    if planck:
        op.wave_lower(list(map(float, wl))).wave_upper(list(map(float, wu)))
    if utau is not None:
        op.user_tau(list(utau))
    if umu is not None:
        op.user_mu(list(umu))
    if phi is not None:
        op.user_phi(list(phi))
    op.ds().nlyr = nlyr
    op.ds().nstr = nstr
    op.ds().nmom = nstr if nmom is None else nmom
    return Disort(op)


def _dev(d):
    return {k: torch.as_tensor(v, dtype=torch.float64, device=DEV) for k, v in d.items()}


def _t(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64, device=DEV)


def _col_err(got, ref):
    """max |got - ref| / max |ref| per (wave, col)"""
    g = got.reshape(got.shape[0] * got.shape[1], -1)
    r = ref.reshape(ref.shape[0] * ref.shape[1], -1)
    scale = np.maximum(np.abs(r).max(axis=1, keepdims=True), 1e-300)
    return (np.abs(g - r) / scale).max()


def _random_case(rng, nwave, ncol, nlyr, nstr, planck, beam=True):
    """the distributions of tests/test_gpu_radiance.py::_random_case"""
    prop = np.zeros((nwave, ncol, nlyr, 2 + nstr))
    prop[..., 0] = 10.0 ** rng.uniform(-3, 0.7, (nwave, ncol, nlyr))
    prop[..., 1] = rng.uniform(0, 0.99, (nwave, ncol, nlyr))
    gg = rng.uniform(0, 0.8, (nwave, ncol, nlyr))
    for l in range(nstr):
        prop[..., 2 + l] = gg ** (l + 1)
    bc = {"albedo": rng.uniform(0, 1, (nwave, ncol)), "fisot": np.full((nwave, ncol), 0.01)}
    if beam:
        bc.update(fbeam=rng.uniform(0.5, 2, (nwave, ncol)), umu0=rng.uniform(0.1, 1, (nwave, ncol)),
                  phi0=rng.uniform(0, 360, (nwave, ncol)))
    kw = {}
    if planck:
        from oracle.disort_np import layer2level
        kw["temf"] = layer2level(np.linspace(290, 180, nlyr)[None, :] +
                                 rng.uniform(-5, 5, (ncol, nlyr)))
        bc["btemp"] = np.full((nwave, ncol), 295.0)
        bc["ttemp"] = np.full((nwave, ncol), 150.0)
        bc["temis"] = np.full((nwave, ncol), 0.3)
        kw["wave_lower"] = np.sort(rng.uniform(100, 1500, nwave))
        kw["wave_upper"] = kw["wave_lower"] + rng.uniform(10, 300, nwave)
    return prop, bc, kw


def _random_rays(rng, ncol, nray):
    """|umu| in [0.1, 1] with a random sign, both hemispheres in every column"""
    umu = rng.uniform(0.1, 1.0, (ncol, nray)) * rng.choice([-1.0, 1.0], (ncol, nray))
    umu[:, 0] = np.abs(umu[:, 0])
    umu[:, 1] = -np.abs(umu[:, 1])
    return umu, rng.uniform(0.0, 360.0, (ncol, nray))


def _oracle_rays(prop, bc, kw, nstr, umu, phi, utau, *, planck=False, corint=False, nmom=None):
    """(nwave, ncol, ntau, nray): the oracle once per column on that column's umu x phi
    grid, a ray = the grid's diagonal"""
    nwave, ncol = prop.shape[:2]
    umu = np.broadcast_to(umu, (ncol, umu.shape[-1]))
    phi = np.broadcast_to(phi, umu.shape)
    nray = umu.shape[1]
    out = None
    for c in range(ncol):
        bcc = {k: np.asarray(v)[:, c:c + 1] for k, v in bc.items()}
        temf = kw["temf"][c:c + 1] if "temf" in kw else None
        _, uref = disort_rad_forward(prop[:, c:c + 1], bcc, temf, nstr=nstr, umu=umu[c],
                                     phi=phi[c], utau=utau, nmom=nmom, planck=planck,
                                     wave_lower=kw.get("wave_lower"),
                                     wave_upper=kw.get("wave_upper"), corint=corint)
        if out is None:
            out = np.zeros((nwave, ncol, uref.shape[3], nray))
        r = np.arange(nray)
        out[:, c] = uref[:, 0, r, :, r].transpose(1, 2, 0)
    return out


def _utau5(rng, prop):
    total = prop[..., 0].sum(axis=-1).min()
    return np.sort(np.concatenate([[0.0, total], rng.uniform(0, total, 3)]))


def _temf(kw):
    return None if "temf" not in kw else torch.as_tensor(kw["temf"], device=DEV)


# --- 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("nstr", [4, 16, 24, 32])
@pytest.mark.parametrize("planck", [False, True])
def test_per_column_rays_vs_oracle(nstr, planck):
    """each column its own five rays, both hemispheres, top / bottom / interior depths:
    the register-path and user-map kernels (nstr 4, 16) and, at nstr 24 / 32, the rolled
    one-lane user kernel that per-column rays take there"""
    rng = np.random.default_rng(8100 + nstr + 50 * planck)
    nwave, ncol, nlyr, nray = 2, 3, 6, 5
    prop, bc, kw = _random_case(rng, nwave, ncol, nlyr, nstr, planck)
    utau = _utau5(rng, prop)
    umu, phi = _random_rays(rng, ncol, nray)
    d = _disort(nstr, nlyr, nwave, ncol, flags="usrtau,lamber,quiet", utau=utau, planck=planck,
                wl=kw.get("wave_lower"), wu=kw.get("wave_upper"))
    rad = d.forward_rays(_t(prop), _dev(bc), _temf(kw), umu=_t(umu), phi=_t(phi))
    assert tuple(rad.shape) == (nwave, ncol, 5, nray) and rad.device == DEV
    ref = _oracle_rays(prop, bc, kw, nstr, umu, phi, utau, planck=planck)
    err = _col_err(rad.cpu().numpy(), ref)
    print("per-column rays", nstr, planck, err)
    assert margin(err) < TOL, err


# --- 2 ---------------------------------------------------------------------------
@pytest.mark.parametrize("nstr", [8, 24])
def test_shared_rays_match_grid_diagonal(nstr):
    """shared rays (nray,) against the diagonal of get_rad() for user_mu = umu_r,
    user_phi = phi_r: the same per-mode arithmetic (nstr 24: the team user kernels in
    both), only the epilogue differs -- 1e-12 of the column maximum"""
    rng = np.random.default_rng(8200 + nstr)
    nwave, ncol, nlyr, nray = 2, 3, 6, 7
    prop, bc, kw = _random_case(rng, nwave, ncol, nlyr, nstr, False)
    utau = _utau5(rng, prop)
    umu, phi = _random_rays(rng, 1, nray)
    umu, phi = umu[0], phi[0]
    g = _disort(nstr, nlyr, nwave, ncol, flags="usrtau,usrang,lamber,quiet", utau=utau,
                umu=umu, phi=phi)
    g.forward(_t(prop), _dev(bc))
    uu = g.get_rad().cpu().numpy()  # (nwave, ncol, nphi, ntau, numu)
    r = np.arange(nray)
    diag = uu[:, :, r, :, r].transpose(1, 2, 3, 0)
    d = _disort(nstr, nlyr, nwave, ncol, flags="usrtau,lamber,quiet", utau=utau)
    rad = d.forward_rays(_t(prop), _dev(bc), umu=_t(umu), phi=_t(phi)).cpu().numpy()
    assert rad.shape == diag.shape == (nwave, ncol, 5, nray)
    err = _col_err(rad, diag)
    print("shared rays vs grid diagonal", nstr, err)
    assert err < 1e-12, err


# --- 3 ---------------------------------------------------------------------------
def test_block_and_chunk_boundaries():
    """70 rays per column (a column's rays cross a 64-lane block) in chunks of 2 solves
    of a 2 x 3 batch (chunks start mid-wave: the column of a solve comes from its global
    index): against the oracle, and bitwise equal to the automatic chunking"""
    from pyharp_amd.disort import _context
    rng = np.random.default_rng(8300)
    nstr, nwave, ncol, nlyr, nray = 4, 2, 3, 5, 70
    prop, bc, kw = _random_case(rng, nwave, ncol, nlyr, nstr, False)
    total = prop[..., 0].sum(axis=-1).min()
    utau = [0.0, 0.4 * total, total]
    umu, phi = _random_rays(rng, ncol, nray)
    d = _disort(nstr, nlyr, nwave, ncol, flags="usrtau,lamber,quiet", utau=utau)
    args = (_t(prop), _dev(bc))
    auto = d.forward_rays(*args, umu=_t(umu), phi=_t(phi)).cpu().numpy()
    ctx = _context(0)
    ctx.set_chunk(2)
    try:
        small = d.forward_rays(*args, umu=_t(umu), phi=_t(phi)).cpu().numpy()
    finally:
        ctx.set_chunk(0)
    ref = _oracle_rays(prop, bc, kw, nstr, umu, phi, utau)
    err = _col_err(small, ref)
    print("70 rays, chunk 2", err)
    assert margin(err) < TOL, err
    assert np.array_equal(small, auto)


# --- 4 ---------------------------------------------------------------------------
def test_team_fallback_many_rays():
    """nstr 18 with 110 rays, more than a layer record holds (109): shared rays leave
    the team user kernels for the one-lane kernels, as the grid path does"""
    rng = np.random.default_rng(8400)
    nstr, nwave, ncol, nlyr, nray = 18, 1, 2, 4, 110
    prop, bc, kw = _random_case(rng, nwave, ncol, nlyr, nstr, False)
    total = prop[..., 0].sum(axis=-1).min()
    utau = [0.0, 0.37 * total, total]
    umu, phi = _random_rays(rng, 1, nray)
    d = _disort(nstr, nlyr, nwave, ncol, flags="usrtau,lamber,quiet", utau=utau)
    rad = d.forward_rays(_t(prop), _dev(bc), umu=_t(umu[0]), phi=_t(phi[0])).cpu().numpy()
    ref = _oracle_rays(prop, bc, kw, nstr, umu, phi, utau)
    err = _col_err(rad, ref)
    print("110 shared rays, nstr 18", err)
    assert margin(err) < TOL, err


# --- 5 ---------------------------------------------------------------------------
@pytest.mark.parametrize("nstr", [8, 24])
def test_tms_ims_along_rays_vs_oracle(nstr):
    """intensity_correction + old_intensity_correction on forward-peaked HG layers with
    48 moments (delta-M truncation active), per-column rays with downward directions
    (the IMS term): the corrected radiances vs the oracle's"""
    rng = np.random.default_rng(8500 + nstr)
    nwave, ncol, nlyr, nmom, nray = 2, 2, 5, 48, 6
    prop = np.zeros((nwave, ncol, nlyr, 2 + nmom))
    prop[..., 0] = 10.0 ** rng.uniform(-3, 0.5, (nwave, ncol, nlyr))
    prop[..., 1] = rng.uniform(0.3, 0.99, (nwave, ncol, nlyr))
    g = rng.uniform(0.6, 0.85, (nwave, ncol, nlyr))
    for l in range(nmom):
        prop[..., 2 + l] = g ** (l + 1)
    bc = {"fbeam": np.ones((nwave, ncol)), "umu0": rng.uniform(0.2, 1, (nwave, ncol)),
          "phi0": rng.uniform(0, 360, (nwave, ncol)), "albedo": rng.uniform(0, 1, (nwave, ncol))}
    total = prop[..., 0].sum(axis=-1).min()
    utau = [0.0, 0.5 * total, total]
    umu, phi = _random_rays(rng, ncol, nray)
    assert (umu < 0).sum(axis=1).min() >= 1
    d = _disort(nstr, nlyr, nwave, ncol, flags="usrtau,lamber" + CORINT, utau=utau, nmom=nmom)
    rad = d.forward_rays(_t(prop), _dev(bc), umu=_t(umu), phi=_t(phi)).cpu().numpy()
    ref = _oracle_rays(prop, bc, {}, nstr, umu, phi, utau, corint=True, nmom=nmom)
    ref0 = _oracle_rays(prop, bc, {}, nstr, umu, phi, utau, nmom=nmom)
    err = _col_err(rad, ref)
    print("TMS + IMS along rays", nstr, err)
    assert margin(err) < TOL, err
    assert _col_err(ref, ref0) > 1e-3  # the correction is not a no-op here


# --- 6 ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["1a", "1b", "1d"])
def test_disotest1_rays(case):
    """DISOTEST-1's published uu along the rays (umu_i, 0 deg): the bound of
    tests/test_gpu_radiance.py::test_disotest1_radiances"""
    g = disotest()
    c = g["cases"][case]
    d = _disort(16, 1, 1, 1, flags="usrtau,lamber,quiet" + CORINT, utau=[0.0, c["tau"]])
    prop = torch.zeros((1, 1, 1, 18), dtype=torch.float64, device=DEV)
    prop[..., 0] = d.ds().utau[1]
    prop[..., 1] = c["ssalb"]
    bc = {"umu0": torch.full((1, 1), 0.1, dtype=torch.float64, device=DEV)}
    bc["fbeam"] = math.pi / bc["umu0"]
    umu = _t(g["common"]["umu"])
    rad = d.forward_rays(prop, bc, umu=umu, phi=torch.zeros_like(umu)).cpu().numpy()
    exp = np.asarray(c["uu"])
    assert rad.shape == (1, 1, 2, 6)
    assert np.all(np.abs(rad[0, 0] - exp) <= 5e-6 * np.abs(exp) + 1e-6), (rad[0, 0], exp)


# --- 7 ---------------------------------------------------------------------------
@pytest.mark.parametrize("nstr", [8, 24])
def test_band_sum(nstr):
    """forward_rays_band: within TOL of the numpy sum of oracle radiances; bitwise equal
    to band_rad(forward_rays), across chunk sizes (3 = whole waves; 2 and 4 = chunk
    boundaries inside a wave; automatic) and with the per-wave radiances stored"""
    from pyharp_amd.disort import _context
    from pyharp_amd.spectral import band_rad
    rng = np.random.default_rng(8700 + nstr)
    nwave, ncol, nlyr, nray = 5, 3, 4, 4
    prop, bc, kw = _random_case(rng, nwave, ncol, nlyr, nstr, False)
    total = prop[..., 0].sum(axis=-1).min()
    utau = [0.0, 0.6 * total]
    umu, phi = _random_rays(rng, ncol, nray)
    w = rng.uniform(0.05, 0.4, nwave)
    d = _disort(nstr, nlyr, nwave, ncol, flags="usrtau,lamber,quiet", utau=utau)
    kws = dict(umu=_t(umu), phi=_t(phi))
    args = (_t(prop), _dev(bc))
    rad = d.forward_rays(*args, **kws)
    auto = d.forward_rays_band(*args, weights=_t(w), **kws)
    assert tuple(auto.shape) == (ncol, 2, nray)
    ref = np.tensordot(w, _oracle_rays(prop, bc, kw, nstr, umu, phi, utau), axes=(0, 0))
    err = _col_err(auto.cpu().numpy()[None], ref[None])
    print("band sum", nstr, err)
    assert margin(err) < TOL, err
    assert np.array_equal(auto.cpu().numpy(), band_rad(rad, _t(w)).cpu().numpy())
    ctx = _context(0)
    for chunk in (3, 2, 4):
        ctx.set_chunk(chunk)
        try:
            stored = torch.full((nwave, ncol, 2, nray), -1.0, dtype=torch.float64, device=DEV)
            out = torch.full((ncol, 2, nray), -1.0, dtype=torch.float64, device=DEV)
            got = d.forward_rays_band(*args, weights=_t(w), out=out, rad=stored, **kws)
        finally:
            ctx.set_chunk(0)
        assert got is out
        assert np.array_equal(out.cpu().numpy(), auto.cpu().numpy()), chunk
        assert np.array_equal(stored.cpu().numpy(), rad.cpu().numpy()), chunk


# --- 8 ---------------------------------------------------------------------------
def test_thermal_only_rays_vs_oracle():
    """no beam: only mode 0, planck sources"""
    rng = np.random.default_rng(8800)
    nstr, nwave, ncol, nlyr, nray = 16, 2, 3, 6, 5
    prop, bc, kw = _random_case(rng, nwave, ncol, nlyr, nstr, True, beam=False)
    utau = _utau5(rng, prop)
    umu, phi = _random_rays(rng, ncol, nray)
    d = _disort(nstr, nlyr, nwave, ncol, flags="usrtau,lamber,quiet", utau=utau, planck=True,
                wl=kw["wave_lower"], wu=kw["wave_upper"])
    rad = d.forward_rays(_t(prop), _dev(bc), _temf(kw), umu=_t(umu), phi=_t(phi)).cpu().numpy()
    ref = _oracle_rays(prop, bc, kw, nstr, umu, phi, utau, planck=True)
    err = _col_err(rad, ref)
    print("thermal only", err)
    assert margin(err) < TOL, err


# --- 9 ---------------------------------------------------------------------------
@pytest.mark.parametrize("nstr", [8, 24])
def test_bad_ray_on_the_device(nstr):
    """umu = 0 and umu = 1.5 in column 1: an input error only the device can see,
    answered by HD_STATUS_BAD_INPUT on exactly that column's solves and NaN for exactly
    those rays; every other ray and column is bitwise what a clean run gives"""
    from pyharp_amd import _lib
    rng = np.random.default_rng(8900 + nstr)
    nwave, ncol, nlyr, nray = 2, 3, 4, 5
    prop, bc, kw = _random_case(rng, nwave, ncol, nlyr, nstr, False)
    umu, phi = _random_rays(rng, ncol, nray)
    bad = umu.copy()
    bad[1, 2], bad[1, 4] = 0.0, 1.5
    d = _disort(nstr, nlyr, nwave, ncol, flags="lamber,quiet")
    args = (_t(prop), _dev(bc))
    clean = d.forward_rays(*args, umu=_t(umu), phi=_t(phi)).cpu().numpy()
    assert np.all(np.isfinite(clean))
    with pytest.raises(RuntimeError, match="at least one solve failed"):
        d.forward_rays(*args, umu=_t(bad), phi=_t(phi))
    status = torch.zeros(nwave * ncol, dtype=torch.int32, device=DEV)
    rad = d.forward_rays(*args, umu=_t(bad), phi=_t(phi), status=status).cpu().numpy()
    st = status.cpu().numpy().reshape(nwave, ncol)
    assert np.all(st[:, 1] & _lib.HD_STATUS_BAD_INPUT)
    assert np.all((st[:, [0, 2]] & _lib.HD_STATUS_ERROR_MASK) == 0)
    assert np.all(np.isnan(rad[:, 1, :, [2, 4]]))
    keep = np.ones(rad.shape, bool)
    keep[:, 1, :, [2, 4]] = False
    assert np.array_equal(rad[keep], clean[keep])
    # the band sum carries the same answer
    w = _t(np.full(nwave, 0.5))
    brad = d.forward_rays_band(*args, umu=_t(bad), phi=_t(phi), weights=w,
                               status=status).cpu().numpy()
    assert np.all(np.isnan(brad[1][:, [2, 4]]))
    assert np.isfinite(brad).sum() == brad.size - 2 * (nlyr + 1)


@pytest.mark.parametrize("nstr", [8, 24])
def test_bad_shared_ray_on_the_device(nstr):
    """a bad cosine in a shared (nray,) list -- at nstr 24 through the team user kernels,
    which read the copy with the bad value replaced: every solve is flagged, that ray is
    NaN in every column, the other rays are bitwise those of a clean run"""
    from pyharp_amd import _lib
    rng = np.random.default_rng(8950 + nstr)
    nwave, ncol, nlyr, nray = 2, 3, 4, 5
    prop, bc, kw = _random_case(rng, nwave, ncol, nlyr, nstr, False)
    umu, phi = _random_rays(rng, 1, nray)
    umu, phi = umu[0], phi[0]
    bad = umu.copy()
    bad[3] = float("nan")
    d = _disort(nstr, nlyr, nwave, ncol, flags="lamber,quiet")
    args = (_t(prop), _dev(bc))
    clean = d.forward_rays(*args, umu=_t(umu), phi=_t(phi)).cpu().numpy()
    with pytest.raises(RuntimeError, match="at least one solve failed"):
        d.forward_rays(*args, umu=_t(bad), phi=_t(phi))
    status = torch.zeros(nwave * ncol, dtype=torch.int32, device=DEV)
    rad = d.forward_rays(*args, umu=_t(bad), phi=_t(phi), status=status).cpu().numpy()
    assert np.all(status.cpu().numpy() & _lib.HD_STATUS_BAD_INPUT)
    assert np.all(np.isnan(rad[..., 3]))
    ok = [0, 1, 2, 4]
    assert np.all(np.isfinite(clean)) and np.array_equal(rad[..., ok], clean[..., ok])


# --- 10 --------------------------------------------------------------------------
def test_ray_argument_errors():
    from pyharp_amd import _lib
    from pyharp_amd.disort import _context
    nstr, nwave, ncol, nlyr = 4, 2, 3, 2
    rng = np.random.default_rng(9000)
    prop, bc, _ = _random_case(rng, nwave, ncol, nlyr, nstr, False)
    d = _disort(nstr, nlyr, nwave, ncol, flags="lamber,quiet")
    args = (_t(prop), _dev(bc))
    mu, ph = _t([0.5, -0.5]), _t([0.0, 10.0])
    with pytest.raises(RuntimeError, match="umu must be"):
        d.forward_rays(*args, umu=_t(np.full((2, 2), 0.5)), phi=_t(np.zeros((2, 2))))
    with pytest.raises(RuntimeError, match="umu must be"):
        d.forward_rays(*args, umu=_t(np.full((1, 3, 2), 0.5)), phi=_t(np.zeros((1, 3, 2))))
    with pytest.raises(RuntimeError, match="phi .* must have umu's shape"):
        d.forward_rays(*args, umu=mu, phi=_t([0.0, 10.0, 20.0]))
    with pytest.raises(RuntimeError, match="float64"):
        d.forward_rays(*args, umu=mu.float(), phi=ph.float())
    with pytest.raises(RuntimeError, match="onlyfl"):
        _disort(nstr, nlyr, nwave, ncol, flags="lamber,onlyfl").forward_rays(*args, umu=mu, phi=ph)
    with pytest.raises(RuntimeError, match="weights"):
        d.forward_rays_band(*args, umu=mu, phi=ph, weights=_t(np.ones(nwave + 1)))
    with pytest.raises(RuntimeError, match="out must be"):
        d.forward_rays(*args, umu=mu, phi=ph, out=torch.empty(3, dtype=torch.float64, device=DEV))
    # the C level: neither rad nor brad
    cfg = _lib.HdConfig(nstr=nstr, nmom=nstr, nlyr=nlyr, nprop=2 + nstr,
                        flags=_lib.HD_FLAG_LAMBER | _lib.HD_FLAG_ONLYFL)
    p = _t(prop)
    inp = _lib.HdInputs(nwave=nwave, ncol=ncol, prop=p.data_ptr())
    rays = _lib.HdRays(nray=2, per_column=0, umu=mu.data_ptr(), phi=ph.data_ptr(), ntau=0)
    with pytest.raises(RuntimeError, match="invalid argument.*rad and brad both NULL"):
        _context(0).solve_rays(cfg, inp, rays, None, None, None, None)
    # brad without weights
    out = torch.empty((ncol, nlyr + 1, 2), dtype=torch.float64, device=DEV)
    rays.brad = out.data_ptr()
    with pytest.raises(RuntimeError, match="invalid argument.*brad needs weight"):
        _context(0).solve_rays(cfg, inp, rays, None, None, None, None)


# --- 11 --------------------------------------------------------------------------
def test_cpu_tensor_round_trip():
    rng = np.random.default_rng(9100)
    nstr, nwave, ncol, nlyr, nray = 8, 2, 3, 4, 4
    prop, bc, kw = _random_case(rng, nwave, ncol, nlyr, nstr, True)
    umu, phi = _random_rays(rng, ncol, nray)
    d = _disort(nstr, nlyr, nwave, ncol, flags="lamber,quiet", planck=True,
                wl=kw["wave_lower"], wu=kw["wave_upper"])
    cpu = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64)  # noqa: E731
    bcc = {k: cpu(v) for k, v in bc.items()}
    w = rng.uniform(0.1, 1, nwave)
    on_cpu = d.forward_rays(cpu(prop), bcc, cpu(kw["temf"]), umu=cpu(umu), phi=cpu(phi))
    on_dev = d.forward_rays(_t(prop), _dev(bc), _temf(kw), umu=_t(umu), phi=_t(phi))
    assert on_cpu.device.type == "cpu" and on_dev.device == DEV
    assert np.array_equal(on_cpu.numpy(), on_dev.cpu().numpy())
    b_cpu = d.forward_rays_band(cpu(prop), bcc, cpu(kw["temf"]), umu=cpu(umu), phi=cpu(phi),
                                weights=cpu(w))
    b_dev = d.forward_rays_band(_t(prop), _dev(bc), _temf(kw), umu=_t(umu), phi=_t(phi),
                                weights=_t(w))
    assert b_cpu.device.type == "cpu"
    assert np.array_equal(b_cpu.numpy(), b_dev.cpu().numpy())


def test_flux_along_rays_matches_forward():
    """the optional flux output is the grid call's"""
    rng = np.random.default_rng(9150)
    nstr, nwave, ncol, nlyr = 8, 2, 3, 4
    prop, bc, _ = _random_case(rng, nwave, ncol, nlyr, nstr, False)
    umu, phi = _random_rays(rng, ncol, 3)
    d = _disort(nstr, nlyr, nwave, ncol, flags="lamber,quiet")
    ref = d.forward(_t(prop), _dev(bc)).cpu().numpy()
    flux = torch.empty((nwave, ncol, nlyr + 1, 2), dtype=torch.float64, device=DEV)
    d.forward_rays(_t(prop), _dev(bc), umu=_t(umu), phi=_t(phi), flux=flux)
    assert np.array_equal(flux.cpu().numpy(), ref)


# --- 12 --------------------------------------------------------------------------
def test_cpp_disort_rays():
    """tests/cpp/disort_rays_dropin.cpp: DISOTEST 1a through harp_amd::
    parse_radiation_directions and DisortImpl::forward_rays / forward_rays_band
    (include/harp_amd/disort.hpp); ray r = lu * 6 + iu"""
    exe = os.path.join(ROOT, "tests", "cpp", "disort_rays_dropin")
    if not os.path.exists(exe):
        subprocess.run([os.path.join(ROOT, "tests", "cpp", "build_rays.sh")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    exp = np.asarray(disotest()["cases"]["1a"]["uu"]).reshape(-1)
    for tag in ("ray", "band"):  # ten identical waves with weights 0.1: the band sum = a wave
        got = {int(l.split()[1]): float(l.split()[2]) for l in out if l.startswith(tag + " ")}
        assert len(got) == 12, out
        for r, v in got.items():
            assert abs(v - exp[r]) <= 5e-6 * abs(exp[r]) + 1e-6, (tag, r, v, exp[r])
