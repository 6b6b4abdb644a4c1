"""Pseudo-spherical beam geometry on the device (hd_solve_spher / hd_solve_flx_spher,
``Disort.forward*(..., zd=)`` with the 'spher' flag) against tests/spher_ref.py: parity on
both paths, the overhead-sun and large-radius limits, chunked calls and the fused band
sum, the flux record, status flags and the C++ drop-in."""

import functools
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import spher_ref as S
from helpers import TOL, margin, rel_err
from test_gpu_flx import _check_record

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
WL = [w[0] for w in S.WAVES]
WU = [w[1] for w in S.WAVES]
BAD_INPUT = 0x01


def _t(x):
    return None if x is None else torch.tensor(np.array(x), dtype=torch.float64, device=DEV)


def _bc(bc):
    return {k: _t(v) for k, v in bc.items()}


def _disort(nstr, nlyr, nwave, ncol, *, planck=False, spher=True, radius=S.RADIUS, wl=WL, wu=WU):
    from pyharp_amd import Disort, DisortOptions
    op = DisortOptions().flags("lamber,quiet,onlyfl" + (",planck" if planck else "") +
                               (",spher" if spher else ""))
    op.nwave(nwave).ncol(ncol).radius(radius)
    if planck:
        op.wave_lower(list(map(float, wl))).wave_upper(list(map(float, wu)))
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
def _case(nstr, profile, planck, per_column):
    """The batch of spher_ref.batch_inputs and its reference, computed once."""
    prop, bc, temf, zd = S.batch_inputs(nstr, profile, planck, per_column)
    flux, flx, scale = S.spher_forward(prop, bc, temf, zd=zd, radius=S.RADIUS, nstr=nstr,
                                       planck=planck, wave_lower=WL, wave_upper=WU)
    for a in (prop, temf, zd, flux, flx, scale, *bc.values()):
        if a is not None:
            a.setflags(write=False)
    return prop, bc, temf, zd, flux, flx, scale


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("per_column", [False, True], ids=["shared_zd", "column_zd"])
@pytest.mark.parametrize("planck", [False, True], ids=["beam", "beam_planck"])
@pytest.mark.parametrize("profile", list(S.TAU_PROFILES))
@pytest.mark.parametrize("nstr", [4, 8, 16, 18, 32])
def test_parity_with_reference(nstr, profile, planck, per_column):
    prop, bc, temf, zd, ref, _, _ = _case(nstr, profile, planck, per_column)
    d = _disort(nstr, prop.shape[2], prop.shape[0], prop.shape[1], planck=planck)
    st = torch.zeros(prop.shape[0] * prop.shape[1], dtype=torch.int32, device=DEV)
    flux = d.forward(_t(prop), _bc(bc), _t(temf), zd=_t(zd), status=st).cpu().numpy()
    assert not (st.cpu().numpy() & 0x0F).any()
    err = rel_err(flux, ref)
    print(f"nstr {nstr} {profile} planck={planck} per_column={per_column}: "
          f"max rel err by column {err.max(axis=(0, 2, 3))}")
    assert margin(err) < TOL


# ------------------------------------------------------------------ 2. limits
@pytest.mark.parametrize("nstr", [8, 24])
def test_overhead_sun_equals_plane_parallel(nstr):
    prop, bc, _, zd, _, _, _ = _case(nstr, "uniform", False, False)
    bc = dict(bc, umu0=np.ones_like(bc["umu0"]))
    nwave, ncol, nlyr = prop.shape[:3]
    a = _disort(nstr, nlyr, nwave, ncol).forward(_t(prop), _bc(bc), zd=_t(zd)).cpu().numpy()
    b = _disort(nstr, nlyr, nwave, ncol, spher=False).forward(_t(prop), _bc(bc)).cpu().numpy()
    assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()


@pytest.mark.parametrize("nstr", [8, 24])
def test_large_radius_equals_plane_parallel(nstr):
    prop, bc, _, zd, _, _, _ = _case(nstr, "thin_bottom", False, False)
    bc = dict(bc, umu0=np.broadcast_to(np.array([1.0, 0.7, 0.4, 0.2]), bc["umu0"].shape).copy())
    nwave, ncol, nlyr = prop.shape[:3]
    radius = 1e12 * zd[-1]
    g = S.geometric_factors(zd, radius, 0.2)
    assert np.abs(g[np.triu_indices(nlyr)] * 0.2 - 1.0).max() < 1e-10
    a = _disort(nstr, nlyr, nwave, ncol, radius=radius).forward(_t(prop), _bc(bc), zd=_t(zd))
    b = _disort(nstr, nlyr, nwave, ncol, spher=False).forward(_t(prop), _bc(bc))
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert np.abs(a - b).max() <= 1e-8 * np.abs(b).max()


# ------------------------------------------------------------------ 3. chunks, band sum
@pytest.mark.parametrize("nstr,planck", [(8, False), (16, True), (18, False), (32, True)])
def test_chunks_and_band(nstr, planck):
    from pyharp_amd.spectral import band_flux
    prop, bc, temf, zd, _, _, _ = _case(nstr, "thin_bottom", planck, True)
    nwave, ncol, nlyr = prop.shape[:3]
    d = _disort(nstr, nlyr, nwave, ncol, planck=planck)
    args = (_t(prop), _bc(bc), _t(temf))
    z = _t(zd)
    one = d.forward(*args, zd=z)
    w = _t([0.7, 0.4])
    bunf = band_flux(one, w).cpu().numpy()
    scale = np.abs(bunf).max()
    for chunk in (3, 5):  # chunks that cut waves (ncol 4)
        cut = _with_chunk(chunk, lambda: d.forward(*args, zd=z))
        if nstr <= 16:
            assert torch.equal(cut, one)
        else:
            assert (cut - one).abs().max().item() <= 1e-12 * one.abs().max().item()
        band = _with_chunk(chunk, lambda: d.forward_band(*args, weights=w, zd=z)).cpu().numpy()
        assert np.abs(band - bunf).max() <= 1e-12 * scale
    band = d.forward_band(*args, weights=w, zd=z).cpu().numpy()
    assert np.abs(band - bunf).max() <= 1e-12 * scale


# ------------------------------------------------------------------ 4. flux record
@pytest.mark.parametrize("nstr,planck", [(8, False), (16, True), (20, True)])
def test_flux_record(nstr, planck):
    prop, bc, temf, zd, _, ref, scale = _case(nstr, "thin_bottom", planck, False)
    nwave, ncol, nlyr = prop.shape[:3]
    d = _disort(nstr, nlyr, nwave, ncol, planck=planck)
    args = (_t(prop), _bc(bc), _t(temf))
    flx = d.forward_flx(*args, zd=_t(zd)).cpu().numpy()
    flux = d.forward(*args, zd=_t(zd)).cpu().numpy()
    # closed forms of the two beam terms
    f0, mu0 = bc["fbeam"], bc["umu0"]
    for w in range(nwave):
        for c in range(ncol):
            p = prop[w, c]
            ssa = np.where(p[:, 1] == 1.0, 1.0 - np.sqrt(10 * np.finfo(float).eps), p[:, 1])
            dtp = (1.0 - ssa * p[:, 1 + nstr]) * p[:, 0]
            ch = S.chapman(zd, S.RADIUS, mu0[w, c], p[:, 0])
            chp = S.chapman(zd, S.RADIUS, mu0[w, c], dtp)
            dirf = mu0[w, c] * f0[w, c]
            assert np.abs(flx[w, c, :, S.IRFLDIR] - dirf * np.exp(-ch)).max() <= 1e-12 * dirf
            so = f0[w, c] / (4.0 * math.pi)
            assert np.abs(flx[w, c, :, S.IUAVGSO] - so * np.exp(-chp)).max() <= 1e-12 * so
    fs = np.abs(flux).max(axis=(2, 3), keepdims=True)[..., 0]
    assert (np.abs(flx[..., S.IFLUP] - flux[..., 0]) <= 1e-13 * fs).all()
    assert (np.abs(flx[..., S.IRFLDIR] + flx[..., S.IRFLDN] - flux[..., 1]) <= 1e-13 * fs).all()
    # all eight components, each on its own scale, dfdt by the magnitude it is a
    # difference of: the plane-parallel record's check
    _check_record(flx, ref, scale)


# ------------------------------------------------------------------ 5. status
@pytest.mark.parametrize("nstr", [8, 20])
@pytest.mark.parametrize("bad", ["flat", "nan"])
def test_bad_zd_flags_its_column(nstr, bad):
    prop, bc, _, zd, _, _, _ = _case(nstr, "uniform", False, True)
    nwave, ncol, nlyr = prop.shape[:3]
    d = _disort(nstr, nlyr, nwave, ncol)
    clean = d.forward(_t(prop), _bc(bc), zd=_t(zd))
    z = np.array(zd)
    z[2, 3] = z[2, 2] if bad == "flat" else np.nan
    st = torch.zeros(nwave * ncol, dtype=torch.int32, device=DEV)
    got = d.forward(_t(prop), _bc(bc), zd=_t(z), status=st)
    st = st.cpu().numpy().reshape(nwave, ncol)
    assert ((st & BAD_INPUT) != 0).tolist() == [[False, False, True, False]] * nwave
    keep = [0, 1, 3]
    assert torch.equal(got[:, keep], clean[:, keep])
    # the flagged column ran with the beam off: nothing but zeros without another source
    assert (got[:, 2] == 0).all()


def test_sun_on_the_horizon_stays_bad_input():
    prop, bc, _, zd, _, _, _ = _case(8, "uniform", False, False)
    nwave, ncol, nlyr = prop.shape[:3]
    mu = np.array(bc["umu0"])
    mu[:, 1] = 0.0
    st = torch.zeros(nwave * ncol, dtype=torch.int32, device=DEV)
    _disort(8, nlyr, nwave, ncol).forward(_t(prop), _bc(dict(bc, umu0=mu)), zd=_t(zd), status=st)
    st = st.cpu().numpy().reshape(nwave, ncol)
    assert ((st & BAD_INPUT) != 0).tolist() == [[False, True, False, False]] * nwave


def test_host_side_errors():
    from pyharp_amd import _lib
    from pyharp_amd.disort import _context
    d = _disort(8, 5, 2, 4)
    prop, bc, _, zd, _, _, _ = _case(8, "uniform", False, False)
    cfg, inp, keep = d._stage(_t(prop), _bc(bc), None, DEV)
    out = torch.empty((2, 4, 6, 2), dtype=torch.float64, device=DEV)
    z = _t(zd)
    for radius, zp in ((0.0, z.data_ptr()), (float("nan"), z.data_ptr()), (S.RADIUS, None)):
        sph = _lib.HdSphere(radius=radius, zd=zp, per_column=0)
        with pytest.raises(RuntimeError, match="invalid argument"):
            _context(0).solve_spher(cfg, inp, sph, None, out.data_ptr(), None, None)
        with pytest.raises(RuntimeError, match="invalid argument"):
            _context(0).solve_flx_spher(cfg, inp, sph, out.data_ptr(), None, None)


# ------------------------------------------------------------------ 6. C++ drop-in
def test_cpp_dropin():
    """harp_amd::DisortImpl::forward with 'spher', options.radius and zd (tests/cpp/
    disort_spher_dropin.cpp, built by tests/cpp/build_spher.sh) against the Python call
    on the same batch."""
    exe = os.path.join(ROOT, "tests", "cpp", "disort_spher_dropin")
    if not os.path.exists(exe):
        subprocess.run([os.path.join(ROOT, "tests", "cpp", "build_spher.sh")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    nwave, ncol, nlyr, nstr = 2, 2, 5, 8
    got = np.full((nwave, ncol, nlyr + 1, 2), np.nan)
    for line in out.strip().splitlines():
        tag, w, c, l, k, val = line.split()
        assert tag == "flux"
        got[int(w), int(c), int(l), int(k)] = float(val)
    prop = np.zeros((nwave, ncol, nlyr, 2 + nstr))
    for w in range(nwave):
        for c in range(ncol):
            for l in range(nlyr):
                prop[w, c, l, 0] = 0.1 + 0.05 * l + 0.02 * w
                prop[w, c, l, 1] = 0.5 + 0.08 * l - 0.1 * c
                prop[w, c, l, 2:] = (0.6 + 0.05 * c) ** np.arange(1, nstr + 1)
    bc = {"fbeam": np.full((nwave, ncol), 1.5),
          "umu0": np.broadcast_to(np.array([0.5, 0.1]), (nwave, ncol)).copy(),
          "albedo": np.full((nwave, ncol), 0.3)}
    zd = 2.0e4 * np.arange(nlyr + 1.0)
    py = _disort(nstr, nlyr, nwave, ncol).forward(_t(prop), _bc(bc), zd=_t(zd)).cpu().numpy()
    # the C++ program fills prop with std::pow, this test with numpy's power: one ulp apart
    assert np.abs(got - py).max() <= 1e-13 * np.abs(py).max()
    ref, _, _ = S.spher_forward(prop, bc, zd=zd, radius=S.RADIUS, nstr=nstr)
    assert margin(rel_err(got, ref)) < TOL
