"""The pseudo-spherical flux path in the hard regimes, against the arbitrary-precision
reference.

Every column of tests/golden/spher_hard.npz (tests/spher_hard_cases.py: a layer's beam
secant on one of its eigenvalues, of either sign, in the top, a middle and the bottom
layer; mu0 down to 1e-6 over shells from 1 mm to 2 R; secants of -1e8 and -5e12; layers of
tau = 0 at either end; 1 - ssa down to 1e-12; thin thermal layers; nmom != nstr) through
``Disort.forward*(..., zd=)``, judged by oracle/disort_mp.py with zd / radius at 50 digits
through helpers.rel_err / TOL.  No double-precision oracle is consulted: tests/spher_ref.py
is itself wrong by O(1) on the resonance family.  No column is left
out.
"""

import numpy as np
import pytest
import torch

import spher_hard_cases as cases
from flx_ref import IFLUP, IRFLDIR, IRFLDN
from hard_cases import WAVE
from helpers import GOLDEN, TOL, margin, rel_err
from oracle.disort_mp import flux_of_record
from test_gpu_hard import _check_record

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fixture():
    return cases.load(GOLDEN)


def _disort(b, nwave=1):
    from pyharp_amd import Disort, DisortOptions
    op = DisortOptions().flags("lamber,quiet,onlyfl,spher" + (",planck" if b["planck"] else ""))
    op.nwave(nwave).ncol(b["prop"].shape[1]).radius(b["radius"])
    if b["planck"]:
        op.wave_lower([WAVE[0]] * nwave).wave_upper([WAVE[1]] * nwave)
    op.ds().nlyr = b["nlyr"]
    op.ds().nstr = b["nstr"]
    op.ds().nmom = b["nmom"]
    return Disort(op)


def _t(x):
    return None if x is None else torch.as_tensor(x, dtype=torch.float64, device=DEV)


def _dev(b):
    return _t(b["prop"]), {k: _t(v) for k, v in b["bc"].items()}, _t(b["temf"]), _t(b["zd"])


def _status(ncol):
    return torch.zeros(ncol, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("nstr", cases.NSTR)
@pytest.mark.parametrize("family", cases.FAMILIES)
def test_forward_against_mp(fixture, family, nstr):
    from pyharp_amd import _lib
    worst = 0.0
    for b in fixture[family, nstr]:
        d = _disort(b)
        p, bc, t, zd = _dev(b)
        d.forward(p, bc, t, zd=zd)  # the synchronous call: raises on any error status
        st = _status(p.shape[1])
        got = d.forward(p, bc, t, zd=zd, status=st).cpu().numpy()
        s = st.cpu().numpy()
        assert np.all(s & _lib.HD_STATUS_ERROR_MASK == 0), (b["name"], s)
        err = rel_err(got, flux_of_record(b["ref"])).max(axis=(0, 2, 3))
        print(f"  {family} n{nstr} {b['name']}: worst {err.max():.3e} (column {err.argmax()})"
              f"  per column {np.array2string(err, precision=1)}")
        worst = max(worst, err.max())
        if family == "resonance" and b["name"] in ("scat", "negative"):
            # the warning means: a layer of this solve was solved for a secant moved off
            # one of its eigenvalues (include/hdisort.h).  Between 1e-11 and 1e-6 the
            # threshold is the implementation's.
            delta = np.abs(b["delta"])
            flag = (s & _lib.HD_STATUS_RESONANCE) != 0
            assert np.all(flag[delta <= 1e-11]), (delta, flag)
            assert not np.any(flag[delta >= 1e-6]), (delta, flag)
    assert margin(worst) < TOL, worst


@pytest.mark.parametrize("nstr", [8, 32])
@pytest.mark.parametrize("family", ["resonance", "thin_thermal", "low_sun", "conservative"])
def test_forward_flx_against_mp(fixture, family, nstr):
    from pyharp_amd import _lib
    for b in fixture[family, nstr]:
        d = _disort(b)
        p, bc, t, zd = _dev(b)
        st = _status(p.shape[1])
        got = d.forward_flx(p, bc, t, zd=zd, status=st).cpu().numpy()
        assert np.all(st.cpu().numpy() & _lib.HD_STATUS_ERROR_MASK == 0), b["name"]
        print(f"  {family} n{nstr} {b['name']}")
        _check_record(got, b["ref"], b["scale"])
        # rfldir + rfldn and flup are forward's two slots
        f = d.forward(p, bc, t, zd=zd).cpu().numpy()
        assert rel_err(got[..., IFLUP:IFLUP + 1], f[..., 0:1]).max() < 1e-10
        assert rel_err((got[..., IRFLDIR] + got[..., IRFLDN])[..., None],
                       f[..., 1:2]).max() < 1e-10


@pytest.mark.parametrize("nstr", [8, 32])
def test_band_of_a_resonance_batch(fixture, nstr):
    """forward_band over a two-wave copy of the resonance batch is the weighted sum of
    forward, and of the mp reference."""
    from pyharp_amd.spectral import band_flux
    b = dict([x for x in fixture["resonance", nstr] if x["name"] == "scat"][0])
    b["prop"] = np.repeat(b["prop"], 2, axis=0)
    b["bc"] = {k: np.repeat(v, 2, axis=0) for k, v in b["bc"].items()}
    d = _disort(b, nwave=2)
    p, bc, t, zd = _dev(b)
    w = torch.as_tensor([0.7, 1.9], dtype=torch.float64, device=DEV)
    band = d.forward_band(p, bc, t, weights=w, zd=zd).cpu().numpy()
    unf = band_flux(d.forward(p, bc, t, zd=zd), w).cpu().numpy()
    assert np.abs(band - unf).max() <= 1e-12 * np.abs(unf).max()
    err = rel_err(band, 2.6 * flux_of_record(b["ref"])[0]).max()
    print(f"  band vs mp: {err:.3e}")
    assert margin(err) < TOL, err
