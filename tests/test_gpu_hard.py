"""The flux solve in the hard regimes, against the arbitrary-precision reference.

Every column of tests/golden/flux_hard.npz (tests/hard_cases.py: backward and two-lobe
phase functions, nmom != nstr, 1 - ssa down to 1e-12, tau from 1e-15 to 1e4 in one column,
a temperature step across a layer of tau down to 1e-15, the beam cosine on a layer
eigenvalue) through Disort.forward, judged by oracle/disort_mp.py at 50 digits with
helpers.rel_err / TOL.  No double-precision oracle is consulted here: on part of these
inputs they are themselves outside TOL.  No column is left out.
"""

import numpy as np
import pytest
import torch

import hard_cases
from flx_ref import IDFDT, IFLUP, IRFLDIR, IRFLDN, NFLX
from helpers import GOLDEN, TOL, margin, rel_err
from oracle.disort_mp import flux_of_record

pytestmark = pytest.mark.gpu

NAMES = ("rfldir", "rfldn", "flup", "dfdt", "uavg", "uavgdn", "uavgup", "uavgso")


@pytest.fixture(scope="module")
def fixture():
    return hard_cases.load(GOLDEN)


def _disort(b, nwave=1):
    from pyharp_amd import Disort, DisortOptions
    op = DisortOptions().flags("lamber,quiet,onlyfl" + (",planck" if b["planck"] else ""))
    op.nwave(nwave).ncol(b["prop"].shape[1])
    if b["planck"]:
        op.wave_lower([hard_cases.WAVE[0]] * nwave).wave_upper([hard_cases.WAVE[1]] * nwave)
    op.ds().nlyr = b["nlyr"]
    op.ds().nstr = b["nstr"]
    op.ds().nmom = b["nmom"]
    return Disort(op)


def _dev(b):
    dev = torch.device("cuda", 0)
    p = torch.as_tensor(b["prop"], dtype=torch.float64, device=dev)
    bc = {k: torch.as_tensor(v, dtype=torch.float64, device=dev) for k, v in b["bc"].items()}
    t = None if b["temf"] is None else torch.as_tensor(b["temf"], dtype=torch.float64,
                                                       device=dev)
    return p, bc, t


def _status(ncol):
    return torch.zeros(ncol, dtype=torch.int32, device=torch.device("cuda", 0))


@pytest.mark.parametrize("nstr", hard_cases.NSTR)
@pytest.mark.parametrize("family", hard_cases.FAMILIES)
def test_forward_against_mp(fixture, family, nstr):
    from pyharp_amd import _lib
    worst = 0.0
    for b in fixture[family, nstr]:
        d = _disort(b)
        p, bc, t = _dev(b)
        d.forward(p, bc, t)  # the synchronous call: raises on any error status
        st = _status(p.shape[1])
        got = d.forward(p, bc, t, status=st).cpu().numpy()
        s = st.cpu().numpy()
        assert np.all(s & _lib.HD_STATUS_ERROR_MASK == 0), (b["name"], s)
        err = rel_err(got, flux_of_record(b["ref"])).max(axis=(0, 2, 3))
        print(f"  {family} n{nstr} {b['name']}: worst {err.max():.3e} (column {err.argmax()})"
              f"  per column {np.array2string(err, precision=1)}")
        worst = max(worst, err.max())
        if family == "resonance" and b["name"] == "scat":
            # the warning means: this solve's beam cosine was moved off an eigenvalue
            # (include/hdisort.h).  Between 1e-11 and 1e-6 the threshold is the
            # implementation's.
            delta = np.abs(np.array(hard_cases.DELTAS))
            flag = (s & _lib.HD_STATUS_RESONANCE) != 0
            assert np.all(flag[delta <= 1e-11]), (delta, flag)
            assert not np.any(flag[delta >= 1e-6]), (delta, flag)
    assert margin(worst) < TOL, worst


def _check_record(got, ref, scale):
    """As tests/test_gpu_flx.py: every component on its own; dfdt by the magnitude it is
    a difference of."""
    for k in range(NFLX):
        if k == IDFDT:
            continue
        err = rel_err(got[..., k:k + 1], ref[..., k:k + 1]).max()
        print(f"    {NAMES[k]}: max rel err {err:.3e}")
        assert margin(err) < TOL, (NAMES[k], err)
    d = np.abs(got[..., IDFDT] - ref[..., IDFDT])
    zero = scale == 0.0
    assert np.all(got[..., IDFDT][zero] == 0.0)
    frac = (d[~zero] / scale[~zero]).max() if np.any(~zero) else 0.0
    print(f"    dfdt: max |d| / ((1-ssa) 4 pi max(uavg, B)) {frac:.3e}")
    assert margin(frac) <= TOL, frac


@pytest.mark.parametrize("nstr", [8, 32])
@pytest.mark.parametrize("family", ["conservative", "thin_thermal", "resonance"])
def test_forward_flx_against_mp(fixture, family, nstr):
    from pyharp_amd import _lib
    for b in fixture[family, nstr]:
        d = _disort(b)
        p, bc, t = _dev(b)
        st = _status(p.shape[1])
        got = d.forward_flx(p, bc, t, status=st).cpu().numpy()
        assert np.all(st.cpu().numpy() & _lib.HD_STATUS_ERROR_MASK == 0), b["name"]
        print(f"  {family} n{nstr} {b['name']}")
        _check_record(got, b["ref"], b["scale"])
        # rfldir + rfldn and flup are forward's two slots
        f = d.forward(p, bc, t).cpu().numpy()
        assert rel_err(got[..., IFLUP:IFLUP + 1], f[..., 0:1]).max() < 1e-10
        assert rel_err((got[..., IRFLDIR] + got[..., IRFLDN])[..., None],
                       f[..., 1:2]).max() < 1e-10


@pytest.mark.parametrize("nstr", [8, 32])
def test_band_of_a_resonance_batch(fixture, nstr):
    """forward_band over a two-wave copy of the resonance batch is the weighted sum of
    forward (as tests/test_gpu_band.py checks the fused sum), and of the mp reference."""
    from pyharp_amd.spectral import band_flux
    b = dict([x for x in fixture["resonance", nstr] if x["name"] == "scat"][0])
    b["prop"] = np.repeat(b["prop"], 2, axis=0)
    b["bc"] = {k: np.repeat(v, 2, axis=0) for k, v in b["bc"].items()}
    d = _disort(b, nwave=2)
    p, bc, t = _dev(b)
    w = torch.as_tensor([0.7, 1.9], dtype=torch.float64, device=p.device)
    band = d.forward_band(p, bc, t, weights=w).cpu().numpy()
    unf = band_flux(d.forward(p, bc, t), w).cpu().numpy()
    assert np.abs(band - unf).max() <= 1e-12 * np.abs(unf).max()
    err = rel_err(band, 2.6 * flux_of_record(b["ref"])[0]).max()
    print(f"  band vs mp: {err:.3e}")
    assert margin(err) < TOL, err
