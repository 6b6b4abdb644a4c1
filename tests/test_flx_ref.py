"""The CPU reference of the full flux record (tests/flx_ref.py) against DISOTEST problem 1.

Pins the helper that tests/test_gpu_flx.py compares hd_solve_flx with: the published
dfdt / uavg of the DISORT test driver (six printed digits, 5e-6 relative -- the
fixture's own precision), and the quadrature identity with the fixture's fluxes.
"""

import math
import os

import numpy as np
import pytest

import flx_ref
from flx_ref import IDFDT, IFLUP, IRFLDIR, IRFLDN, IUAVG, flx_ref_column
from helpers import GOLDEN, disotest

PRINTED = 5e-6  # six printed digits


def _case(name):
    d = disotest()
    c, k = d["common"], d["cases"][name]
    nstr = c["nstr"]
    pmom = np.zeros((1, nstr + 1))
    pmom[:, 0] = 1.0  # isotropic
    flx, scale, quad = flx_ref_column([k["tau"]], [k["ssalb"]], pmom, nstr, umu0=c["umu0"],
                                      fbeam=c["fbeam_times_umu0"] / c["umu0"],
                                      albedo=c["albedo"])
    return k, flx, scale, quad


def test_1a_dfdt_and_uavg():
    _, flx, _, _ = _case("1a")
    np.testing.assert_allclose(flx[:, IDFDT], [25.4067, 18.6531], rtol=PRINTED)
    np.testing.assert_allclose(flx[:, IUAVG], [2.52725, 1.85546], rtol=PRINTED)


def test_1d_top_dfdt():
    _, flx, _, _ = _case("1d")
    assert flx[0, IDFDT] == pytest.approx(25.7766, rel=PRINTED)


def test_1b_conservative_dfdt_is_exactly_zero():
    _, flx, scale, _ = _case("1b")  # ssa_in = 1: (1 - ssa_in) = 0
    assert np.all(flx[:, IDFDT] == 0.0)
    assert np.all(scale == 0.0)


@pytest.mark.parametrize("name", ["1a", "1b", "1d"])
def test_fluxes_match_fixture_and_quadrature_identity(name):
    k, flx, _, own = _case(name)
    # the helper's flup is 2 pi sum w mu I+ at the nodes: the fixture's flup
    for comp, key in ((IRFLDIR, "rfldir"), (IRFLDN, "rfldn"), (IFLUP, "flup")):
        np.testing.assert_allclose(flx[:, comp], k[key], rtol=PRINTED, atol=1e-6)
    # ... and the oracle's own fluxes far below the printed digits.  Not for 1b: its
    # dithered ssa = 1 - 4.7e-8 amplifies rounding by 1 / (1 - ssa) = 2e7 in the two
    # routes' different arithmetic (observed 1e-8)
    if k["ssalb"] < 1.0:
        np.testing.assert_allclose(flx[:, IFLUP], own[:, 0], rtol=1e-10, atol=1e-13)
        np.testing.assert_allclose(flx[:, IRFLDIR] + flx[:, IRFLDN], own[:, 1], rtol=1e-10,
                                   atol=1e-13)
    assert math.isfinite(float(np.abs(flx).sum()))


@pytest.mark.parametrize("nstr,nlyr,source", [(2, 1, "beam"), (4, 5, "beam_planck"),
                                              (8, 2, "planck"), (8, 5, "fisot"),
                                              (18, 1, "beam_planck")])
def test_stored_parity_cases_are_this_helper(nstr, nlyr, source):
    """tests/golden/flx_parity.npz (tests/golden/make_flx_golden.py) holds the inputs and
    this helper's record for every GPU parity case; a sample is recomputed here."""
    z = np.load(os.path.join(GOLDEN, "flx_parity.npz"))
    key = flx_ref.parity_key(nstr, nlyr, source)
    prop, bc, temf = flx_ref.parity_inputs(nstr, nlyr, source)
    assert np.array_equal(z[key + "/prop"], prop)
    for k, v in bc.items():
        assert np.array_equal(z[key + "/bc_" + k], v), k
    if temf is not None:
        assert np.array_equal(z[key + "/temf"], temf)
    ref, scale = flx_ref.parity_reference(nstr, nlyr, source)
    np.testing.assert_allclose(z[key + "/ref"], ref, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(z[key + "/scale"], scale, rtol=1e-12, atol=1e-300)


def test_every_parity_case_is_stored():
    z = np.load(os.path.join(GOLDEN, "flx_parity.npz"))
    for nstr in flx_ref.PARITY_NSTR:
        for nlyr in flx_ref.PARITY_NLYR:
            for source in flx_ref.PARITY_SOURCES:
                ref = z[flx_ref.parity_key(nstr, nlyr, source) + "/ref"]
                assert ref.shape == (2, 3, nlyr + 1, flx_ref.NFLX) and np.all(np.isfinite(ref))
