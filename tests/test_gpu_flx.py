"""hd_solve_flx / Disort.forward_flx: DISORT's full flux record per level on the GPU.

rfldir, rfldn, flup, dfdt, uavg, uavgdn, uavgup, uavgso (include/hdisort.h HD_FLX_*),
checked against

* the CPU reference tests/flx_ref.py (the NumPy intensity oracle's mode-0 field at the
  quadrature nodes, integrated), stored with its inputs in tests/golden/flx_parity.npz
  (tests/test_flx_ref.py keeps the file and the helper together): every component on its
  own with helpers.rel_err / TOL; dfdt, a difference that vanishes in equilibrium, by
  |d| <= TOL (1 - ssa_in) 4 pi max(uavg_ref, B_lev);
* hd_solve on the same inputs (flup, rfldir + rfldn) at 1e-10 in the same metric: four
  orders under TOL, far above FP64 summation noise (6.5e-16 between two
  summation orders);
* itself across lane / wave / chunk boundaries and a HIP-graph replay, bitwise;
* exact properties of the equations that do not go through the oracle.
"""

import math
import os
import subprocess

import numpy as np
import pytest
import torch

import flx_ref
from flx_ref import (IDFDT, IFLUP, IRFLDIR, IRFLDN, IUAVG, IUAVGDN, IUAVGSO, IUAVGUP, NFLX,
                     PARITY_NLYR, PARITY_NSTR, PARITY_SOURCES, PARITY_WAVES)
from helpers import GOLDEN, TOL, margin, rel_err

pytestmark = pytest.mark.gpu

NAMES = ("rfldir", "rfldn", "flup", "dfdt", "uavg", "uavgdn", "uavgup", "uavgso")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _disort(nstr, nlyr, nwave, ncol, planck=False, wl=None, wu=None, extra="", radius=None):
    from pyharp_amd import Disort, DisortOptions
    op = DisortOptions().flags("lamber,quiet,onlyfl" + (",planck" if planck else "") + extra)
    op.nwave(nwave).ncol(ncol)
    if planck:
        op.wave_lower(list(map(float, wl))).wave_upper(list(map(float, wu)))
    if radius is not None:
        op.radius(radius)
    op.ds().nlyr = nlyr
    op.ds().nstr = nstr
    op.ds().nmom = nstr
    return Disort(op)


def _dev(prop, bc, temf=None):
    dev = torch.device("cuda", 0)
    p = torch.as_tensor(prop, dtype=torch.float64, device=dev)
    b = {k: torch.as_tensor(v, dtype=torch.float64, device=dev) for k, v in bc.items()}
    t = None if temf is None else torch.as_tensor(temf, dtype=torch.float64, device=dev)
    return p, b, t


def _flx(d, prop, bc, temf=None, **kw):
    p, b, t = _dev(prop, bc, temf)
    return d.forward_flx(p, b, t, **kw).cpu().numpy()


def _flux(d, prop, bc, temf=None):
    p, b, t = _dev(prop, bc, temf)
    return d.forward(p, b, t).cpu().numpy()


def _hg_batch(rng, nwave, ncol, nlyr, nstr, g=0.8):
    prop = np.zeros((nwave, ncol, nlyr, 2 + nstr))
    prop[..., 0] = 10.0 ** rng.uniform(-2.0, 0.5, (nwave, ncol, nlyr))
    prop[..., 1] = rng.uniform(0.05, 0.98, (nwave, ncol, nlyr))
    for l in range(nstr):
        prop[..., 2 + l] = g ** (l + 1)
    bc = {"fbeam": rng.uniform(0.5, 2.0, (nwave, ncol)), "umu0": rng.uniform(0.2, 1.0, (nwave, ncol)),
          "albedo": rng.uniform(0.0, 1.0, (nwave, ncol))}
    return prop, bc


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(GOLDEN, "flx_parity.npz"))
    return {k: z[k] for k in z.files}


def _wl_wu():
    return [w[0] for w in PARITY_WAVES], [w[1] for w in PARITY_WAVES]


def _golden_case(golden, nstr, nlyr, source):
    key = flx_ref.parity_key(nstr, nlyr, source) + "/"
    d = {k[len(key):]: v for k, v in golden.items() if k.startswith(key)}
    bc = {k[3:]: v for k, v in d.items() if k.startswith("bc_")}
    return d["prop"], bc, d.get("temf"), d["ref"], d["scale"]


def _check_record(got, ref, scale):
    """Every component against the reference on its own (the components have different
    units); dfdt by the magnitude it is a difference of."""
    for k in range(NFLX):
        if k == IDFDT:
            continue
        err = rel_err(got[..., k:k + 1], ref[..., k:k + 1]).max()
        print(f"  {NAMES[k]}: max rel err {err:.3e}")
        assert margin(err) < TOL, (NAMES[k], err)
    d = np.abs(got[..., IDFDT] - ref[..., IDFDT])
    zero = scale == 0.0
    assert np.all(got[..., IDFDT][zero] == 0.0)
    frac = (d[~zero] / scale[~zero]).max() if np.any(~zero) else 0.0
    print(f"  dfdt: max |d| / ((1-ssa) 4 pi max(uavg, B)) {frac:.3e}")
    assert margin(frac) <= TOL, frac


# --------------------------------------------------------------------------- #
# parity with the CPU reference
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("source", PARITY_SOURCES)
@pytest.mark.parametrize("nlyr", PARITY_NLYR)
@pytest.mark.parametrize("nstr", PARITY_NSTR)
def test_parity_with_reference(golden, nstr, nlyr, source):
    """Inputs and the reference record of every case: tests/golden/flx_parity.npz
    (tests/flx_ref.py parity_inputs says how the special layers are laid out and why)."""
    prop, bc, temf, ref, scale = _golden_case(golden, nstr, nlyr, source)
    planck = temf is not None
    wl, wu = _wl_wu()
    d = _disort(nstr, nlyr, 2, 3, planck=planck, wl=wl, wu=wu)
    got = _flx(d, prop, bc, temf)
    assert got.shape == (2, 3, nlyr + 1, NFLX)
    _check_record(got, ref, scale)
    if "beam" in source:  # delta-M is active: the scaled direct term is another number
        so_dir = got[..., IUAVGSO] * 4.0 * math.pi * bc["umu0"][..., None]
        assert np.abs(so_dir[:, :, 0] / got[:, :, 0, IRFLDIR] - 1.0).max() > 1e-6


# --------------------------------------------------------------------------- #
# consistency with hd_solve
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("source", ["beam", "beam_planck"])
@pytest.mark.parametrize("nstr", PARITY_NSTR)
def test_consistent_with_hd_solve(golden, nstr, source):
    prop, bc, temf, _, _ = _golden_case(golden, nstr, 5, source)
    wl, wu = _wl_wu()
    d = _disort(nstr, 5, 2, 3, planck=temf is not None, wl=wl, wu=wu)
    flx = _flx(d, prop, bc, temf)
    f = _flux(d, prop, bc, temf)
    up = rel_err(flx[..., IFLUP:IFLUP + 1], f[..., 0:1]).max()
    dn = rel_err((flx[..., IRFLDIR] + flx[..., IRFLDN])[..., None], f[..., 1:2]).max()
    print(f"  flup vs slot 0: {up:.3e}; rfldir + rfldn vs slot 1: {dn:.3e}")
    assert margin(up) < 1e-10 and margin(dn) < 1e-10, (up, dn)
    np.testing.assert_allclose(flx[..., IUAVG], flx[..., IUAVGUP] + flx[..., IUAVGDN] +
                               flx[..., IUAVGSO], rtol=1e-15, atol=0.0)


@pytest.mark.parametrize("chunk", [0, 23])
@pytest.mark.parametrize("nstr", [18, 32])
def test_team_flup_bitwise_with_hd_solve(nstr, chunk):
    """Team path: hd_solve's sweep (two waves per SIMD, its operands parked in LDS and
    re-read from the records) and the one-wave sweep body of hd_solve_flx do the same
    arithmetic in the same order, so the upward fluxes agree to the bit -- with a beam and
    Planck emission, in one chunk and in chunks of 23 of the 93 solves."""
    from pyharp_amd.disort import _context
    nwave, ncol, nlyr = 3, 31, 14
    rng = np.random.default_rng(1800 + nstr)
    prop, bc = _hg_batch(rng, nwave, ncol, nlyr, nstr)
    bc.update(btemp=np.full((nwave, ncol), 290.0), ttemp=np.full((nwave, ncol), 160.0),
              temis=rng.uniform(0.1, 0.9, (nwave, ncol)))
    temf = np.linspace(285.0, 190.0, nlyr + 1)[None, :] + rng.uniform(-5, 5, (ncol, nlyr + 1))
    wl, wu = [200.0, 600.0, 1000.0], [400.0, 900.0, 1100.0]
    d = _disort(nstr, nlyr, nwave, ncol, planck=True, wl=wl, wu=wu)
    ctx = _context(0)
    ctx.set_chunk(chunk)
    try:
        flx = _flx(d, prop, bc, temf)
        f = _flux(d, prop, bc, temf)
    finally:
        ctx.set_chunk(0)
    assert np.all(np.isfinite(f)) and np.all(f[..., 0] > 0.0)
    assert np.array_equal(flx[..., IFLUP], f[..., 0])


@pytest.mark.parametrize("nstr", [18, 32])
def test_team_large_chunk_bitwise_with_small_chunks(nstr):
    """Team path: a chunk of at least 4 096 solves takes the nontemporal instantiations of
    the layer kernel and of hd_solve's sweep, a smaller one the plain ones; where a record
    is kept between the two kernels does not change a bit of it.  4 099 solves of two layers
    (a last team of three) with a beam and Planck emission, in one chunk and in chunks of
    1 024: fluxes and status equal bit for bit."""
    from pyharp_amd import _lib
    from pyharp_amd.disort import _context
    nwave, ncol, nlyr = 1, 4099, 2
    assert _lib.chunk_solves(nstr, nlyr, nwave * ncol, planck=True) == nwave * ncol
    rng = np.random.default_rng(4099 + nstr)
    prop, bc = _hg_batch(rng, nwave, ncol, nlyr, nstr)
    bc.update(btemp=np.full((nwave, ncol), 290.0), ttemp=np.full((nwave, ncol), 160.0),
              temis=rng.uniform(0.1, 0.9, (nwave, ncol)))
    temf = np.linspace(285.0, 190.0, nlyr + 1)[None, :] + rng.uniform(-5, 5, (ncol, nlyr + 1))
    d = _disort(nstr, nlyr, nwave, ncol, planck=True, wl=[200.0], wu=[400.0])
    p, b, t = _dev(prop, bc, temf)
    ctx = _context(0)
    out = []
    for chunk in (0, 1024):
        st = torch.zeros(nwave * ncol, dtype=torch.int32, device=p.device)
        ctx.set_chunk(chunk)
        try:
            out.append((d.forward(p, b, t, status=st).cpu().numpy(), st.cpu().numpy()))
        finally:
            ctx.set_chunk(0)
    (f, st), (f2, st2) = out
    assert np.all(np.isfinite(f)) and np.all(f[..., 0] > 0.0)
    assert np.array_equal(f, f2)
    assert np.array_equal(st, st2)


@pytest.mark.parametrize("call", ["forward", "forward_spher", "forward_flx_spher"])
@pytest.mark.parametrize("nstr", [6, 16])
def test_reg_large_chunk_bitwise_with_small_chunks(nstr, call):
    """The same on the one-lane path (nstr 6 and 16: at 4 and 8 a chunk this small runs the
    quad sweep): one chunk of 4 099 solves takes the nontemporal instantiations of
    hd_layer_kernel / hd_sweep_kernel (forward), of hd_layer_spher_kernel /
    hd_sweep_spher_kernel (forward with zd) and of the latter's FLX form with the flx
    back-substitution (forward_flx with zd); chunks of 1 024 take the plain ones."""
    from pyharp_amd import _lib
    from pyharp_amd.disort import _context
    nwave, ncol, nlyr = 1, 4099, 2
    assert _lib.chunk_solves(nstr, nlyr, nwave * ncol, planck=True) == nwave * ncol
    rng = np.random.default_rng(4099 + nstr)
    prop, bc = _hg_batch(rng, nwave, ncol, nlyr, nstr)
    bc.update(btemp=np.full((nwave, ncol), 290.0), ttemp=np.full((nwave, ncol), 160.0),
              temis=rng.uniform(0.1, 0.9, (nwave, ncol)))
    temf = np.linspace(285.0, 190.0, nlyr + 1)[None, :] + rng.uniform(-5, 5, (ncol, nlyr + 1))
    spher = call != "forward"
    d = _disort(nstr, nlyr, nwave, ncol, planck=True, wl=[200.0], wu=[400.0],
                extra=",spher" if spher else "", radius=3.39e6 if spher else None)
    p, b, t = _dev(prop, bc, temf)
    kw = {}
    if spher:
        kw["zd"] = torch.as_tensor(np.linspace(0.0, 20.0e3, nlyr + 1), dtype=torch.float64,
                                   device=p.device)
    fwd = d.forward_flx if call == "forward_flx_spher" else d.forward
    ctx = _context(0)
    out = []
    for chunk in (0, 1024):
        st = torch.zeros(nwave * ncol, dtype=torch.int32, device=p.device)
        ctx.set_chunk(chunk)
        try:
            out.append((fwd(p, b, t, status=st, **kw).cpu().numpy(), st.cpu().numpy()))
        finally:
            ctx.set_chunk(0)
    (f, st), (f2, st2) = out
    assert np.all(np.isfinite(f)) and np.all(f[..., IFLUP if f.shape[-1] == NFLX else 0] > 0.0)
    assert np.array_equal(f, f2)
    assert np.array_equal(st, st2)


# --------------------------------------------------------------------------- #
# lane / wave / chunk edges: a solve's record does not depend on where it ran
# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def edge_batches():
    """130 distinct solves per path (nstr 8: one lane per solve; nstr 24: four 16-lane
    teams per wave) and their one-chunk records."""
    out = {}
    for nstr in (8, 24):
        rng = np.random.default_rng(900 + nstr)
        prop, bc = _hg_batch(rng, 1, 130, 6, nstr)
        d = _disort(nstr, 6, 1, 130)
        out[nstr] = (prop, bc, _flx(d, prop, bc))
    return out


@pytest.mark.parametrize("nstr,nsolve", [(8, 1), (8, 65), (24, 5)])
def test_partial_waves(edge_batches, nstr, nsolve):
    prop, bc, full = edge_batches[nstr]
    assert np.all(np.isfinite(full))
    d = _disort(nstr, 6, 1, nsolve)
    got = _flx(d, prop[:, :nsolve], {k: v[:, :nsolve] for k, v in bc.items()})
    assert np.array_equal(got, full[:, :nsolve])


@pytest.mark.parametrize("nstr", [8, 24])
def test_three_chunks_bitwise(edge_batches, nstr):
    """set_chunk(48) with 130 solves: chunks of 48 + 48 + 34 across the three streams."""
    from pyharp_amd.disort import _context
    prop, bc, full = edge_batches[nstr]
    d = _disort(nstr, 6, 1, 130)
    ctx = _context(0)
    ctx.set_chunk(48)
    try:
        got = _flx(d, prop, bc)
    finally:
        ctx.set_chunk(0)
    assert np.array_equal(got, full)


def test_six_chunks_run_the_capped_backsub_bitwise(edge_batches):
    """set_chunk(24) with 130 solves at nstr 8: six chunks, so all but the last take
    hd_backsub_flx_kernel (the occupancy-capped back-substitution beside the next chunk's
    layer kernel; up to three chunks all take the tail kernel).  Same bits as one chunk:
    a solve's record does not depend on which back-substitution ran it."""
    from pyharp_amd.disort import _context
    prop, bc, full = edge_batches[8]
    d = _disort(8, 6, 1, 130)
    ctx = _context(0)
    ctx.set_chunk(24)
    try:
        got = _flx(d, prop, bc)
    finally:
        ctx.set_chunk(0)
    assert np.array_equal(got, full)


def test_nontemporal_chunk_bitwise():
    """4 200 solves at nstr 4: one chunk of >= 4 096 solves runs the nontemporal-record
    instantiations (sweep, tail back-substitution); in six chunks of 700 the plain ones
    with the capped back-substitution.  Same bits, and hd_solve's fluxes at 1e-10."""
    from pyharp_amd.disort import _context
    nstr, nlyr, n = 4, 3, 4200
    rng = np.random.default_rng(905)
    prop, bc = _hg_batch(rng, 1, n, nlyr, nstr)
    d = _disort(nstr, nlyr, 1, n)
    one = _flx(d, prop, bc)
    ctx = _context(0)
    ctx.set_chunk(700)
    try:
        six = _flx(d, prop, bc)
    finally:
        ctx.set_chunk(0)
    assert np.all(np.isfinite(one)) and np.array_equal(one, six)
    f = _flux(d, prop, bc)
    assert rel_err(one[..., IFLUP:IFLUP + 1], f[..., 0:1]).max() < 1e-10
    assert rel_err((one[..., IRFLDIR] + one[..., IRFLDN])[..., None], f[..., 1:2]).max() < 1e-10


# --------------------------------------------------------------------------- #
# exact physics, independent of the oracle
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("nstr", [8, 24])
def test_solves_left_out_of_the_parity_cases(nstr):
    """The two kinds of solve the parity inputs leave out (tests/flx_ref.py parity_inputs:
    no CPU reference to TOL there), against properties that need none.
    * A beam-lit column of one layer of tau = 1e-6: Beer's law in both depths, the delta-M
      relation between them, a diffuse field of the order tau, and hd_solve's two fluxes.
    * A conservative column (every ssa = 1) over a surface of albedo 1, beam-lit: nothing
      absorbs but the dither (ssa = 1 - 4.712e-8), so the net flux at a level is what the
      layers below it absorb: at most 4.712e-8 x 4 pi max(uavg) x total tau (+ 5 %: uavg
      is known at the levels only and may peak inside a layer) -- dfdt is an exact zero and the record is finite."""
    rng = np.random.default_rng(380 + nstr)
    nwave, ncol, nlyr = 2, 3, 1
    prop, bc = _hg_batch(rng, nwave, ncol, nlyr, nstr)
    prop[..., 0] = 1.0e-6
    d = _disort(nstr, nlyr, nwave, ncol)
    flx, f = _flx(d, prop, bc), _flux(d, prop, bc)
    mu0, fb = bc["umu0"][..., None], bc["fbeam"][..., None]
    tau = np.concatenate([prop[..., 0], np.zeros((nwave, ncol, 1))], axis=2)  # level 0 = surface
    fdm = 0.8 ** nstr
    taup = tau * (1.0 - prop[:, :, :, 1] * fdm)  # one layer: its ssa for both levels
    np.testing.assert_allclose(flx[..., IRFLDIR], mu0 * fb * np.exp(-tau / mu0), rtol=1e-14)
    np.testing.assert_allclose(flx[..., IUAVGSO], fb * np.exp(-taup / mu0) / (4 * math.pi),
                               rtol=1e-14)
    assert np.abs(flx[..., IRFLDN]).max() < 1e-5 * (mu0 * fb).max()
    assert np.abs(flx[..., IUAVGDN]).max() < 1e-4 * fb.max()
    assert rel_err(flx[..., IFLUP:IFLUP + 1], f[..., 0:1]).max() < 1e-10
    assert np.abs(flx[..., IRFLDIR] + flx[..., IRFLDN] - f[..., 1]).max() <= \
        1e-12 * np.abs(f[..., 1]).max()

    nlyr = 3
    prop, bc = _hg_batch(rng, nwave, ncol, nlyr, nstr)
    prop[..., 1] = 1.0
    bc["albedo"] = np.ones((nwave, ncol))
    flx = _flx(_disort(nstr, nlyr, nwave, ncol), prop, bc)
    assert np.all(np.isfinite(flx)) and np.all(flx[..., IDFDT] == 0.0)
    net = flx[..., IFLUP] - flx[..., IRFLDIR] - flx[..., IRFLDN]
    bound = 4.712160915387242e-08 * 4.0 * math.pi * flx[..., IUAVG].max(axis=2) * \
        prop[..., 0].sum(axis=2)
    frac = (np.abs(net).max(axis=2) / bound).max()
    print(f"  conservative over albedo 1: max |net| / dither absorption bound {frac:.3f}")
    assert frac <= 1.05



@pytest.mark.parametrize("nstr", [8, 24])
def test_isothermal_enclosure(nstr):
    """btemp = ttemp = T, temis = 1, uniform temf, albedo 0: I = B(T) in every stream,
    so uavg = B(T), uavgso = 0 and dfdt = 0 (by its bound) at every level."""
    rng = np.random.default_rng(310 + nstr)
    nwave, ncol, nlyr, T = 2, 4, 7, 255.0
    prop, _ = _hg_batch(rng, nwave, ncol, nlyr, nstr)
    prop[0, 1, :, 1] = 0.0
    wl, wu = [20.0, 600.0], [350.0, 640.0]
    bc = {"albedo": np.zeros((nwave, ncol)), "btemp": np.full((nwave, ncol), T),
          "ttemp": np.full((nwave, ncol), T), "temis": np.ones((nwave, ncol))}
    temf = np.full((ncol, nlyr + 1), T)
    d = _disort(nstr, nlyr, nwave, ncol, planck=True, wl=wl, wu=wu)
    flx = _flx(d, prop, bc, temf)
    from oracle.disort_np import plkavg
    for w in range(nwave):
        b = flx[w, :, :, IFLUP].mean() / math.pi  # every stream carries B(T): flup = pi B
        assert abs(b / plkavg(wl[w], wu[w], T) - 1.0) < 2e-6
        assert np.abs(flx[w, :, :, IUAVG] / b - 1.0).max() < 1e-9
        assert np.abs(flx[w, :, :, IFLUP] / (math.pi * b) - 1.0).max() < 1e-9
        assert np.abs(flx[w, :, :, IUAVGUP] / (0.5 * b) - 1.0).max() < 1e-9
        ssa_in = np.concatenate([prop[w, :, :, 1], prop[w, :, -1:, 1]], axis=1)
        bound = TOL * (1.0 - ssa_in) * 4.0 * math.pi * np.maximum(flx[w, :, :, IUAVG], b)
        assert np.all(np.abs(flx[w, :, :, IDFDT]) <= bound)
    assert np.all(flx[..., IUAVGSO] == 0.0) and np.all(flx[..., IRFLDIR] == 0.0)


@pytest.mark.parametrize("nstr", [8, 24])
def test_conservative_and_beamless_zeros(nstr):
    rng = np.random.default_rng(320 + nstr)
    nwave, ncol, nlyr = 2, 3, 4
    prop, bc = _hg_batch(rng, nwave, ncol, nlyr, nstr)
    d = _disort(nstr, nlyr, nwave, ncol)
    cons = prop.copy()
    cons[..., 1] = 1.0  # ssa_in = 1 everywhere: (1 - ssa_in) is an exact zero
    flx = _flx(d, cons, bc)
    assert np.all(np.isfinite(flx)) and np.all(flx[..., IDFDT] == 0.0)
    assert np.all(flx[..., IUAVG] > 0.0)
    nobeam = {"albedo": bc["albedo"], "fisot": np.ones((nwave, ncol))}
    flx = _flx(d, prop, nobeam)
    assert np.all(flx[..., IRFLDIR] == 0.0) and np.all(flx[..., IUAVGSO] == 0.0)
    assert np.all(flx[..., IUAVGDN] > 0.0)


@pytest.mark.parametrize("nstr", [8, 24])
def test_pure_absorption_beam(nstr):
    rng = np.random.default_rng(330 + nstr)
    nwave, ncol, nlyr = 2, 3, 5
    prop, bc = _hg_batch(rng, nwave, ncol, nlyr, nstr)
    prop[..., 1] = 0.0
    bc["albedo"] = np.zeros((nwave, ncol))
    d = _disort(nstr, nlyr, nwave, ncol)
    flx = _flx(d, prop, bc)
    lhs = flx[..., IUAVGSO] * 4.0 * math.pi * bc["umu0"][..., None]
    assert np.abs(lhs - flx[..., IRFLDIR]).max() <= 1e-14 * np.abs(flx[..., IRFLDIR]).max()
    top = flx[:, :, -1, IUAVGSO]
    assert np.abs(flx[..., IUAVGDN]).max() <= 1e-14 * top.max()
    assert np.abs(flx[..., IUAVGUP]).max() <= 1e-14 * top.max()
    # the record is Beer's law: the divergence of the net flux is 4 pi uavgso
    np.testing.assert_allclose(flx[..., IDFDT], 4.0 * math.pi * flx[..., IUAVG], rtol=1e-14)


def _divergence_error(nlyr):
    """max over layers of | d(flup - rfldir - rfldn)/dtau - mean of the two levels' dfdt |
    for a homogeneous beam-lit slab of total tau 0.5 in nlyr equal layers.  (The largest
    eigenvalue at nstr 8 is k = 15: its boundary layers need k dtau << 1 for the
    second-order regime -- 0.19 at 40 layers here; a slab of tau 2, k dtau = 0.75, gives
    3.45x in the CPU reference too.)"""
    nstr, tau_tot = 8, 0.5
    prop = np.zeros((1, 1, nlyr, 2 + nstr))
    prop[..., 0] = tau_tot / nlyr
    prop[..., 1] = 0.6
    for l in range(nstr):
        prop[..., 2 + l] = 0.8 ** (l + 1)
    bc = {"fbeam": np.full((1, 1), 1.3), "umu0": np.full((1, 1), 0.5),
          "albedo": np.full((1, 1), 0.2)}
    flx = _flx(_disort(nstr, nlyr, 1, 1), prop, bc)[0, 0]
    net = flx[:, IFLUP] - flx[:, IRFLDIR] - flx[:, IRFLDN]
    # tau grows downwards, the level index upwards
    cd = (net[:-1] - net[1:]) / (tau_tot / nlyr)
    mean = 0.5 * (flx[:-1, IDFDT] + flx[1:, IDFDT])
    return np.abs(cd - mean).max(), np.abs(mean).max()


def test_dfdt_is_the_flux_divergence():
    """dfdt is exact at the levels, so the centred difference of the net flux over a
    layer agrees with the mean of its two levels' dfdt to second order in dtau: the
    error drops >= 3.5x (4x in the limit) when the 40 layers are halved."""
    e40, m40 = _divergence_error(40)
    e80, _ = _divergence_error(80)
    print(f"  err(40) {e40:.3e}  err(80) {e80:.3e}  ratio {e40 / e80:.3f}  |dfdt| {m40:.3e}")
    assert e40 < 1e-3 * m40
    assert e40 / e80 >= 3.5


# --------------------------------------------------------------------------- #
# status, capture, band sum, bindings
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("nstr", [8, 24])
def test_status_bits(nstr):
    from pyharp_amd import _lib
    rng = np.random.default_rng(340 + nstr)
    nwave, ncol, nlyr = 2, 3, 4
    prop, bc = _hg_batch(rng, nwave, ncol, nlyr, nstr)
    d = _disort(nstr, nlyr, nwave, ncol)
    dev = torch.device("cuda", 0)
    ub = bc["umu0"].copy()
    ub[1, 2] = 1.2  # cdisort's c_chekin error with a beam
    with pytest.raises(RuntimeError):
        _flx(d, prop, dict(bc, umu0=ub))
    st = torch.zeros(nwave * ncol, dtype=torch.int32, device=dev)
    _flx(d, prop, dict(bc, umu0=ub), status=st)
    s = st.cpu().numpy().reshape(nwave, ncol)
    assert s[1, 2] & _lib.HD_STATUS_BAD_INPUT and np.count_nonzero(s & 0x0F) == 1, s
    pn = prop.copy()
    pn[0, 1, 2, 0] = np.nan
    st.zero_()
    got = _flx(d, pn, bc, status=st)
    s = st.cpu().numpy().reshape(nwave, ncol)
    assert s[0, 1] & _lib.HD_STATUS_NONFINITE, s
    assert np.count_nonzero(s & 0x0F) == 1, s
    assert np.all(np.isfinite(np.delete(got.reshape(nwave * ncol, -1), 1, axis=0)))


def test_graph_capture_replay():
    """A warm call sizes the scratch; the captured call then allocates nothing and its
    replay equals the eager record bitwise (one chunk, one stream)."""
    nstr, nwave, ncol, nlyr = 8, 2, 3, 9
    rng = np.random.default_rng(350)
    prop, bc = _hg_batch(rng, nwave, ncol, nlyr, nstr)
    d = _disort(nstr, nlyr, nwave, ncol)
    p, b, _ = _dev(prop, bc)
    ref = d.forward_flx(p, b).clone()
    st = torch.zeros(nwave * ncol, dtype=torch.int32, device=p.device)
    out = torch.empty_like(ref)
    d.forward_flx(p, b, status=st, out=out)  # warm
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            d.forward_flx(p, b, status=st, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


def test_band_flx():
    from pyharp_amd.spectral import band_flux, band_flx
    nstr, nwave, ncol, nlyr = 8, 5, 3, 6
    rng = np.random.default_rng(360)
    prop, bc = _hg_batch(rng, nwave, ncol, nlyr, nstr)
    d = _disort(nstr, nlyr, nwave, ncol)
    p, b, _ = _dev(prop, bc)
    flx = d.forward_flx(p, b)
    w = torch.as_tensor(rng.uniform(0.1, 1.0, nwave), device=p.device)
    got = band_flx(flx, w)
    assert tuple(got.shape) == (ncol, nlyr + 1, NFLX)
    ref = (flx * w[:, None, None, None]).sum(0)
    assert (got - ref).abs().max().item() <= 1e-14 * ref.abs().max().item()
    bf = band_flux(d.forward(p, b), w)  # (ncol, nlev, 2): slot 0 is the upward flux
    err = rel_err(got[..., [IFLUP]].cpu().numpy(), bf[..., 0:1].cpu().numpy()).max()
    assert err < 1e-10, err
    with pytest.raises(RuntimeError, match="band_flx"):
        band_flx(flx[..., :2].contiguous(), w)
    with pytest.raises(RuntimeError, match="band_flux"):
        band_flux(flx, w)


def test_cpu_tensor_round_trip():
    nstr, nwave, ncol, nlyr = 8, 2, 3, 4
    rng = np.random.default_rng(370)
    prop, bc = _hg_batch(rng, nwave, ncol, nlyr, nstr)
    d = _disort(nstr, nlyr, nwave, ncol)
    on_dev = _flx(d, prop, bc)
    got = d.forward_flx(torch.as_tensor(prop), {k: torch.as_tensor(v) for k, v in bc.items()})
    assert got.device.type == "cpu" and tuple(got.shape) == (nwave, ncol, nlyr + 1, NFLX)
    assert np.array_equal(got.numpy(), on_dev)


def test_refused_configurations():
    prop = torch.zeros((1, 1, 2, 10), dtype=torch.float64, device="cuda:0")
    from pyharp_amd import Disort, DisortOptions
    op = DisortOptions().flags("lamber,quiet,onlyfl,usrtau").nwave(1).ncol(1)
    op.user_tau([0.0, 0.1])
    op.ds().nlyr, op.ds().nstr, op.ds().nmom = 2, 8, 8
    with pytest.raises(RuntimeError, match="usrtau"):
        Disort(op).forward_flx(prop, {})
    op = DisortOptions().flags("lamber,quiet").nwave(1).ncol(1)
    op.ds().nlyr, op.ds().nstr, op.ds().nmom = 2, 8, 8
    with pytest.raises(RuntimeError, match="onlyfl"):
        Disort(op).forward_flx(prop, {})
    d = _disort(8, 2, 1, 1)
    with pytest.raises(RuntimeError, match="out must be"):
        d.forward_flx(prop, {}, out=torch.empty((1, 1, 3, 2), dtype=torch.float64,
                                                device="cuda:0"))


def test_index_constants():
    from pyharp_amd import index
    assert (index.IRFLDIR, index.IRFLDN, index.IFLUP, index.IDFDT, index.IUAVG, index.IUAVGDN,
            index.IUAVGUP, index.IUAVGSO, index.NFLX) == (0, 1, 2, 3, 4, 5, 6, 7, 8)
    assert (IRFLDIR, IRFLDN, IFLUP, IDFDT, IUAVG, IUAVGDN, IUAVGUP, IUAVGSO) == tuple(range(8))


def test_cpp_dropin_disotest_1a():
    """harp_amd::DisortImpl::forward_flx (include/harp_amd/disort.hpp) on DISOTEST 1a;
    tests/cpp/build_flx.sh compiles the program, which prints `flx <level> <name> <value>`."""
    from helpers import disotest
    exe = os.path.join(ROOT, "tests", "cpp", "disort_flx_dropin")
    if not os.path.exists(exe):
        subprocess.run([os.path.join(ROOT, "tests", "cpp", "build_flx.sh")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = np.full((2, NFLX), np.nan)
    for line in out.strip().splitlines():
        tag, lev, name, val = line.split()
        assert tag == "flx"
        got[int(lev), NAMES.index(name)] = float(val)
    t = disotest()
    c, k = t["common"], t["cases"]["1a"]
    pmom = np.zeros((1, c["nstr"] + 1))
    pmom[:, 0] = 1.0
    ref, scale, _ = flx_ref.flx_ref_column([k["tau"]], [k["ssalb"]], pmom, c["nstr"],
                                           umu0=c["umu0"],
                                           fbeam=c["fbeam_times_umu0"] / c["umu0"],
                                           albedo=c["albedo"])
    # the program's level 0 is the surface; the helper's column runs top -> bottom
    _check_record(got[None, None], ref[::-1][None, None], scale[::-1][None, None])
    np.testing.assert_allclose(got[::-1, IDFDT], [25.4067, 18.6531], rtol=5e-6)
