"""HIP Beer-Lambert solver (hd_beer_flux / hd_beer_flux_band / hd_beer_rays through
pyharp_amd.BeerLambert): parity with its numpy restatement (tests/beer_ref.py, the same
formulas) and with the DISORT solver of the same library at ssa = 0, the layer-transfer
edge cases, the bitwise band sums, status bits, CPU tensors and graph capture.

Bounds.  Against Disort the project's TOL = 1e-6 (two algorithms).  Against beer_ref the
same TOL and, beside it, TIGHT: the same formulas in the same precision, so what remains
is rounding -- ten times the worst error of the first GPU run (MEASURED, recorded in
profiles/beer/parity_margins.json), capped at 1e-10: two different algorithms already
agree to 1.3e-10 on the CPU (tests/test_beer_cpu.py), so a same-formula difference above
that would be a defect.
"""

import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import beer_ref
from helpers import TOL, margin, rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED = 1.905e-14  # worst error against beer_ref in the first GPU run (parity_margins.json)
TIGHT = min(1.0e-10, 10.0 * MEASURED)
BAD = 0x01


def _beer(nstr, nlyr, nwave, ncol, *, planck=False, wl=None, wu=None, alpha=0.0):
    from pyharp_amd import BeerLambert, BeerLambertOptions
    op = BeerLambertOptions().nstr(nstr).nlyr(nlyr).nwave(nwave).ncol(ncol).alpha(alpha)
    if planck:
        op.planck(True).wave_lower(list(map(float, wl))).wave_upper(list(map(float, wu)))
    return BeerLambert(op)


def _t(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64, device=DEV)


def _dev(d):
    return {k: _t(v) for k, v in d.items()}


def _ray_err(got, ref):
    """max |got - ref| / max |ref| per solve"""
    scale = np.maximum(np.abs(ref).max(axis=-1, keepdims=True), 1e-300)
    return (np.abs(got - ref) / scale).max()


def _case(rng, nwave, ncol, nlyr, nprop, planck, beam=True):
    prop = rng.uniform(0.0, 0.9, (nwave, ncol, nlyr, nprop))  # slots >= 1: ignored junk
    prop[..., 0] = 10.0 ** rng.uniform(-5, 1, (nwave, ncol, nlyr))
    bc = {"albedo": rng.uniform(0, 1, (nwave, ncol)), "fisot": rng.uniform(0, 0.1, (nwave, ncol))}
    if beam:
        bc.update(fbeam=rng.uniform(0.5, 2, (nwave, ncol)), umu0=rng.uniform(0.1, 1, (nwave, ncol)))
    kw = {}
    if planck:
        from oracle.disort_np import layer2level
        kw["temf"] = layer2level(np.linspace(290, 180, max(nlyr, 2))[None, :] +
                                 rng.uniform(-5, 5, (ncol, max(nlyr, 2))))[:, :nlyr + 1]
        bc.update(btemp=rng.uniform(250, 300, (nwave, ncol)),
                  ttemp=rng.uniform(100, 200, (nwave, ncol)),
                  temis=rng.uniform(0.1, 0.9, (nwave, ncol)))
        kw["wave_lower"] = np.sort(rng.uniform(100, 1500, nwave))
        kw["wave_upper"] = kw["wave_lower"] + rng.uniform(10, 300, nwave)
    return prop, bc, kw


def _ref_kw(kw):
    return dict(planck="temf" in kw, wave_lower=kw.get("wave_lower"),
                wave_upper=kw.get("wave_upper"))


def _temf(kw):
    return _t(kw["temf"]) if "temf" in kw else None


UMU5 = np.array([-1.0, -0.3, 0.05, 0.37, 1.0])


# --- 1: parity with the restatement --------------------------------------------------
@pytest.mark.parametrize("layout", ["67x1", "1x67"])
@pytest.mark.parametrize("nlyr", [1, 3, 17])
@pytest.mark.parametrize("nstr", [2, 8, 32])
def test_parity_with_restatement(nstr, nlyr, layout):
    """67 solves (one wave and three lanes) as 67 waves x 1 column and 1 wave x 67
    columns; nprop 1 (extinction only) and 2 + nstr; without and with Planck emission;
    nlyr 17 crosses a 16-layer tile"""
    nwave, ncol = (67, 1) if layout == "67x1" else (1, 67)
    for nprop in (1, 2 + nstr):
        for planck in (False, True):
            rng = np.random.default_rng(9000 + 100 * nstr + nlyr + 7 * planck + nprop)
            prop, bc, kw = _case(rng, nwave, ncol, nlyr, nprop, planck)
            b = _beer(nstr, nlyr, nwave, ncol, planck=planck, wl=kw.get("wave_lower"),
                      wu=kw.get("wave_upper"))
            flux = b.forward(_t(prop), _dev(bc), _temf(kw)).cpu().numpy()
            ref = beer_ref.beer_flux(prop, bc, kw.get("temf"), nstr=nstr, **_ref_kw(kw))
            err = rel_err(flux, ref).max()
            umu = np.where(rng.uniform(size=(ncol, 5)) < 0.5, -1.0, 1.0) * \
                rng.uniform(0.02, 1.0, (ncol, 5))
            rad = b.forward_rays(_t(prop), _dev(bc), _temf(kw), umu=_t(umu)).cpu().numpy()
            rref = beer_ref.beer_rays(prop, bc, kw.get("temf"), nstr=nstr, umu=umu, **_ref_kw(kw))
            rerr = _ray_err(rad, rref)
            print(f"beer parity nstr={nstr} nlyr={nlyr} {layout} nprop={nprop} planck={planck} "
                  f"flux {err:.3e} rays {rerr:.3e}")
            assert margin(max(err, rerr)) < TOL
            assert max(err, rerr) < TIGHT, (err, rerr)


# --- 2: parity with Disort on the same device ------------------------------------------
@functools.lru_cache(maxsize=None)
def _disort_pair(nstr):
    """one ssa = 0 thermal + beam problem through both solvers"""
    from pyharp_amd import Disort, DisortOptions
    rng = np.random.default_rng(9500 + nstr)
    nwave, ncol, nlyr = 3, 5, 12
    prop, bc, kw = _case(rng, nwave, ncol, nlyr, 2 + nstr, True)
    prop[..., 1:] = 0.0
    wl, wu = list(map(float, kw["wave_lower"])), list(map(float, kw["wave_upper"]))
    b = _beer(nstr, nlyr, nwave, ncol, planck=True, wl=wl, wu=wu)

    def disort(flags):
        op = DisortOptions().flags(flags).nwave(nwave).ncol(ncol).wave_lower(wl).wave_upper(wu)
        op.ds().nlyr, op.ds().nstr, op.ds().nmom = nlyr, nstr, nstr
        return Disort(op)

    args = (_t(prop), _dev(bc), _temf(kw))
    umu = torch.tensor(UMU5, dtype=torch.float64, device=DEV)
    return dict(
        bflux=b.forward(*args).cpu().numpy(),
        dflux=disort("lamber,quiet,onlyfl,planck").forward(*args).cpu().numpy(),
        brad=b.forward_rays(*args, umu=umu).cpu().numpy(),
        drad=disort("lamber,quiet,planck").forward_rays(
            *args, umu=umu, phi=torch.zeros_like(umu)).cpu().numpy())


@pytest.mark.parametrize("nstr", [8, 16])
def test_flux_vs_disort(nstr):
    r = _disort_pair(nstr)
    err = rel_err(r["bflux"], r["dflux"]).max()
    print("beer flux vs Disort.forward", nstr, err)
    assert margin(err) < TOL


@pytest.mark.parametrize("nstr", [8, 16])
def test_rays_vs_disort(nstr):
    """Disort.forward_rays at the layer boundaries, top first: upward rays at the top
    level, downward ones at the bottom level"""
    r = _disort_pair(nstr)
    ref = np.where(UMU5 > 0, r["drad"][:, :, 0, :], r["drad"][:, :, -1, :])
    err = _ray_err(r["brad"], ref)
    print("beer rays vs Disort.forward_rays", nstr, err)
    assert margin(err) < TOL


# --- 3: edge layers -------------------------------------------------------------------
def test_edge_layers():
    """tau = 0, 1e-12, 1e-3, either side of the series switch (x = 1/8 along mu = 1) and
    800 in one column"""
    nstr, nlyr = 8, 6
    prop = np.zeros((1, 2, nlyr, 1))
    prop[0, 0, :, 0] = [1e-3, 0.0, 800.0, 0.1249999, 1e-12, 0.1250001]
    prop[0, 1, :, 0] = [0.0, 0.1250001, 1e-12, 0.1249999, 800.0, 1e-3]
    rng = np.random.default_rng(9600)
    _, bc, kw = _case(rng, 1, 2, nlyr, 1, True)
    b = _beer(nstr, nlyr, 1, 2, planck=True, wl=kw["wave_lower"], wu=kw["wave_upper"])
    flux = b.forward(_t(prop), _dev(bc), _temf(kw)).cpu().numpy()
    rad = b.forward_rays(_t(prop), _dev(bc), _temf(kw), umu=_t(UMU5)).cpu().numpy()
    assert np.isfinite(flux).all() and np.isfinite(rad).all()
    err = rel_err(flux, beer_ref.beer_flux(prop, bc, kw["temf"], nstr=nstr, **_ref_kw(kw))).max()
    rerr = _ray_err(rad, beer_ref.beer_rays(prop, bc, kw["temf"], nstr=nstr, umu=UMU5,
                                            **_ref_kw(kw)))
    print("edge layers", err, rerr)
    assert margin(max(err, rerr)) < TOL
    assert max(err, rerr) < TIGHT


def test_empty_column_returns_the_boundary_values_exactly():
    """every tau = 0: nothing is absorbed or emitted on the way, so every level carries
    the boundary's flux and every ray its boundary's intensity, to the bit"""
    nstr, nlyr = 8, 19
    rng = np.random.default_rng(9700)
    prop, bc, kw = _case(rng, 2, 3, nlyr, 3, True)
    prop[..., 0] = 0.0
    b = _beer(nstr, nlyr, 2, 3, planck=True, wl=kw["wave_lower"], wu=kw["wave_upper"])
    flux = b.forward(_t(prop), _dev(bc), _temf(kw)).cpu().numpy()
    assert np.array_equal(flux, np.broadcast_to(flux[:, :, :1, :], flux.shape))
    ref = beer_ref.beer_flux(prop, bc, kw["temf"], nstr=nstr, **_ref_kw(kw))
    assert rel_err(flux, ref).max() < TIGHT
    rad = b.forward_rays(_t(prop), _dev(bc), _temf(kw), umu=_t(UMU5)).cpu().numpy()
    assert np.array_equal(rad[..., 2:], np.broadcast_to(rad[..., 2:3], rad[..., 2:].shape))
    assert np.array_equal(rad[..., :2], np.broadcast_to(rad[..., :1], rad[..., :2].shape))
    # upward: the surface's intensity = up flux / pi (sum w mu = 1/2, to rounding);
    # downward: fisot + temis B(ttemp)
    assert np.abs(rad[..., 4] * np.pi / flux[:, :, 0, 0] - 1.0).max() < 1e-14
    rref = beer_ref.beer_rays(prop, bc, kw["temf"], nstr=nstr, umu=UMU5, **_ref_kw(kw))
    assert _ray_err(rad, rref) < TIGHT


# --- 4: band sums ---------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(130, 1), (5, 67), (700, 1)])
def test_band_sums_bitwise(shape):
    """forward_band / forward_rays_band are hd_band_sum of the stored per-wave result,
    to the bit, at the automatic chunking and in chunks of 16 solves (which start inside a
    wave at 67 columns), with and without the per-wave values stored.  One column with
    128 or more waves in a chunk takes the LDS-staged sum: one batch at 130 waves, three
    (the last one partial) at 700"""
    from pyharp_amd.disort import _context
    from pyharp_amd.spectral import band_rad
    nwave, ncol = shape
    nstr, nlyr = 4, 5
    rng = np.random.default_rng(9800 + nwave)
    prop, bc, kw = _case(rng, nwave, ncol, nlyr, 2, True)
    b = _beer(nstr, nlyr, nwave, ncol, planck=True, wl=kw["wave_lower"], wu=kw["wave_upper"])
    args = (_t(prop), _dev(bc), _temf(kw))
    w = _t(rng.uniform(0.1, 2.0, nwave))
    umu = _t(np.where(rng.uniform(size=(ncol, 3)) < 0.5, -1.0, 1.0) * rng.uniform(0.05, 1, (ncol, 3)))
    flux = b.forward(*args)
    rad = b.forward_rays(*args, umu=umu)
    fsum, rsum = band_rad(flux, w), band_rad(rad, w)
    ctx = _context(0)
    for chunk in (0, 16):
        ctx.set_chunk(chunk)
        try:
            assert torch.equal(b.forward(*args), flux), chunk
            assert torch.equal(b.forward_band(*args, weights=w), fsum), chunk
            assert torch.equal(b.forward_rays_band(*args, umu=umu, weights=w), rsum), chunk
            fst = torch.full_like(flux, -1.0)
            out = torch.full_like(fsum, -1.0)
            assert b.forward_band(*args, weights=w, out=out, flux=fst) is out
            assert torch.equal(out, fsum) and torch.equal(fst, flux), chunk
            rst = torch.full_like(rad, -1.0)
            out = torch.full_like(rsum, -1.0)
            assert b.forward_rays_band(*args, umu=umu, weights=w, out=out, rad=rst) is out
            assert torch.equal(out, rsum) and torch.equal(rst, rad), chunk
        finally:
            ctx.set_chunk(0)
    assert tuple(fsum.shape) == (ncol, nlyr + 1, 2) and tuple(rsum.shape) == (ncol, 3)


def test_small_batch_kernel_returns_the_one_lane_kernels_bits():
    """chunks of at most 2 048 solves run with a solve's streams in neighbouring lanes;
    the level flux is summed in the one-lane kernel's order, so 2 100 solves in one chunk
    (one lane per solve) and in chunks of 1 000 agree to the bit, at every team width"""
    from pyharp_amd.disort import _context
    nlyr, nwave, ncol = 5, 3, 700
    ctx = _context(0)
    for nstr in (4, 6, 12, 32):
        rng = np.random.default_rng(9850 + nstr)
        prop, bc, kw = _case(rng, nwave, ncol, nlyr, 1, True)
        b = _beer(nstr, nlyr, nwave, ncol, planck=True, wl=kw["wave_lower"], wu=kw["wave_upper"])
        args = (_t(prop), _dev(bc), _temf(kw))
        one = b.forward(*args)
        ctx.set_chunk(1000)
        try:
            team = b.forward(*args)
        finally:
            ctx.set_chunk(0)
        assert torch.equal(team, one), nstr


# --- 5: status ------------------------------------------------------------------------
def test_bad_ray_cosine_flags_its_column_only():
    nstr, nlyr, nwave, ncol = 4, 3, 2, 4
    rng = np.random.default_rng(9900)
    prop, bc, _ = _case(rng, nwave, ncol, nlyr, 1, False)
    b = _beer(nstr, nlyr, nwave, ncol)
    good = np.tile([0.5, -0.5, 1.0], (ncol, 1))
    ref = b.forward_rays(_t(prop), _dev(bc), umu=_t(good)).cpu().numpy()
    for c, bad in ((1, 0.0), (2, float("nan")), (3, 1.5)):
        umu = good.copy()
        umu[c, 1] = bad
        st = torch.full((nwave * ncol,), -1, dtype=torch.int32, device=DEV)
        rad = b.forward_rays(_t(prop), _dev(bc), umu=_t(umu), status=st).cpu().numpy()
        flagged = st.cpu().numpy().reshape(nwave, ncol)
        assert np.isnan(rad[:, c, 1]).all()
        rad[:, c, 1] = ref[:, c, 1]
        assert np.array_equal(rad, ref)
        assert (flagged[:, c] == BAD).all() and (np.delete(flagged, c, axis=1) == 0).all()
        with pytest.raises(RuntimeError, match="at least one solve failed"):
            b.forward_rays(_t(prop), _dev(bc), umu=_t(umu))
    # shared rays: every solve carries the bad ray
    st = torch.zeros(nwave * ncol, dtype=torch.int32, device=DEV)
    rad = b.forward_rays(_t(prop), _dev(bc), umu=_t([0.5, 0.0]), status=st).cpu().numpy()
    assert (st.cpu().numpy() == BAD).all() and np.isnan(rad[..., 1]).all()
    assert np.array_equal(rad[..., 0], ref[..., 0])


def test_bad_inputs_flag_their_own_solve():
    nstr, nlyr, nwave, ncol = 4, 3, 3, 5
    rng = np.random.default_rng(9910)
    prop, bc, _ = _case(rng, nwave, ncol, nlyr, 2, False)
    b = _beer(nstr, nlyr, nwave, ncol)
    ref = b.forward(_t(prop), _dev(bc)).cpu().numpy()
    prop2 = prop.copy()
    prop2[1, 2, 1, 0] = -0.1
    prop2[2, 4, 0, 0] = float("inf")
    bc2 = {k: v.copy() for k, v in bc.items()}
    bc2["albedo"][0, 1] = 1.5
    bc2["umu0"][0, 3] = 0.0
    want = np.zeros((nwave, ncol), dtype=np.int32)
    for w, c in ((1, 2), (2, 4), (0, 1), (0, 3)):
        want[w, c] = BAD
    st = torch.full((nwave * ncol,), -1, dtype=torch.int32, device=DEV)
    flux = b.forward(_t(prop2), _dev(bc2), status=st).cpu().numpy()
    got = st.cpu().numpy().reshape(nwave, ncol)
    assert np.array_equal(got & 0x0B, want), got  # NONFINITE may join on the inf solve
    ok = want == 0
    assert np.array_equal(flux[ok], ref[ok])
    with pytest.raises(RuntimeError, match="at least one solve failed"):
        b.forward(_t(prop2), _dev(bc2))
    # rays validate the thickness too (no down pass runs without an albedo array)
    st.fill_(-1)
    b.forward_rays(_t(prop2), {"fisot": _t(bc["fisot"])}, umu=_t([0.5, -0.5]), status=st)
    got = st.cpu().numpy().reshape(nwave, ncol)
    assert (got[1, 2] & BAD) and (got[2, 4] & BAD)
    got[1, 2] = got[2, 4] = 0
    assert not got.any()


def test_alpha_with_an_empty_column_is_flagged():
    nstr, nlyr, nwave, ncol = 4, 3, 1, 3
    rng = np.random.default_rng(9920)
    prop, bc, kw = _case(rng, nwave, ncol, nlyr, 1, True)
    prop[0, 1, :, 0] = 0.0
    b = _beer(nstr, nlyr, nwave, ncol, planck=True, wl=kw["wave_lower"], wu=kw["wave_upper"],
              alpha=1.3)
    st = torch.zeros(nwave * ncol, dtype=torch.int32, device=DEV)
    b.forward_rays(_t(prop), _dev(bc), _temf(kw), umu=_t([0.7, -0.7]), status=st)
    assert st.cpu().tolist() == [0, BAD, 0]
    with pytest.raises(RuntimeError, match="at least one solve failed"):
        b.forward_rays(_t(prop), _dev(bc), _temf(kw), umu=_t([0.7, -0.7]))


# --- 6: alpha -------------------------------------------------------------------------
def test_alpha_term_vs_restatement():
    """alpha = 1.3 at the top of the atmosphere: slant depths on both sides of
    x_s = alpha + 1 (the series / continued-fraction split) and beyond 1000 (no term)"""
    nstr, nlyr, nwave, ncol = 8, 4, 2, 4
    rng = np.random.default_rng(9930)
    prop, bc, kw = _case(rng, nwave, ncol, nlyr, 1, True)
    for c, total in enumerate((1e-3, 0.5, 6.0, 300.0)):
        prop[:, c, :, 0] *= total / prop[:, c, :, 0].sum(axis=-1, keepdims=True)
    umu = np.array([1.0, 0.6, 0.25, -0.5])  # 300 / 0.25 > 1000
    b = _beer(nstr, nlyr, nwave, ncol, planck=True, wl=kw["wave_lower"], wu=kw["wave_upper"],
              alpha=1.3)
    rad = b.forward_rays(_t(prop), _dev(bc), _temf(kw), umu=_t(umu)).cpu().numpy()
    ref = beer_ref.beer_rays(prop, bc, kw["temf"], nstr=nstr, umu=umu, alpha=1.3, **_ref_kw(kw))
    plain = beer_ref.beer_rays(prop, bc, kw["temf"], nstr=nstr, umu=umu, **_ref_kw(kw))
    assert (ref[..., 0] > plain[..., 0] * (1 + 1e-6))[:, :3].all()  # the term is there
    err = _ray_err(rad, ref)
    print("alpha 1.3", err)
    assert margin(err) < TOL
    assert err < TIGHT


# --- 7: CPU tensors, graph capture, the C++ module ---------------------------------
def test_cpu_tensors_round_trip():
    nstr, nlyr, nwave, ncol = 8, 7, 3, 4
    rng = np.random.default_rng(9940)
    prop, bc, kw = _case(rng, nwave, ncol, nlyr, 2, True)
    b = _beer(nstr, nlyr, nwave, ncol, planck=True, wl=kw["wave_lower"], wu=kw["wave_upper"])
    cpu = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64)  # noqa: E731
    w = rng.uniform(0.1, 1, nwave)
    dargs = (_t(prop), _dev(bc), _temf(kw))
    cargs = (cpu(prop), {k: cpu(v) for k, v in bc.items()}, cpu(kw["temf"]))
    for name, kws in (("forward", {}), ("forward_band", dict(weights=w)),
                      ("forward_rays", dict(umu=UMU5)),
                      ("forward_rays_band", dict(umu=UMU5, weights=w))):
        on_dev = getattr(b, name)(*dargs, **{k: _t(v) for k, v in kws.items()})
        on_cpu = getattr(b, name)(*cargs, **{k: cpu(v) for k, v in kws.items()})
        assert on_cpu.device.type == "cpu" and on_dev.device == DEV
        assert torch.equal(on_cpu, on_dev.cpu()), name


def test_graph_capture_replay():
    """a captured call never allocates: refused until an eager call of the same shape
    has sized the context, then replayed to the same bits"""
    import threading
    nstr, nlyr, nwave, ncol = 8, 20, 3, 70
    rng = np.random.default_rng(9950)
    prop, bc, kw = _case(rng, nwave, ncol, nlyr, 2, True)
    p, bd, tf = _t(prop), _dev(bc), _temf(kw)
    umu, w = _t(UMU5), _t(rng.uniform(0.1, 1, nwave))
    res = {}

    def worker():  # a fresh thread has a fresh context: nothing sized yet
        try:
            from pyharp_amd.disort import _context
            _context(0)
            b0 = _beer(nstr, nlyr, nwave, ncol)  # no emission: no wave bounds to upload
            b = _beer(nstr, nlyr, nwave, ncol, planck=True, wl=kw["wave_lower"],
                      wu=kw["wave_upper"])
            st = torch.zeros(nwave * ncol, dtype=torch.int32, device=DEV)
            flux = torch.empty((nwave, ncol, nlyr + 1, 2), dtype=torch.float64, device=DEV)
            brad = torch.empty((ncol, 5), dtype=torch.float64, device=DEV)
            s = torch.cuda.Stream(device=DEV)
            s.wait_stream(torch.cuda.current_stream(DEV))
            g0 = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.stream(s):
                    with torch.cuda.graph(g0, stream=s):
                        b0.forward(p, bd, status=st, out=flux)
            except RuntimeError as e:
                res["refused"] = str(e)
            torch.cuda.synchronize()
            res["flux"] = b.forward(p, bd, tf, status=st, out=flux).clone()  # sizes the scratch
            res["brad"] = b.forward_rays_band(p, bd, tf, umu=umu, weights=w, status=st,
                                              out=brad).clone()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            s.wait_stream(torch.cuda.current_stream(DEV))
            with torch.cuda.stream(s):
                with torch.cuda.graph(g, stream=s):
                    b.forward(p, bd, tf, status=st, out=flux)
                    b.forward_rays_band(p, bd, tf, umu=umu, weights=w, status=st, out=brad)
            flux.zero_()
            brad.zero_()
            g.replay()
            torch.cuda.synchronize()
            res["flux_replay"], res["brad_replay"] = flux.clone(), brad.clone()
        except Exception as e:  # surfaced by the asserts below
            res["error"] = repr(e)

    t = threading.Thread(target=worker)
    t.start()
    t.join()
    assert "error" not in res, res["error"]
    assert "stream capture" in res.get("refused", ""), res.get("refused")
    assert torch.equal(res["flux_replay"], res["flux"])
    assert torch.equal(res["brad_replay"], res["brad"])


def test_cpp_beer_dropin():
    """tests/cpp/beer_dropin.cpp: harp_amd::BeerLambert's four methods on a small
    thermal problem; its printed lines against the Python module on the same inputs"""
    exe = os.path.join(ROOT, "tests", "cpp", "beer_dropin")
    if not os.path.exists(exe):
        subprocess.run([os.path.join(ROOT, "tests", "cpp", "build_beer.sh")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    nwave, ncol, nlyr, nstr = 4, 2, 5, 8
    prop = np.zeros((nwave, ncol, nlyr, 1))
    for w in range(nwave):
        for c in range(ncol):
            for l in range(nlyr):
                prop[w, c, l, 0] = 0.05 * (1 + w) * (1 + l) / (1 + c)
    bc = {"albedo": np.full((nwave, ncol), 0.3), "btemp": np.full((nwave, ncol), 290.0)}
    temf = np.tile(np.linspace(280.0, 200.0, nlyr + 1), (ncol, 1))
    wl = [100.0 + 200.0 * w for w in range(nwave)]
    wu = [300.0 + 200.0 * w for w in range(nwave)]
    wts = np.array([0.1, 0.2, 0.3, 0.4])
    b = _beer(nstr, nlyr, nwave, ncol, planck=True, wl=wl, wu=wu, alpha=0.0)
    ba = _beer(nstr, nlyr, nwave, ncol, planck=True, wl=wl, wu=wu, alpha=1.3)
    args = (_t(prop), _dev(bc), _t(temf))
    umu = _t([1.0, 0.5, -0.5])
    exp = {"flux": b.forward(*args)[:, 1].reshape(-1),
           "bflux": b.forward_band(*args, weights=_t(wts))[1].reshape(-1),
           "rad": ba.forward_rays(*args, umu=umu)[:, 1].reshape(-1),
           "brad": ba.forward_rays_band(*args, umu=umu, weights=_t(wts))[1].reshape(-1)}
    for tag, want in exp.items():
        got = {int(l.split()[1]): float(l.split()[2]) for l in out if l.startswith(tag + " ")}
        want = want.cpu().numpy()
        assert len(got) == want.size, (tag, out)
        for i, v in got.items():
            assert abs(v - want[i]) <= 1e-12 * abs(want[i]), (tag, i, v, want[i])
