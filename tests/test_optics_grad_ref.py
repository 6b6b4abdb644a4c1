"""The judge of the optics gradients (tests/optics_grad_ref.py) without a GPU: its
forwards against the numpy restatement it restates (oracle/harp_np.py), its autograd
gradients against central differences of that restatement, the closed-form points of the
derivative conventions (include/hdharp.h "Gradients of the optics"), the four _bwd
symbols, and the modules' host-side refusals, which fire before a device is touched.

Bounds.  Forward: the same formulas in the same precision, 1e-13 relative.  Gradients:
1e-6 of the tensor's largest component (central differences at these steps carry about
1e-9).  Steps: 1e-2 where the function is exactly linear in the input (conc in RFM and
attenuate, dz), a relative 1e-6 otherwise.  ext0 of band_loop_optics is NOT linear (the
ssa divides by ext0 + ...), so it takes the relative 1e-6.  Every sampled wavelength,
ln p and temperature anomaly lies at least ten steps from a knot (asserted below), so no
difference quotient straddles a kink.
"""

import os

import numpy as np
import pytest
import torch

import optics_grad_ref as ogr
from oracle import harp_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1.0e-6
H_REL = 1.0e-6


# ---- cases ---------------------------------------------------------------------------
def _tables(rng):
    """two attenuators on one species (the second with an asymmetry table, descending
    wavelengths) and one on another"""
    t = []
    for n, sp, g, desc in ((5, 1, None, False), (4, 1, True, True), (6, 2, True, False)):
        wl = np.sort(rng.uniform(0.2, 5.0, n))
        if desc:
            wl = wl[::-1].copy()
        kd = np.stack([rng.uniform(0.5, 3.0, n), rng.uniform(0.1, 0.95, n)], axis=1)
        t.append((wl, kd, sp, rng.uniform(-0.8, 0.8, n) if g else None))
    return t


def _coords(rng, tables, n):
    """n wavelengths inside and outside the tables, none within 1e-3 of a knot"""
    knots = np.concatenate([t[0] for t in tables])
    out = []
    while len(out) < n:
        x = rng.uniform(0.1, 6.0)
        if np.abs(knots - x).min() > 1e-3:
            out.append(x)
    return np.array(out)


def _rfm_table(rng, nw=4, npres=6, nt=5):
    return dict(wave=np.linspace(10.0, 150.0, nw), lnp=np.log(np.logspace(6, 1, npres)),
                tgrid=np.linspace(-40.0, 40.0, nt), tref=np.linspace(320.0, 150.0, npres),
                kdata=rng.uniform(-4.0, 2.0, (nw, npres, nt)))


def _rfm_state(rng, tab, ncol, nlyr):
    """p, T inside the grid, with one (col, lyr) above the pressure range and one beyond
    the anomaly range; conc with an exact zero"""
    pres = np.exp(rng.uniform(tab["lnp"].min() + 0.1, tab["lnp"].max() - 0.1, (ncol, nlyr)))
    pres[0, 0] = 5.0e6
    tref = np.array([[harp_np.interpn([np.log(p)], tab["tref"], [tab["lnp"]]) for p in row]
                     for row in pres])
    temp = tref + rng.uniform(-35.0, 35.0, (ncol, nlyr))
    temp[-1, -1] = tref[-1, -1] + 55.0
    conc = rng.uniform(0.01, 2.0, (ncol, nlyr, 3))
    conc[0, -1, 1] = 0.0
    return conc, pres, temp, temp - tref


def _rfm_np(tab, conc, pres, temp, species=1):
    return harp_np.rfm_forward(tab["wave"], tab["lnp"], tab["tgrid"], tab["tref"], tab["kdata"],
                               conc, pres, temp, species)


def _rfm_t(tab, conc, pres, temp, species=1):
    return ogr.rfm_forward(tab["wave"], tab["lnp"], tab["tgrid"], tab["tref"], tab["kdata"],
                           conc, pres, temp, species)


def _rel(got, ref):
    return (np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)).max()


# ---- forwards ------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["wavelength", "wavenumber"])
def test_table_forwards_equal_the_restatement(kind):
    rng = np.random.default_rng(31)
    tables = _tables(rng)
    x = _coords(rng, tables, 7)
    x[0], x[1] = tables[0][0][2], tables[0][0][-1]  # on an inner knot, on the last knot
    kw = {kind: x if kind == "wavelength" else 1.0e4 / x}
    conc = rng.uniform(0.0, 2.0, (2, 3, 3))
    conc[1, 1] = 0.0  # a layer without extinction
    dz = rng.uniform(10.0, 100.0, (2, 3))
    ext0 = rng.uniform(0.0, 1.0, (7, 2, 3))
    wl, kd, sp, _ = tables[0]
    errs = [_rel(ogr.attenuate(wl, kd, sp, conc, **kw).numpy(),
                 harp_np.attenuate(wl, kd, sp, conc, **kw))]
    t3 = [t[:3] for t in tables]
    got = ogr.band_optics(t3, conc, dz, 4, **kw).numpy()
    ref = harp_np.band_optics(t3, conc, dz, 4, **kw)
    assert np.array_equal(got[..., 1] == 0.0, ref[..., 1] == 0.0) and (got[:, 1, 1, 1] == 0).all()
    errs.append(_rel(got, ref))
    for nmom, e0 in ((0, None), (8, ext0)):
        errs.append(_rel(ogr.band_loop_optics(tables, conc, dz, nmom, ext0=e0, **kw).numpy(),
                         harp_np.band_loop_optics(tables, conc, dz, nmom, ext0=e0, **kw)))
    print("optics_grad_ref table forwards vs harp_np", kind, errs)
    assert max(errs) < 1e-13


def test_rfm_forward_equals_the_restatement():
    rng = np.random.default_rng(32)
    tab = _rfm_table(rng)
    conc, pres, temp, _ = _rfm_state(rng, tab, 2, 4)
    pres[1, 0] = np.exp(tab["lnp"][2])                  # on a pressure knot
    err = _rel(_rfm_t(tab, conc, pres, temp).numpy(), _rfm_np(tab, conc, pres, temp))
    print("optics_grad_ref rfm forward vs harp_np", err)
    assert err < 1e-13


def test_epilogue_forwards_equal_the_restatement():
    rng = np.random.default_rng(33)
    x, w = rng.uniform(-1, 1, (17, 3, 5, 2)), rng.uniform(0.1, 2.0, 17)
    assert _rel(ogr.band_sum(x, w).numpy(), harp_np.band_flux(x, w)) < 1e-13
    bf, dz, rho = rng.uniform(1, 9, (3, 6, 2)), rng.uniform(1, 2, (3, 5)), rng.uniform(1, 2, (3, 5))
    assert _rel(ogr.heating_rate(bf, dz, rho, 844.0).numpy(),
                harp_np.heating_rate(bf, dz, rho, 844.0)) < 1e-13


# ---- gradients against central differences -------------------------------------------
def _fd(loss, base, h, relative):
    """central differences of loss in one input, component by component"""
    g = np.zeros_like(base)
    for idx in np.ndindex(base.shape):
        step = h * max(abs(base[idx]), 1.0) if relative else h
        xp, xm = base.copy(), base.copy()
        xp[idx] += step
        xm[idx] -= step
        g[idx] = (loss(xp) - loss(xm)) / (2.0 * step)
    return g


def _check(tag, fn_t, fn_n, inputs, steps):
    """autograd of fn_t against central differences of fn_n in every named input"""
    leaves = {k: torch.tensor(v, requires_grad=True) for k, v in inputs.items()}
    out = fn_t(**leaves)
    cot = np.random.default_rng(7).uniform(-1, 1, tuple(out.shape))
    (torch.as_tensor(cot) * out).sum().backward()
    for k, (h, relative) in steps.items():
        def loss(x, k=k):
            return float((cot * fn_n(**{**inputs, k: x})).sum())
        ref = _fd(loss, inputs[k], h, relative)
        err = np.abs(leaves[k].grad.numpy() - ref).max() / np.abs(ref).max()
        print(f"optics_grad_ref {tag} d/d{k}: {err:.3e} of the largest component "
              f"{np.abs(ref).max():.3e}")
        assert err < TOL, (tag, k, err)


def test_table_gradients_against_central_differences():
    rng = np.random.default_rng(41)
    tables = _tables(rng)
    x = _coords(rng, tables, 5)
    # the coordinate is not differentiated: it only has to stay off the knots (asserted in
    # _coords); the inputs below are smooth everywhere
    conc = rng.uniform(0.05, 2.0, (2, 3, 3))
    dz = rng.uniform(10.0, 100.0, (2, 3))
    ext0 = rng.uniform(0.1, 1.0, (5, 2, 3))
    wl, kd, sp, _ = tables[0]
    t3 = [t[:3] for t in tables]
    _check("attenuate", lambda conc: ogr.attenuate(wl, kd, sp, conc, wavelength=x),
           lambda conc: harp_np.attenuate(wl, kd, sp, conc, wavelength=x),
           dict(conc=conc), dict(conc=(1e-2, False)))
    _check("band_optics", lambda conc, dz: ogr.band_optics(t3, conc, dz, 3, wavenumber=1e4 / x),
           lambda conc, dz: harp_np.band_optics(t3, conc, dz, 3, wavenumber=1e4 / x),
           dict(conc=conc, dz=dz), dict(conc=(H_REL, True), dz=(1e-2, False)))
    for nmom, e0 in ((0, None), (8, ext0)):
        inputs = dict(conc=conc, dz=dz)
        steps = dict(conc=(H_REL, True), dz=(1e-2, False))
        if e0 is not None:
            inputs["ext0"] = e0
            steps["ext0"] = (H_REL, True)
        _check(f"band_loop nmom={nmom}",
               lambda **kw: ogr.band_loop_optics(tables, kw["conc"], kw["dz"], nmom, wavelength=x,
                                                 ext0=kw.get("ext0")),
               lambda **kw: harp_np.band_loop_optics(tables, kw["conc"], kw["dz"], nmom,
                                                     wavelength=x, ext0=kw.get("ext0")),
               inputs, steps)


def test_rfm_gradients_against_central_differences():
    rng = np.random.default_rng(42)
    tab = _rfm_table(rng)
    conc, pres, temp, tempa = _rfm_state(rng, tab, 2, 3)
    # ten steps from every knot: ln p moves by 1e-6 per step, the anomaly by 1e-6 T (and by
    # T_ref' 1e-6 when p moves)
    lnp = np.log(pres)
    assert np.abs(lnp[..., None] - tab["lnp"]).min() > 10 * H_REL
    slope = np.abs(np.diff(tab["tref"]) / np.diff(tab["lnp"])).max()
    assert np.abs(tempa[..., None] - tab["tgrid"]).min() > 10 * H_REL * (temp.max() + slope)
    assert (lnp > tab["lnp"].max()).any() and (tempa > tab["tgrid"].max()).any()
    _check("rfm", lambda conc, pres, temp: _rfm_t(tab, conc, pres, temp),
           lambda conc, pres, temp: _rfm_np(tab, conc, pres, temp),
           dict(conc=conc, pres=pres, temp=temp),
           dict(conc=(1e-2, False), pres=(H_REL, True), temp=(H_REL, True)))


def test_epilogue_gradients_against_central_differences():
    rng = np.random.default_rng(43)
    x, w = rng.uniform(-1, 1, (4, 2, 3, 2)), rng.uniform(0.1, 2.0, 4)
    _check("band_sum", lambda x: ogr.band_sum(x, w), lambda x: harp_np.band_flux(x, w),
           dict(x=x), dict(x=(1e-2, False)))
    bf, dz, rho = rng.uniform(1, 9, (2, 4, 2)), rng.uniform(1, 2, (2, 3)), rng.uniform(1, 2, (2, 3))
    _check("heating_rate", lambda bflux, dz, rho: ogr.heating_rate(bflux, dz, rho, 844.0),
           lambda bflux, dz, rho: harp_np.heating_rate(bflux, dz, rho, 844.0),
           dict(bflux=bf, dz=dz, rho=rho),
           dict(bflux=(1e-2, False), dz=(H_REL, True), rho=(H_REL, True)))


# ---- the closed-form points of the conventions ------------------------------------------
def test_slopes_at_the_knots_and_beyond_the_table():
    """one wave, one pressure (every p clamps), anomalies [-10, 0, 10] with ln k = 1, 2, 4:
    slope 0.1 left of 0 and 0.2 right of it"""
    tab = dict(wave=np.array([50.0]), lnp=np.array([np.log(1.0e4)]), tgrid=np.array([-10.0, 0.0, 10.0]),
               tref=np.array([200.0]), kdata=np.array([[[1.0, 2.0, 4.0]]]))
    temp = torch.tensor([[150.0, 195.0, 200.0, 205.0, 210.0, 300.0]], dtype=torch.float64,
                        requires_grad=True)
    pres = torch.tensor([[3.0e3, 1.0e4, 1.0e4, 2.0e4, 1.0e4, 1.0e4]], dtype=torch.float64,
                        requires_grad=True)
    conc = torch.ones((1, 6, 1), dtype=torch.float64, requires_grad=True)
    out = ogr.rfm_forward(tab["wave"], tab["lnp"], tab["tgrid"], tab["tref"], tab["kdata"], conc,
                          pres, temp, 0)
    out.sum().backward()
    o = out.detach().numpy()[0, 0, :, 0]
    # below the table, inside the left cell, ON the inner knot (the right cell's slope),
    # inside the right cell, ON the last knot, above the table
    want = np.array([0.0, 0.1, 0.2, 0.2, 0.0, 0.0]) * o
    assert np.allclose(temp.grad.numpy()[0], want, rtol=1e-14, atol=0.0)
    assert (temp.grad.numpy()[0, [0, 4, 5]] == 0.0).all()
    assert (pres.grad.numpy() == 0.0).all()  # a one-knot axis clamps everywhere
    assert np.allclose(conc.grad.numpy()[0, :, 0], o, rtol=1e-15)


def test_band_optics_layer_without_extinction():
    rng = np.random.default_rng(51)
    tables = [t[:3] for t in _tables(rng)]
    x = _coords(rng, tables, 3)
    conc = torch.tensor(rng.uniform(0.1, 1.0, (1, 2, 3)))
    conc[0, 1] = 0.0
    conc.requires_grad_()
    dz = torch.tensor([[30.0, 70.0]], dtype=torch.float64, requires_grad=True)
    prop = ogr.band_optics(tables, conc, dz, 2, wavelength=x)
    assert (prop[:, 0, 1, :] == 0.0).all()
    prop[..., 1].sum().backward()  # through ssa alone: nothing from the empty layer
    assert (conc.grad[0, 1] == 0.0).all() and dz.grad[0, 1] == 0.0
    conc.grad, dz.grad = None, None
    prop = ogr.band_optics(tables, conc, dz, 2, wavelength=x)
    prop[..., 0].sum().backward()  # through tau: k_a dz per attenuator
    k = sum(float(harp_np.interp1(xx, t[0], t[1])[0]) for xx in x for t in tables if t[2] == 1)
    assert abs(conc.grad[0, 1, 1].item() - 70.0 * k) < 1e-12 * 70.0 * k
    assert conc.grad[0, 1, 0] == 0.0  # a species nobody reads


# ---- the library: no GPU needed, fails before this feature --------------------------------
BWD = ("hd_attenuate_bwd", "hd_band_optics_bwd", "hd_band_loop_optics_bwd",
       "hd_rfm_attenuate_bwd")


def test_header_declares_and_library_exports_the_adjoints():
    from pyharp_amd import _build, _lib
    with open(os.path.join(ROOT, "include", "hdharp.h")) as f:
        src = f.read()
    _build.build()
    lib = _lib.load()
    for name in BWD:
        assert name + "(" in src, name
        assert name in _lib.HARP_EXPORTED
        assert hasattr(lib, name), name
    assert "hd_harp_grad.hip" in _build.SOURCES


# ---- host-side refusals: before a device or the library is touched -------------------------
def _attenuator(tmp_path):
    from pyharp_amd.opacity import AttenuatorOptions, S8Fuller
    p = tmp_path / "s8.txt"
    p.write_text("# wl k ssa\n0.5 1.0 0.5\n1.0 2.0 0.6\n2.0 1.5 0.7\n")
    return S8Fuller(AttenuatorOptions().opacity_files([str(p)]).species_ids([0])
                    .species_weights([1.0]))


def _conc(requires_grad=True):
    return torch.full((2, 3, 1), 0.1, dtype=torch.float64, requires_grad=requires_grad)


def test_coordinate_requiring_grad_is_refused(tmp_path):
    from pyharp_amd.opacity import band_loop_optics, band_optics
    a = _attenuator(tmp_path)
    dz = torch.ones(3, dtype=torch.float64)
    wl = torch.tensor([0.7, 1.5], dtype=torch.float64, requires_grad=True)
    with pytest.raises(RuntimeError, match="wavelength requires grad"):
        a.forward(_conc(False), {"wavelength": wl})
    with pytest.raises(RuntimeError, match="wavenumber requires grad"):
        band_optics([a], _conc(), dz, {"wavenumber": wl})
    with pytest.raises(RuntimeError, match="wavelength requires grad"):
        band_loop_optics([a], _conc(), dz, {"wavelength": wl}, 4)


def test_out_with_an_input_that_requires_grad_is_refused(tmp_path):
    from pyharp_amd.opacity import band_loop_optics, band_optics
    from pyharp_amd.spectral import band_flux, band_flx, band_rad
    a = _attenuator(tmp_path)
    kw = {"wavelength": torch.tensor([0.7, 1.5], dtype=torch.float64)}
    dz = torch.ones(3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="out=.*requires grad"):
        band_optics([a], _conc(), dz, kw, out=torch.empty(2, 2, 3, 2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="out=.*requires grad"):
        band_optics([a], _conc(False), dz.clone().requires_grad_(), kw,
                    out=torch.empty(2, 2, 3, 2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="out=.*requires grad"):
        band_loop_optics([a], _conc(False), dz, kw, 0,
                         ext0=torch.ones(2, 2, 3, dtype=torch.float64, requires_grad=True),
                         out=torch.empty(2, 2, 3, 2, dtype=torch.float64))
    w = torch.ones(2, dtype=torch.float64)
    f = torch.ones(2, 2, 4, 2, dtype=torch.float64, requires_grad=True)
    for fn, x in ((band_flux, f), (band_rad, f),
                  (band_flx, torch.ones(2, 2, 4, 8, dtype=torch.float64, requires_grad=True))):
        with pytest.raises(RuntimeError, match="out=.*requires grad"):
            fn(x, w, out=torch.empty(tuple(x.shape[1:]), dtype=torch.float64))


def test_weights_requiring_grad_are_refused():
    from pyharp_amd.spectral import band_flux, band_flx, band_rad
    w = torch.ones(2, dtype=torch.float64, requires_grad=True)
    for fn, shape in ((band_flux, (2, 2, 4, 2)), (band_rad, (2, 5)), (band_flx, (2, 2, 4, 8))):
        with pytest.raises(RuntimeError, match="weights requires grad"):
            fn(torch.ones(shape, dtype=torch.float64), w)


def test_no_grad_and_plain_inputs_take_the_plain_path(monkeypatch, tmp_path):
    """nothing to differentiate: the calls reach today's device check, not a refusal and not
    an autograd Function"""
    from pyharp_amd import opacity, spectral
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for cls in (opacity._AttenuateGrad, opacity._BandOpticsGrad, opacity._BandLoopGrad,
                opacity._RfmGrad, spectral._BandSumGrad, spectral._HeatingGrad):
        monkeypatch.setattr(cls, "apply", lambda *a, **k: pytest.fail("the autograd path"))
    a = _attenuator(tmp_path)
    kw = {"wavelength": torch.tensor([0.7, 1.5], dtype=torch.float64)}
    dz = torch.ones(3, dtype=torch.float64)
    out = torch.empty(2, 2, 3, 2, dtype=torch.float64)
    rng = np.random.default_rng(1)
    tab = _rfm_table(rng)
    rfm = opacity.RFM.from_arrays(tab["wave"], np.exp(tab["lnp"]), tab["tgrid"], tab["tref"],
                                  tab["kdata"])
    st = {"pres": torch.full((2, 3), 1e4, dtype=torch.float64),
          "temp": torch.full((2, 3), 250.0, dtype=torch.float64, requires_grad=True)}
    with pytest.raises(RuntimeError, match="no HIP device"):
        opacity.band_optics([a], _conc(False), dz, kw, out=out)
    with pytest.raises(RuntimeError, match="no HIP device"):
        a.forward(_conc(False), kw)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="no HIP device"):
            opacity.band_optics([a], _conc(), dz, kw, out=out)
        with pytest.raises(RuntimeError, match="no HIP device"):
            opacity.band_loop_optics([a], _conc(), dz, kw, 0, out=out)
        with pytest.raises(RuntimeError, match="no HIP device"):
            rfm.forward(_conc(), st)
        with pytest.raises(RuntimeError, match="device"):
            spectral.band_flux(torch.ones(2, 2, 4, 2, dtype=torch.float64, requires_grad=True),
                               torch.ones(2), out=torch.empty(2, 4, 2, dtype=torch.float64))
        with pytest.raises(RuntimeError, match="device"):
            spectral.heating_rate(torch.ones(2, 4, 2, dtype=torch.float64, requires_grad=True),
                                  torch.ones(3), torch.ones(3), 1.0)
