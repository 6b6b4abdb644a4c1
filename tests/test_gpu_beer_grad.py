"""Gradients of the HIP Beer-Lambert solver (hd_beer_flux_bwd / hd_beer_rays_bwd through
pyharp_amd.BeerLambert and torch autograd): parity with the float64 torch reference
(tests/beer_grad_ref.py, pinned on the CPU by tests/test_beer_grad_ref.py independently of
the kernels), bitwise properties, exact cases, status bits and CPU tensors.  The judge is
the CPU reference: no finite differences of the GPU against itself, no gradcheck.

Bounds.  The error of a gradient tensor is taken relative to its largest component in
the column.  Against the reference the project's TOL = 1e-6 and, beside it, TIGHT: the
same formulas in the same precision, so what remains is rounding -- ten times the worst
error of the first GPU run (MEASURED, recorded in profiles/beer_grad/parity_margins.json),
capped at 1e-9.
"""

import numpy as np
import pytest
import torch

import beer_grad_ref
from helpers import TOL, margin
from test_gpu_beer import _beer, _case, _ref_kw

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
MEASURED = 1.258e-11  # worst error against beer_grad_ref in the first GPU run (a column of one
# solve under e^-16000: d/dfisot of a band ray radiance, nstr 32, nlyr 33)
TIGHT = min(1.0e-9, 10.0 * MEASURED)
BAD = 0x01
BC = ("fbeam", "umu0", "albedo", "btemp", "ttemp", "temis", "fisot")
UMU_SHARED = np.array([-1.0, -0.3, 0.02, 0.37, 1.0])


def _leaf(x, dev=DEV):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev,
                        requires_grad=True)


def _grad_case(rng, nwave, ncol, nlyr, nprop, planck, alpha=0.0):
    """_case with the regimes of the adjoint: slant thicknesses on both sides of the series
    switch, an exactly empty and a tau = 50 layer, albedo 0 / 0.3 / 1, the beam off and on
    with mu0 = 1 and 0.1"""
    prop, bc, kw = _case(rng, nwave, ncol, nlyr, nprop, planck)
    tau = prop[..., 0].reshape(nwave * ncol, nlyr)
    tau[5, nlyr - 1] = 50.0
    if nlyr > 1 or alpha == 0.0:  # (alpha with an empty column is a bad input)
        tau[3, 0] = 0.0
    prop[..., 0] = tau.reshape(nwave, ncol, nlyr)
    for k, every, vals in (("albedo", 4, (0.0, 0.3, 1.0)), ("umu0", 5, (1.0, 0.1))):
        flat = bc[k].reshape(-1)
        for i, v in enumerate(vals):
            flat[i::every] = v
    bc["fbeam"].reshape(-1)[::3] = 0.0
    return prop, bc, kw


def _per_column_umu(rng, ncol):
    umu = np.where(rng.uniform(size=(ncol, 5)) < 0.5, -1.0, 1.0) * rng.uniform(0.02, 1.0, (ncol, 5))
    umu[0] = [1.0, -1.0, 0.02, -0.02, 0.5]
    return umu


def _run(fn, prop, bc, temf, cot, dev=DEV, **kws):
    """(result, {input: gradient}) of fn with every differentiable input a leaf; the tau
    leaf enters prop's slot 0"""
    tau = _leaf(prop[..., 0], dev)
    rest = torch.as_tensor(prop[..., 1:], dtype=torch.float64, device=dev)
    leaves = {k: _leaf(v, dev) for k, v in bc.items()}
    tf = _leaf(temf, dev) if temf is not None else None
    out = fn(torch.cat([tau[..., None], rest], dim=-1), leaves, tf, **kws)
    out.backward(torch.as_tensor(cot, dtype=torch.float64, device=out.device))
    grads = {"tau": tau.grad, **{k: v.grad for k, v in leaves.items()}}
    if tf is not None:
        grads["temf"] = tf.grad
    return out.detach(), grads


def _col_err(got, ref, name):
    """max |got - ref| over the largest |ref| of the tensor in the column"""
    got, ref = np.asarray(got), np.asarray(ref)
    axes = {"tau": (0, 2), "temf": (1,)}.get(name, (0,))
    scale = np.abs(ref).max(axis=axes, keepdims=True)
    return (np.abs(got - ref) / np.maximum(scale, 1e-300)).max()


def _compare(tag, got, ref):
    worst = 0.0
    for k, g in ref.items():
        assert got[k] is not None, (tag, k)
        err = _col_err(got[k].cpu().numpy(), g.numpy(), k)
        print(f"beer grad {tag} d/d{k}: {err:.3e}")
        worst = max(worst, err)
    return worst


# --- 1: parity with the reference -------------------------------------------------------
@pytest.mark.parametrize("layout", ["67x1", "1x67"])
@pytest.mark.parametrize("nlyr", [1, 3, 17, 33])
@pytest.mark.parametrize("nstr", [2, 8, 16, 32])
def test_parity_with_reference(nstr, nlyr, layout):
    """67 solves (one wave and three lanes) as 67 waves x 1 column and 1 wave x 67 columns;
    nprop 1 without emission and shared rays, nprop 6 with emission, per-column rays and
    alpha = 0.7; nlyr 17 and 33 cross the 16-layer tile once and twice; all four calls,
    every differentiable input requiring grad at once"""
    nwave, ncol = (67, 1) if layout == "67x1" else (1, 67)
    worst = 0.0
    for nprop, planck, alpha in ((1, False, 0.0), (6, True, 0.7)):
        rng = np.random.default_rng(9100 + 100 * nstr + nlyr + 7 * planck)
        prop, bc, kw = _grad_case(rng, nwave, ncol, nlyr, nprop, planck, alpha)
        opts = dict(planck=planck, wl=kw.get("wave_lower"), wu=kw.get("wave_upper"))
        b, br = _beer(nstr, nlyr, nwave, ncol, **opts), _beer(nstr, nlyr, nwave, ncol, alpha=alpha, **opts)
        umu = _per_column_umu(rng, ncol) if planck else UMU_SHARED
        w = rng.uniform(0.1, 2.0, nwave)
        temf = kw.get("temf")
        rkw = dict(nstr=nstr, **_ref_kw(kw))
        cpu = torch.device("cpu")
        wsum = lambda x: (torch.as_tensor(w).reshape((-1,) + (1,) * (x.dim() - 1)) * x).sum(0)  # noqa: E731
        ref_flux = lambda *a: beer_grad_ref.beer_flux(*a, **rkw)  # noqa: E731
        ref_rays = lambda *a: beer_grad_ref.beer_rays(*a, umu=umu, alpha=alpha, **rkw)  # noqa: E731
        calls = (
            ("forward", b.forward, {}, ref_flux, (nwave, ncol, nlyr + 1, 2)),
            ("forward_band", b.forward_band, dict(weights=torch.as_tensor(w, device=DEV)),
             lambda *a: wsum(ref_flux(*a)), (ncol, nlyr + 1, 2)),
            ("forward_rays", br.forward_rays, dict(umu=torch.as_tensor(umu, device=DEV)), ref_rays,
             (nwave, ncol, 5)),
            ("forward_rays_band", br.forward_rays_band,
             dict(umu=torch.as_tensor(umu, device=DEV), weights=torch.as_tensor(w, device=DEV)),
             lambda *a: wsum(ref_rays(*a)), (ncol, 5)))
        for name, fn, kws, ref_fn, shape in calls:
            cot = rng.uniform(-1.0, 1.0, shape)  # the loss: a fixed cotangent dotted into the result
            out, got = _run(fn, prop, bc, temf, cot, **kws)
            rout, ref = _run(ref_fn, prop, bc, temf, cot, dev=cpu)
            assert tuple(out.shape) == shape
            fwd = (np.abs(out.cpu().numpy() - rout.numpy()).max() / np.abs(rout.numpy()).max())
            assert fwd < 1e-12, (name, fwd)
            worst = max(worst, _compare(f"nstr={nstr} nlyr={nlyr} {layout} planck={planck} {name}",
                                        got, ref))
    print(f"beer grad parity nstr={nstr} nlyr={nlyr} {layout}: worst {worst:.3e}")
    assert margin(worst) < TOL
    assert worst < TIGHT, worst


# --- 2: bits ----------------------------------------------------------------------------
def _bit_case():
    nstr, nlyr, nwave, ncol = 8, 5, 67, 3
    rng = np.random.default_rng(9200)
    prop, bc, kw = _grad_case(rng, nwave, ncol, nlyr, 2, True)
    b = _beer(nstr, nlyr, nwave, ncol, planck=True, wl=kw["wave_lower"], wu=kw["wave_upper"])
    umu = torch.as_tensor(_per_column_umu(rng, ncol), device=DEV)
    w = torch.as_tensor(rng.uniform(0.1, 2.0, nwave), device=DEV)
    return rng, prop, bc, kw, b, umu, w


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_forward_of_a_differentiated_call_is_the_plain_call():
    rng, prop, bc, kw, b, umu, w = _bit_case()
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64, device=DEV)  # noqa: E731
    plain = (t(prop), {k: t(v) for k, v in bc.items()}, t(kw["temf"]))
    for name, kws, shape in (("forward", {}, (67, 3, 6, 2)), ("forward_band", dict(weights=w), (3, 6, 2)),
                             ("forward_rays", dict(umu=umu), (67, 3, 5)),
                             ("forward_rays_band", dict(umu=umu, weights=w), (3, 5))):
        want = getattr(b, name)(*plain, **kws)
        assert want.grad_fn is None
        out, _ = _run(getattr(b, name), prop, bc, kw["temf"], np.ones(shape), **kws)
        assert torch.equal(out, want), name
        leaf = plain[0].clone().requires_grad_(True)
        with torch.no_grad():
            assert getattr(b, name)(leaf, plain[1], plain[2], **kws).grad_fn is None


def test_chunked_and_repeated_gradients_are_bitwise_equal():
    """67 x 3 solves unchunked, in chunks of 40 (which start inside a wave and inside a
    column's waves) and of 1 000; gtemf sums over the waves of a column in wave order
    through memory, so it too is the same to the bit; and a second run repeats the first"""
    from pyharp_amd.disort import _context
    rng, prop, bc, kw, b, umu, w = _bit_case()
    calls = (("forward", {}, (67, 3, 6, 2)), ("forward_rays", dict(umu=umu), (67, 3, 5)),
             ("forward_band", dict(weights=w), (3, 6, 2)))
    ctx = _context(0)
    for name, kws, shape in calls:
        cot = rng.uniform(-1.0, 1.0, shape)
        _, one = _run(getattr(b, name), prop, bc, kw["temf"], cot, **kws)
        _, two = _run(getattr(b, name), prop, bc, kw["temf"], cot, **kws)
        assert _same(one, two), name
        assert all(torch.isfinite(g).all() for g in one.values()), name
        for chunk in (40, 1000):
            ctx.set_chunk(chunk)
            try:
                _, got = _run(getattr(b, name), prop, bc, kw["temf"], cot, **kws)
            finally:
                ctx.set_chunk(0)
            assert _same(got, one), (name, chunk)


def test_band_gradient_is_the_per_wave_gradient_of_the_weighted_cotangent():
    rng, prop, bc, kw, b, umu, w = _bit_case()
    for band, plain, kws, shape in (("forward_band", "forward", {}, (3, 6, 2)),
                                    ("forward_rays_band", "forward_rays", dict(umu=umu), (3, 5))):
        gband = rng.uniform(-1.0, 1.0, shape)
        _, got = _run(getattr(b, band), prop, bc, kw["temf"], gband, weights=w, **kws)
        per_wave = w.cpu().numpy().reshape((-1,) + (1,) * len(shape)) * gband[None]
        _, want = _run(getattr(b, plain), prop, bc, kw["temf"], per_wave, **kws)
        assert _same(got, want), band


# --- 3: exact cases ---------------------------------------------------------------------
def test_empty_column_gradients():
    """every tau = 0: nothing is emitted on the way, so the interior levels' temperatures
    have no gradient, exactly; the boundary gradients are the reference's closed forms (with
    sum w mu = 1/2: dF_up/dalbedo = F_down - pi B(btemp), dF_up/dfisot = pi albedo, ...)"""
    nstr, nlyr, nwave, ncol = 8, 19, 2, 3
    rng = np.random.default_rng(9300)
    prop, bc, kw = _case(rng, nwave, ncol, nlyr, 3, True)
    prop[..., 0] = 0.0
    b = _beer(nstr, nlyr, nwave, ncol, planck=True, wl=kw["wave_lower"], wu=kw["wave_upper"])
    cot = rng.uniform(0.1, 1.0, (nwave, ncol, nlyr + 1, 2))  # (one sign: sums without cancellation)
    _, got = _run(b.forward, prop, bc, kw["temf"], cot)
    _, ref = _run(lambda *a: beer_grad_ref.beer_flux(*a, nstr=nstr, **_ref_kw(kw)), prop, bc,
                  kw["temf"], cot, dev=torch.device("cpu"))
    assert (got["temf"].cpu().numpy() == 0.0).all()
    assert (ref["temf"].numpy() == 0.0).all()
    for k in BC:
        err = _col_err(got[k].cpu().numpy(), ref[k].numpy(), k)
        print("empty column d/d" + k, err)
        assert err < 1e-14, (k, err)
    # the closed form of one of them, from the cotangents alone
    alb = bc["albedo"]
    want = np.pi * (cot[..., 1].sum(-1) + alb * cot[..., 0].sum(-1))  # dL/dfisot
    assert np.abs(got["fisot"].cpu().numpy() / want - 1.0).max() < 1e-14


def test_black_surface_without_beam_has_no_albedo_partner_gradients():
    """albedo = 0 and no beam: nothing downward reaches the upward fluxes, so an upward
    cotangent leaves fisot, ttemp, temis and the beam without gradient, exactly"""
    nstr, nlyr, nwave, ncol = 4, 6, 2, 3
    rng = np.random.default_rng(9310)
    prop, bc, kw = _case(rng, nwave, ncol, nlyr, 1, True)
    bc["albedo"][:] = 0.0
    bc["fbeam"][:] = 0.0
    b = _beer(nstr, nlyr, nwave, ncol, planck=True, wl=kw["wave_lower"], wu=kw["wave_upper"])
    cot = np.zeros((nwave, ncol, nlyr + 1, 2))
    cot[..., 0] = rng.uniform(0.1, 1.0, (nwave, ncol, nlyr + 1))
    _, got = _run(b.forward, prop, bc, kw["temf"], cot)
    for k in ("fisot", "ttemp", "temis", "fbeam", "umu0"):
        assert (got[k] == 0.0).all(), k
    assert (got["btemp"] > 0.0).all() and (got["albedo"] != 0.0).all()


# --- 4: status --------------------------------------------------------------------------
def test_bad_inputs_get_nan_gradients_and_their_neighbours_none():
    """the forward's own bad-input cases: tau < 0 in one solve, mu0 = 2 in another"""
    nstr, nlyr, nwave, ncol = 4, 3, 3, 5
    rng = np.random.default_rng(9400)
    prop, bc, kw = _case(rng, nwave, ncol, nlyr, 2, True)
    b = _beer(nstr, nlyr, nwave, ncol, planck=True, wl=kw["wave_lower"], wu=kw["wave_upper"])
    umu = torch.as_tensor(UMU_SHARED, device=DEV)
    prop2 = prop.copy()
    prop2[1, 2, 1, 0] = -0.1
    bc2 = {k: v.copy() for k, v in bc.items()}
    bc2["umu0"][0, 3] = 2.0
    bad = np.zeros((nwave, ncol), dtype=bool)
    bad[1, 2] = bad[0, 3] = True
    for name, kws, shape in (("forward", {}, (nwave, ncol, nlyr + 1, 2)),
                             ("forward_rays", dict(umu=umu), (nwave, ncol, 5))):
        cot = rng.uniform(-1.0, 1.0, shape)
        _, ref = _run(getattr(b, name), prop, bc, kw["temf"], cot, **kws)
        st = torch.zeros(nwave * ncol, dtype=torch.int32, device=DEV)
        tau = _leaf(prop2[..., 0])
        leaves = {k: _leaf(v) for k, v in bc2.items()}
        tf = _leaf(kw["temf"])
        out = getattr(b, name)(torch.stack([tau, torch.as_tensor(prop2[..., 1], device=DEV)], -1),
                               leaves, tf, status=st, **kws)
        assert np.array_equal(st.cpu().numpy().reshape(nwave, ncol) & BAD, bad * BAD)
        st.zero_()  # what follows is the backward's own
        out.backward(torch.as_tensor(cot, device=DEV))
        assert np.array_equal(st.cpu().numpy().reshape(nwave, ncol) & BAD, bad * BAD), name
        for k, g in [("tau", tau.grad)] + [(k, v.grad) for k, v in leaves.items()]:
            g, r = g.cpu().numpy(), ref[k].cpu().numpy()
            assert np.isnan(g[bad]).all(), (name, k)
            assert np.array_equal(g[~bad], r[~bad]), (name, k)
        # temf sums over the waves of a column: NaN in the bad solves' columns only
        g, r = tf.grad.cpu().numpy(), ref["temf"].cpu().numpy()
        cols = bad.any(axis=0)
        assert np.isnan(g[cols]).all() and np.array_equal(g[~cols], r[~cols]), name


# --- 5: CPU tensors ---------------------------------------------------------------------
def test_cpu_tensors_round_trip_with_gradients():
    nstr, nlyr, nwave, ncol = 8, 7, 3, 4
    rng = np.random.default_rng(9500)
    prop, bc, kw = _grad_case(rng, nwave, ncol, nlyr, 2, True)
    b = _beer(nstr, nlyr, nwave, ncol, planck=True, wl=kw["wave_lower"], wu=kw["wave_upper"])
    w = rng.uniform(0.1, 1.0, nwave)
    cpu = torch.device("cpu")
    for name, kws, shape in (("forward", {}, (nwave, ncol, nlyr + 1, 2)),
                             ("forward_rays_band", dict(umu=UMU_SHARED, weights=w), (ncol, 5))):
        cot = rng.uniform(-1.0, 1.0, shape)
        on = lambda d: {k: torch.as_tensor(v, device=d) for k, v in kws.items()}  # noqa: E731
        out_d, on_dev = _run(getattr(b, name), prop, bc, kw["temf"], cot, **on(DEV))
        out_c, on_cpu = _run(getattr(b, name), prop, bc, kw["temf"], cot, dev=cpu, **on(cpu))
        assert out_c.device.type == "cpu" and torch.equal(out_c, out_d.cpu())
        for k, g in on_cpu.items():
            assert g.device.type == "cpu" and torch.equal(g, on_dev[k].cpu()), (name, k)


def test_broadcast_boundary_conditions_and_prop_leaf():
    """a scalar and an (ncol,) bc entry get their summed gradient, and prop itself as the
    leaf gets the tau gradient in slot 0 and zeros elsewhere, both from torch"""
    nstr, nlyr, nwave, ncol = 4, 3, 3, 4
    rng = np.random.default_rng(9510)
    prop, bc, kw = _case(rng, nwave, ncol, nlyr, 3, False)
    bc["albedo"][:] = 0.25
    bc["fisot"][:] = bc["fisot"][:1]
    b = _beer(nstr, nlyr, nwave, ncol)
    cot = rng.uniform(-1.0, 1.0, (nwave, ncol, nlyr + 1, 2))
    _, full = _run(b.forward, prop, bc, None, cot)
    p = _leaf(prop)
    alb = torch.tensor(0.25, dtype=torch.float64, device=DEV, requires_grad=True)
    fis = _leaf(bc["fisot"][0])
    bcs = {k: torch.as_tensor(v, device=DEV) for k, v in bc.items()}
    bcs.update(albedo=alb, fisot=fis)
    b.forward(p, bcs).backward(torch.as_tensor(cot, device=DEV))
    assert torch.equal(p.grad[..., 0], full["tau"]) and (p.grad[..., 1:] == 0.0).all()
    assert alb.grad.shape == () and fis.grad.shape == (ncol,)
    assert torch.allclose(alb.grad, full["albedo"].sum(), rtol=1e-13, atol=0.0)
    assert torch.allclose(fis.grad, full["fisot"].sum(0), rtol=1e-13, atol=0.0)


# --- 6: the C-ABI's argument checks -------------------------------------------------------
def test_c_abi_refuses_ambiguous_cotangents_and_temperatures_without_planck():
    from pyharp_amd import _lib
    from pyharp_amd.disort import _context
    nwave, ncol, nlyr = 2, 3, 4
    t = lambda *s: torch.zeros(*s, dtype=torch.float64, device=DEV)  # noqa: E731
    prop, per_wave, band, w = t(nwave, ncol, nlyr, 1), t(nwave, ncol, nlyr + 1, 2), t(ncol, nlyr + 1, 2), t(nwave)
    gtau, gtemf, galb = t(nwave, ncol, nlyr), t(ncol, nlyr + 1), t(nwave, ncol)
    cfg = _lib.HdConfig(nstr=4, nmom=0, nlyr=nlyr, nprop=1,
                        flags=_lib.HD_FLAG_LAMBER | _lib.HD_FLAG_ONLYFL)
    inp = _lib.HdInputs(nwave=nwave, ncol=ncol, prop=prop.data_ptr())
    ctx = _context(0)
    ok = _lib.HdBeerGrads(gtau=gtau.data_ptr())
    for cot in (_lib.HdBeerCot(), _lib.HdBeerCot(per_wave=per_wave.data_ptr(), band=band.data_ptr(),
                                                 weight=w.data_ptr()),
                _lib.HdBeerCot(band=band.data_ptr()), _lib.HdBeerCot(weight=w.data_ptr())):
        with pytest.raises(RuntimeError, match="invalid argument.*either per_wave or band"):
            ctx.beer_flux_bwd(cfg, inp, cot, ok, None, None)
    good = _lib.HdBeerCot(per_wave=per_wave.data_ptr())
    with pytest.raises(RuntimeError, match="need HD_FLAG_PLANCK"):
        ctx.beer_flux_bwd(cfg, inp, good, _lib.HdBeerGrads(gtemf=gtemf.data_ptr()), None, None)
    with pytest.raises(RuntimeError, match="needs that boundary input"):
        ctx.beer_flux_bwd(cfg, inp, good, _lib.HdBeerGrads(g_albedo=galb.data_ptr()), None, None)
    ctx.beer_flux_bwd(cfg, inp, good, ok, None, None)  # all tau = 0, zero cotangent
    torch.cuda.synchronize()
    assert (gtau == 0.0).all()
