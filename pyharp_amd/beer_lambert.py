"""Beer-Lambert solver on MI355X: fluxes and ray radiances of a purely absorbing,
emitting atmosphere (the reference's second RT solver, ``BeerLambert`` with its one
option ``alpha``, src/rtsolver/rtsolver.hpp:34-64; C-ABI include/hdbeer.h)::

    op = BeerLambertOptions().nstr(8).nwave(16).ncol(1).nlyr(40)
    op.planck(True).wave_lower([...]).wave_upper([...])
    solver = BeerLambert(op)
    flux = solver.forward(prop, bc, temf)                  # (nwave, ncol, nlyr+1, 2)
    bflux = solver.forward_band(prop, bc, temf, weights=w)  # (ncol, nlyr+1, 2)
    toa = solver.forward_rays(prop, bc, temf, umu=mu)       # (nwave, ncol, nray)
    btoa = solver.forward_rays_band(prop, bc, temf, umu=mu, weights=w)  # (ncol, nray)

``prop`` (nwave, ncol, nlyr, nprop >= 1) f64, layer 0 = bottom; ONLY slot 0 (the layer's
optical thickness) is read -- extinction is treated as absorption, whatever the
single-scattering albedo and phase moments say.  At ssa = 0 the results are those of
``Disort`` (the discrete-ordinate equations decouple), without its linear algebra.
``bc`` and ``temf`` as for ``Disort``; ``nstr`` is the order of the double-Gauss
quadrature the fluxes are summed with.  A ray's radiance emerges at the top for
``umu > 0`` and at the surface for ``umu < 0``; ``parse_radiation_directions`` supplies
``umu`` (its azimuths have no meaning without scattering).

The four methods are differentiable (hd_beer_flux_bwd / hd_beer_rays_bwd, the exact adjoint;
DESIGN.md section 3d "Gradients") in ``prop[..., 0]``, ``temf`` and the bc entries: with grad
mode on and one of them requiring grad the result carries a ``grad_fn``; otherwise the call
is the plain one, bit for bit.  ``umu``, ``weights`` and ``alpha`` are not differentiable,
and ``out=`` / ``flux=`` / ``rad=`` cannot be combined with an input that requires grad.

CPU tensors are staged with torch copies and the result comes back on the CPU; CUDA
tensors stay on the device.  There is no CPU path: without a HIP device or the built
library the calls raise.
"""

from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from . import _lib
from .disort import _BC_IGNORED, _BC_KEYS, _arg, _beam_hint, _context
from .rtsolver import RTSolver


def _ptr(t):
    return t.data_ptr() if t is not None else None


class BeerLambertOptions:
    alpha = _arg("alpha", 0.0)
    nstr = _arg("nstr", 8)
    nwave = _arg("nwave", 1)
    ncol = _arg("ncol", 1)
    nlyr = _arg("nlyr", 1)
    planck = _arg("planck", False)
    wave_lower = _arg("wave_lower", list)
    wave_upper = _arg("wave_upper", list)
    device = _arg("device", 0)

    def __repr__(self):
        return (f"BeerLambertOptions(alpha={self.alpha()}, nstr={self.nstr()}, "
                f"nwave={self.nwave()}, ncol={self.ncol()}, nlyr={self.nlyr()}, "
                f"planck={self.planck()})")


class BeerLambert(RTSolver):
    """MI355X Beer-Lambert module (hd_beer_flux / hd_beer_flux_band / hd_beer_rays)."""

    def __init__(self, options: Optional[BeerLambertOptions] = None):
        self.options = options if options is not None else BeerLambertOptions()
        self._waves = None
        self.reset()

    def reset(self):
        op = self.options
        nstr = op.nstr()
        if nstr < 2 or nstr % 2 or nstr > 32:
            raise RuntimeError(f"BeerLambert: nstr={nstr} must be even and in [2, 32]")
        if op.nlyr() < 1:
            raise RuntimeError(f"BeerLambert: nlyr={op.nlyr()} must be >= 1")
        alpha = float(op.alpha())
        if not math.isfinite(alpha) or alpha < 0.0:
            raise RuntimeError(f"BeerLambert: alpha={alpha} must be finite and >= 0")
        self.planck = bool(op.planck())
        if self.planck and (len(op.wave_lower()) != op.nwave()
                            or len(op.wave_upper()) != op.nwave()):
            raise RuntimeError("BeerLambert: planck needs wave_lower/wave_upper of size nwave")

    # ------------------------------------------------------------------ #
    def forward(self, prop: torch.Tensor, bc: Optional[Dict[str, torch.Tensor]] = None,
                temf: Optional[torch.Tensor] = None, *, status: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Fluxes (nwave, ncol, nlyr+1, 2): level 0 = surface, [..., 0] upward,
        [..., 1] direct + diffuse downward (``Disort.forward``'s layout)."""
        return self._run("forward", prop, bc, temf, status, out, None, None)

    def forward_band(self, prop: torch.Tensor, bc: Optional[Dict[str, torch.Tensor]] = None,
                     temf: Optional[torch.Tensor] = None, *, weights: torch.Tensor,
                     out: Optional[torch.Tensor] = None, flux: Optional[torch.Tensor] = None,
                     status: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The band flux (ncol, nlyr+1, 2) = sum_w weights[w] F_w, one fma per wave in
        wave order: bitwise equal to ``spectral.band_rad(forward(...), weights)``.
        Per-wave fluxes are stored only if ``flux`` is given."""
        return self._run("forward_band", prop, bc, temf, status, flux, None, (weights, out))

    def forward_rays(self, prop: torch.Tensor, bc: Optional[Dict[str, torch.Tensor]] = None,
                     temf: Optional[torch.Tensor] = None, *, umu: torch.Tensor,
                     out: Optional[torch.Tensor] = None,
                     status: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Emergent radiances (nwave, ncol, nray): ``umu`` float64 (nray,) -- shared -- or
        (ncol, nray) -- each column's own; at the top for umu > 0 (with the options'
        ``alpha`` term), at the surface for umu < 0.  A ray with umu = 0, |umu| > 1 or a
        non-finite umu is NaN and fails its column's solves (HD_STATUS_BAD_INPUT)."""
        return self._run("forward_rays", prop, bc, temf, status, out, umu, None)

    def forward_rays_band(self, prop: torch.Tensor,
                          bc: Optional[Dict[str, torch.Tensor]] = None,
                          temf: Optional[torch.Tensor] = None, *, umu: torch.Tensor,
                          weights: torch.Tensor, out: Optional[torch.Tensor] = None,
                          rad: Optional[torch.Tensor] = None,
                          status: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The band radiance (ncol, nray) = sum_w weights[w] rad_w (the legacy
        ``btoa(n) += wght[b] * toa(b, n)``), bitwise equal to
        ``spectral.band_rad(forward_rays(...), weights)``.  Per-wave radiances are stored
        only if ``rad`` (nwave, ncol, nray) is given."""
        return self._run("forward_rays_band", prop, bc, temf, status, rad, umu, (weights, out))

    # ------------------------------------------------------------------ #
    def _device_inputs(self, prop, bc, temf, dev):
        """(prop on dev, the given bc entries on dev as (nwave, ncol), hd_config,
        hd_inputs) of checked arguments; the tensors back the pointers of hd_inputs"""
        op = self.options
        f64 = torch.float64
        nwave, ncol, nlyr, nprop = prop.shape

        def dev_tensor(x, shape=None):
            t = torch.as_tensor(x, dtype=f64)
            if shape is not None and tuple(t.shape) != shape:
                t = t.expand(shape)
            return t.to(dev).contiguous()

        keep = [dev_tensor(prop)]
        bct = {k: dev_tensor(bc[k], (nwave, ncol)) for k in _BC_KEYS if bc.get(k) is not None}
        tf = wl = wu = None
        if self.planck:
            tf = dev_tensor(temf)
            # cached per device: no host->device copy per call (keeps the calls capturable
            # into a HIP graph once warmed up)
            key = (str(dev), tuple(op.wave_lower()), tuple(op.wave_upper()))
            if self._waves is None or self._waves[0] != key:
                self._waves = (key, torch.tensor(op.wave_lower(), dtype=f64, device=dev),
                               torch.tensor(op.wave_upper(), dtype=f64, device=dev))
            wl, wu = self._waves[1], self._waves[2]
            keep.append(tf)
        cfg = _lib.HdConfig(nstr=int(op.nstr()), nmom=0, nlyr=nlyr, nprop=nprop,
                            flags=_lib.HD_FLAG_LAMBER | _lib.HD_FLAG_ONLYFL |
                            (_lib.HD_FLAG_PLANCK if self.planck else 0))
        inp = _lib.HdInputs(nwave=nwave, ncol=ncol, prop=_ptr(keep[0]),
                            fbeam=_ptr(bct.get("fbeam")), umu0=_ptr(bct.get("umu0")),
                            albedo=_ptr(bct.get("albedo")), btemp=_ptr(bct.get("btemp")),
                            ttemp=_ptr(bct.get("ttemp")), temis=_ptr(bct.get("temis")),
                            fisot=_ptr(bct.get("fisot")), temf=_ptr(tf), wave_lower=_ptr(wl),
                            wave_upper=_ptr(wu))
        return keep, bct, cfg, inp

    def _wants_grad(self, who, prop, bc, temf, umu, band, vals):
        """True if the call is to be differentiated: grad mode on and a differentiable
        input requires grad.  Raises for what cannot be served."""
        if not torch.is_grad_enabled():
            return False

        def req(x):
            return isinstance(x, torch.Tensor) and x.requires_grad

        if req(umu):
            raise RuntimeError(f"{who}: umu requires grad, but the view angles are not "
                               "differentiable (detach umu)")
        if band is not None and req(band[0]):
            raise RuntimeError(f"{who}: weights requires grad, but the band weights are not "
                               "differentiable (detach weights)")
        if not (req(prop) or (self.planck and req(temf)) or any(req(bc.get(k)) for k in _BC_KEYS)):
            return False
        if vals is not None or (band is not None and band[1] is not None):
            raise RuntimeError(f"{who}: out=, flux= and rad= cannot be combined with an input "
                               "that requires grad (autograd owns the result)")
        return True

    def _run(self, name, prop, bc, temf, status, vals, umu, band):
        """vals: the caller's per-wave output or None; umu None: fluxes; band: (weights,
        the caller's band output or None) or None."""
        who = "BeerLambert." + name
        op = self.options
        f64 = torch.float64
        rays = umu is not None
        bc = {} if bc is None else bc
        # --- host-side checks, before a device or the library is touched ---
        if not isinstance(prop, torch.Tensor) or prop.dim() != 4:
            raise RuntimeError(f"{who}: prop must be (nwave, ncol, nlyr, nprop)")
        nwave, ncol, nlyr, nprop = prop.shape
        if nlyr != op.nlyr():
            raise RuntimeError(f"{who}: prop has {nlyr} layers, options.nlyr() = {op.nlyr()}")
        if nprop < 1:
            raise RuntimeError(f"{who}: prop needs at least the optical thickness (nprop >= 1)")
        for k in bc:
            if k not in _BC_KEYS and k not in _BC_IGNORED:
                raise RuntimeError(f"{who}: unknown boundary condition '{k}'")
        for k in _BC_KEYS:
            if bc.get(k) is not None:
                shp = tuple(torch.as_tensor(bc[k]).shape)
                try:
                    ok = torch.broadcast_shapes(shp, (nwave, ncol)) == (nwave, ncol)
                except RuntimeError:
                    ok = False
                if not ok:
                    raise RuntimeError(f"{who}: bc['{k}'] {shp} must be (nwave, ncol) = "
                                       f"{(nwave, ncol)}")
        if self.planck and temf is None:
            raise RuntimeError(f"{who}: planck set but temf not given")
        if self.planck and not (nwave == len(op.wave_lower()) == len(op.wave_upper())):
            raise RuntimeError(f"{who}: planck: prop has {nwave} waves but wave_lower/"
                               f"wave_upper hold {len(op.wave_lower())}/{len(op.wave_upper())}")
        if self.planck and tuple(torch.as_tensor(temf).shape) != (ncol, nlyr + 1):
            raise RuntimeError(f"{who}: temf must be (ncol, nlyr+1) = {(ncol, nlyr + 1)}, got "
                               f"{tuple(torch.as_tensor(temf).shape)}")
        alpha = float(op.alpha())
        if not rays and alpha != 0.0:
            raise RuntimeError(f"{who}: alpha = {alpha} applies to ray radiances only; the flux "
                               "calls need alpha = 0")
        if rays:
            if not isinstance(umu, torch.Tensor) or umu.dtype != f64:
                raise RuntimeError(f"{who}: umu must be a float64 tensor")
            if umu.dim() not in (1, 2) or umu.shape[-1] < 1 or \
                    (umu.dim() == 2 and umu.shape[0] != ncol):
                raise RuntimeError(f"{who}: umu must be (nray,) or (ncol, nray) = ({ncol}, nray), "
                                   f"got {tuple(umu.shape)}")
        if band is not None:
            wts = torch.as_tensor(band[0], dtype=f64).reshape(-1)
            if wts.numel() != nwave:
                raise RuntimeError(f"{who}: {wts.numel()} weights for {nwave} waves")
        grad = self._wants_grad(who, prop, bc, temf, umu, band, vals)
        if not torch.cuda.is_available():
            raise RuntimeError(f"{who}: no HIP device available (pyharp_amd has no CPU path)")
        if grad:
            return _beer_grad_call(self, name, prop, bc, temf, status, umu, band)
        # --- staging ---
        in_dev = prop.device
        dev = in_dev if in_dev.type == "cuda" else torch.device("cuda", int(op.device()))
        keep, bct, cfg, inp = self._device_inputs(prop, bc, temf, dev)
        tail = (umu.shape[-1],) if rays else (nlyr + 1, 2)
        ptr = _ptr

        def given(t, shape, what):
            if t is not None and (t.device != dev or t.dtype != f64 or not t.is_contiguous()
                                  or tuple(t.shape) != shape):
                raise RuntimeError(f"{who}: {what} must be a contiguous float64 tensor of "
                                   f"shape {shape} on {dev}")
            return t

        vname = "out" if band is None else ("rad" if rays else "flux")
        vals = given(vals, (nwave, ncol) + tail, vname)
        if status is not None and (status.device != dev or status.dtype != torch.int32
                                   or not status.is_contiguous()
                                   or status.numel() < nwave * ncol):
            raise RuntimeError(f"{who}: status must be a contiguous int32 tensor of "
                               f">= {nwave * ncol} elements on {dev}")
        bout = None
        if band is not None:
            bout = given(band[1], (ncol,) + tail, "out")
            if bout is None:
                bout = torch.empty((ncol,) + tail, dtype=f64, device=dev)
            wts = wts.to(dev).contiguous()
        elif vals is None:
            vals = torch.empty((nwave, ncol) + tail, dtype=f64, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        ctx = _context(dev.index)
        try:
            with torch.cuda.device(dev):
                if rays:
                    mu_d = umu.to(dev).contiguous()
                    r = _lib.HdBeerRays(nray=tail[0], per_column=int(umu.dim() == 2),
                                        umu=mu_d.data_ptr(), alpha=alpha,
                                        weight=ptr(wts) if band is not None else None,
                                        brad=ptr(bout))
                    ctx.beer_rays(cfg, inp, r, ptr(vals), ptr(status), stream)
                elif band is not None:
                    hb = _lib.HdBand(weight=wts.data_ptr(), bflux=bout.data_ptr())
                    ctx.beer_flux_band(cfg, inp, hb, ptr(vals), ptr(status), stream)
                else:
                    ctx.beer_flux(cfg, inp, vals.data_ptr(), ptr(status), stream)
        except RuntimeError as err:
            if "at least one solve failed" in str(err) and _beam_hint(bc):
                raise RuntimeError(str(err) + _beam_hint(bc)) from err
            raise
        del keep, bct
        res = bout if band is not None else vals
        return res.to(in_dev) if in_dev.type != "cuda" else res


# ---------------------------------------------------------------------- #
# gradients (hd_beer_flux_bwd / hd_beer_rays_bwd)
# ---------------------------------------------------------------------- #
def _beer_grad_call(solver, name, prop, bc, temf, status, umu, band):
    """The call through autograd.  The optical depth enters as the slot-0 view of prop
    and the bc entries expanded to (nwave, ncol), both by differentiable torch ops: the
    gradient of a broadcast entry is summed, and that of prop's other slots zeroed, by
    torch."""
    nwave, ncol = prop.shape[:2]
    bcs = [None if bc.get(k) is None else
           torch.as_tensor(bc[k], dtype=torch.float64).expand(nwave, ncol) for k in _BC_KEYS]
    tf = torch.as_tensor(temf, dtype=torch.float64) if solver.planck else None
    wts = None if band is None else torch.as_tensor(band[0], dtype=torch.float64).reshape(-1)
    return _BeerGrad.apply(solver, name, prop.detach(), status, umu, wts, prop[..., 0], tf, *bcs)


class _BeerGrad(torch.autograd.Function):
    """forward: BeerLambert._run as without autograd; backward: one library call."""

    @staticmethod
    def forward(ctx, solver, name, prop, status, umu, wts, tau, temf, *bcs):
        bc = {k: v for k, v in zip(_BC_KEYS, bcs) if v is not None}
        res = solver._run(name, prop, bc, temf, status, None, umu,
                          None if wts is None else (wts, None))
        ctx.solver, ctx.status = solver, status
        ctx.save_for_backward(prop, umu, wts, temf, *bcs)
        return res

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        solver = ctx.solver
        prop, umu, wts, temf, *bcs = ctx.saved_tensors
        bc = {k: v for k, v in zip(_BC_KEYS, bcs) if v is not None}
        nwave, ncol, nlyr, _ = prop.shape
        f64 = torch.float64
        in_dev = prop.device
        dev = in_dev if in_dev.type == "cuda" else torch.device("cuda", int(solver.options.device()))
        keep, bct, cfg, inp = solver._device_inputs(prop, bc, temf, dev)
        need = dict(zip(("gtau", "gtemf") + tuple("g_" + k for k in _BC_KEYS),
                        ctx.needs_input_grad[6:]))
        shapes = {"gtau": (nwave, ncol, nlyr), "gtemf": (ncol, nlyr + 1)}
        out = {}
        for k, wanted in need.items():
            if not wanted or (not solver.planck and k in ("gtemf", "g_btemp", "g_ttemp")):
                continue  # (without emission the temperatures are not read: no gradient)
            out[k] = torch.empty(shapes.get(k, (nwave, ncol)), dtype=f64, device=dev)
        g_dev = gout.to(device=dev, dtype=f64).contiguous()
        if wts is None:
            cot = _lib.HdBeerCot(per_wave=g_dev.data_ptr())
        else:
            wts_d = wts.to(dev).contiguous()
            cot = _lib.HdBeerCot(band=g_dev.data_ptr(), weight=wts_d.data_ptr())
        grads = _lib.HdBeerGrads(**{k: v.data_ptr() for k, v in out.items()})
        # the bits of the backward go to the caller's status beside the forward's; without
        # one a solve the forward accepted cannot fail here
        st = torch.empty(nwave * ncol, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        hctx = _context(dev.index)
        with torch.cuda.device(dev):
            if umu is not None:
                mu_d = umu.to(dev).contiguous()
                r = _lib.HdBeerRays(nray=umu.shape[-1], per_column=int(umu.dim() == 2),
                                    umu=mu_d.data_ptr(), alpha=float(solver.options.alpha()))
                hctx.beer_rays_bwd(cfg, inp, r, cot, grads, st.data_ptr(), stream)
            else:
                hctx.beer_flux_bwd(cfg, inp, cot, grads, st.data_ptr(), stream)
        if ctx.status is not None:
            ctx.status.view(-1)[:nwave * ncol] |= st
        del keep, bct
        res = [out.get(k) for k in need]
        res = [g if g is None or in_dev.type == "cuda" else g.to(in_dev) for g in res]
        return (None,) * 6 + tuple(res)
