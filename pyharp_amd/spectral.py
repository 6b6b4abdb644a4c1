"""Spectral (g-point) sharding of a correlated-k band over ranks, and the band
epilogue after the solve (band flux, heating rate, spherical correction).

pyharp sums the per-g fluxes of a band with the ck weights after the solve
(examples/amars_lw.cpp:84-88: ``bflx = (flux * weights.view({-1,1,1,1})).sum(0)``;
legacy accumulation src/rtsolver/rt_solver_disort.cpp_:268-271).  With the
g-points of a band spread over ranks, each rank solves its own g-points and the
band flux is completed by ONE all-reduce (sum) of the weighted partial band
flux (ncol, nlyr+1, 2) -- the only exchange step of the path (RCCL over xGMI
with the "nccl" backend; gloo on CPU in the tests).
"""

from __future__ import annotations

import ctypes
from typing import List, Optional

import torch

from . import _lib


def shard_gpoints(ngpoint: int, world: int, rank: int) -> List[int]:
    """g-points owned by `rank`: {g : g mod world == rank} (round-robin)."""
    if not 0 <= rank < world:
        raise ValueError(f"rank {rank} outside world {world}")
    return [g for g in range(ngpoint) if g % world == rank]


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _dev_f64(t: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise RuntimeError(f"{what}: expects a device (HIP) tensor -- pyharp_amd has no CPU path")
    return t.to(torch.float64).contiguous()


def _req(x) -> bool:
    return isinstance(x, torch.Tensor) and x.requires_grad


def _wants_grad(who, weights, inputs, out=None) -> bool:
    """True if the call is to be differentiated: grad mode on and a differentiable
    input requires grad.  Raises for what cannot be served."""
    if not torch.is_grad_enabled():
        return False
    if _req(weights):
        raise RuntimeError(f"{who}: weights requires grad, but the band weights are not "
                           "differentiable (detach weights)")
    if not any(_req(x) for x in inputs):
        return False
    if out is not None:
        raise RuntimeError(f"{who}: out= cannot be combined with an input that requires grad "
                           "(autograd owns the result)")
    return True


class _BandSumGrad(torch.autograd.Function):
    """forward: band_flux / band_flx / band_rad as without autograd; backward:
    weights (x) g, elementwise (no reduction: torch ops, no kernel of its own)."""

    @staticmethod
    def forward(ctx, fn, x, weights):
        ctx.save_for_backward(weights)
        ctx.x_meta = (x.dtype, x.dim())
        return fn(x, weights)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (w,) = ctx.saved_tensors
        dtype, dim = ctx.x_meta
        w = w.to(device=g.device, dtype=torch.float64).reshape((-1,) + (1,) * (dim - 1))
        return None, (w * g.unsqueeze(0)).to(dtype), None


class _HeatingGrad(torch.autograd.Function):
    """forward: heating_rate as without autograd; backward: the two-point stencil
    transposed, in torch ops."""

    @staticmethod
    def forward(ctx, bflux, dz, rho, cp):
        ctx.cp = cp
        ctx.save_for_backward(bflux, dz, rho)
        return heating_rate(bflux, dz, rho, cp)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        bflux, dz, rho = ctx.saved_tensors
        f = bflux.to(torch.float64)
        d, r = dz.to(g.device), rho.to(g.device)
        gf = gd = gr = None
        q = g / (r * ctx.cp * d)  # dT/dt = -q D with D = dF[k+1] - dF[k], dF = F_up - F_dn
        if ctx.needs_input_grad[0]:
            gdf = torch.zeros(f.shape[:2], dtype=torch.float64, device=g.device)
            gdf[:, 1:] -= q
            gdf[:, :-1] += q
            gf = torch.stack([gdf, -gdf], dim=-1).to(bflux.dtype)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            df = f[..., 0] - f[..., 1]
            qd = q * (df[:, 1:] - df[:, :-1])
            if ctx.needs_input_grad[1]:
                gd = (qd / d).to(dz.device)
            if ctx.needs_input_grad[2]:
                gr = (qd / r).to(rho.device)
        return gf, gd, gr, None


def band_flux(flux: torch.Tensor, weights: torch.Tensor,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sum_g w_g F_g for flux (G, ncol, nlev, 2) and weights (G,), in g order
    (hd_band_flux; examples/amars_lw.cpp:84-88, amars_sw.cpp:169-196 with
    w = d(wavenumber)).  Differentiable in flux."""
    if _wants_grad("band_flux", weights, (flux,), out):
        return _BandSumGrad.apply(band_flux, flux, torch.as_tensor(weights))
    f = _dev_f64(flux, "band_flux")
    G, ncol, nlev, two = f.shape
    if two != 2:
        raise RuntimeError("band_flux: flux must be (G, ncol, nlev, 2)")
    w = torch.as_tensor(weights, dtype=torch.float64).to(f.device).contiguous()
    if w.numel() != G:
        raise RuntimeError(f"band_flux: {w.numel()} weights for {G} g-points")
    if out is None:
        out = torch.empty((ncol, nlev, 2), dtype=torch.float64, device=f.device)
    with torch.cuda.device(f.device):
        _lib.check(_lib.load().hd_band_flux(f.data_ptr(), w.data_ptr(), G, ncol, nlev,
                                            out.data_ptr(), _stream(f.device)))
    return out


def band_flx(flx: torch.Tensor, weights: torch.Tensor,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sum_g w_g flx_g for the full flux record (G, ncol, nlev, NFLX) of
    Disort.forward_flx and weights (G,), in g order: (ncol, nlev, NFLX).  The same
    kernel as band_flux (hd_band_flux sums (level, component) pairs without looking
    at them: nlev * NFLX / 2 "levels" of two).  Differentiable in flx."""
    from .index import NFLX
    if _wants_grad("band_flx", weights, (flx,), out):
        return _BandSumGrad.apply(band_flx, flx, torch.as_tensor(weights))
    f = _dev_f64(flx, "band_flx")
    if f.dim() != 4 or f.shape[3] != NFLX:
        raise RuntimeError(f"band_flx: flx must be (G, ncol, nlev, {NFLX})")
    G, ncol, nlev, _ = f.shape
    w = torch.as_tensor(weights, dtype=torch.float64).to(f.device).contiguous()
    if w.numel() != G:
        raise RuntimeError(f"band_flx: {w.numel()} weights for {G} g-points")
    if out is None:
        out = torch.empty((ncol, nlev, NFLX), dtype=torch.float64, device=f.device)
    with torch.cuda.device(f.device):
        _lib.check(_lib.load().hd_band_flux(f.data_ptr(), w.data_ptr(), G, ncol,
                                            nlev * (NFLX // 2), out.data_ptr(),
                                            _stream(f.device)))
    return out


def band_rad(x: torch.Tensor, weights: torch.Tensor,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sum_w weights[w] x[w] for any per-wave field x (nwave, ...), e.g. the ray
    radiances (nwave, ncol, ntau, nray) of Disort.forward_rays: shape x.shape[1:]
    (hd_band_sum; the legacy driver's ``btoa(n) += wght[b] * toa(b, n)``,
    rt_solver_disort.cpp_:268-271).  One fma per wave in wave order: bitwise equal to
    the sum Disort.forward_rays_band fuses into the solve.  Differentiable in x."""
    if _wants_grad("band_rad", weights, (x,), out):
        return _BandSumGrad.apply(band_rad, x, torch.as_tensor(weights))
    f = _dev_f64(x, "band_rad")
    if f.dim() < 1:
        raise RuntimeError("band_rad: x must be (nwave, ...)")
    nwave = f.shape[0]
    w = torch.as_tensor(weights, dtype=torch.float64).to(f.device).reshape(-1).contiguous()
    if w.numel() != nwave:
        raise RuntimeError(f"band_rad: {w.numel()} weights for {nwave} waves")
    if out is None:
        out = torch.empty(tuple(f.shape[1:]), dtype=torch.float64, device=f.device)
    elif (out.device != f.device or out.dtype != torch.float64 or not out.is_contiguous()
          or out.shape != f.shape[1:]):
        raise RuntimeError(f"band_rad: out must be a contiguous float64 tensor of shape "
                           f"{tuple(f.shape[1:])} on {f.device}")
    with torch.cuda.device(f.device):
        _lib.check(_lib.load().hd_band_sum(f.data_ptr(), w.data_ptr(), nwave, out.numel(),
                                           out.data_ptr(), _stream(f.device)))
    return out


def heating_rate(bflux: torch.Tensor, dz: torch.Tensor, rho: torch.Tensor,
                 cp: float) -> torch.Tensor:
    """dT/dt (ncol, nlyr) [K/s] = -(1/(rho c_p)) d(F_up - F_dn)/dz from the band
    flux (ncol, nlyr+1, 2), level 0 = bottom (examples/amars_sw.cpp:291-302).
    Differentiable in bflux, dz and rho."""
    grad = _wants_grad("heating_rate", None, (bflux, dz, rho))
    f = _dev_f64(bflux, "heating_rate")
    ncol, nlev, _ = f.shape
    nlyr = nlev - 1
    d = torch.as_tensor(dz, dtype=torch.float64).to(f.device)
    r = torch.as_tensor(rho, dtype=torch.float64).to(f.device)
    d = d.reshape(-1)[:nlyr].expand(ncol, nlyr) if d.numel() == nlyr else d.reshape(ncol, nlyr)
    r = r.reshape(-1).expand(ncol, nlyr) if r.numel() == nlyr else r.reshape(ncol, nlyr)
    if grad:  # (dz and rho broadcast by the torch ops above: torch sums their gradient)
        return _HeatingGrad.apply(bflux, d, r, float(cp))
    d, r = d.contiguous(), r.contiguous()
    out = torch.empty((ncol, nlyr), dtype=torch.float64, device=f.device)
    with torch.cuda.device(f.device):
        _lib.check(_lib.load().hd_heating_rate(f.data_ptr(), d.data_ptr(), r.data_ptr(),
                                               float(cp), ncol, nlyr, out.data_ptr(),
                                               _stream(f.device)))
    return out


def spherical_flux_correction(bflux: torch.Tensor, x1f: torch.Tensor, area: torch.Tensor,
                              vol: torch.Tensor) -> torch.Tensor:
    """In place on the band flux (ncol, nlev, 2) along the level axis
    (src/utils/spherical_flux_correction.cpp:3-17; legacy
    rt_solver_disort.cpp_:186-207): top-level fluxes stay, lower levels are
    rescaled so the flux divergence per volume matches the plane-parallel one."""
    f = _dev_f64(bflux, "spherical_flux_correction")
    if f.data_ptr() != bflux.data_ptr():
        raise RuntimeError("spherical_flux_correction: bflux must be a contiguous f64 tensor")
    ncol, nlev, _ = f.shape
    dev = f.device
    x = torch.as_tensor(x1f, dtype=torch.float64).to(dev).contiguous()
    a = torch.as_tensor(area, dtype=torch.float64).to(dev).contiguous()
    v = torch.as_tensor(vol, dtype=torch.float64).to(dev).contiguous()
    if x.numel() != nlev or a.numel() != nlev or v.numel() < nlev - 1:
        raise RuntimeError("spherical_flux_correction: x1f/area need nlev entries, vol nlev-1")
    with torch.cuda.device(dev):
        _lib.check(_lib.load().hd_spherical_flux_correction(f.data_ptr(), x.data_ptr(),
                                                            a.data_ptr(), v.data_ptr(), ncol,
                                                            nlev, _stream(dev)))
    return bflux


def allreduce_band_flux(partial: torch.Tensor, group=None) -> torch.Tensor:
    """Complete the band sum across ranks (in place; returns the tensor)."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(partial, op=dist.ReduceOp.SUM, group=group)
    return partial
