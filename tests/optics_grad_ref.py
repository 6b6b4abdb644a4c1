"""The judge of the optics gradients (TEST INFRASTRUCTURE ONLY): a float64 torch
restatement of the four optics calls of include/hdharp.h (hd_attenuate, hd_band_optics,
hd_band_loop_optics, hd_rfm_attenuate), of the heating rate and of the band sum, built
from differentiable torch ops in the expression order of oracle/harp_np.py.  torch's
autograd through it defines the gradients the kernels are compared with.

Index pairs are computed without grad, as locate does it (harp_np.locate on the detached
values), then the two-point formula is applied: inside a cell autograd sees the slope
(v2 - v1)/(x2 - x1), where the pair collapses (clamped ends, the last knot) it sees the
constant (v1 + v2)/2, and on an inner knot the cell locate returns (the right one).
tests/test_optics_grad_ref.py pins this module on the CPU against harp_np and its
central differences.
"""

import numpy as np
import torch

from oracle import harp_np

F64 = torch.float64


def _t(x):
    return x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, np.float64))


def index_pair(axis, x):
    """(i1, i2) of interpn.h for every element of x (any shape), as LongTensors"""
    axis = np.asarray(axis, np.float64)
    xv = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, np.float64)
    n = len(axis)
    i1 = np.zeros(xv.shape, np.int64)
    i2 = np.zeros(xv.shape, np.int64)
    for idx in np.ndindex(xv.shape):
        j = harp_np.locate(axis, xv[idx])
        if j == -1:
            i1[idx] = i2[idx] = 0
        elif j == n - 1:
            i1[idx] = i2[idx] = n - 1
        else:
            i1[idx], i2[idx] = j, j + 1
    return torch.as_tensor(i1), torch.as_tensor(i2)


def lerp(axis, i1, i2, x, v1, v2):
    """interpn.h's two-point formula; (v1 + v2)/2 where the pair collapses"""
    axis = _t(axis)
    x1, x2 = axis[i1], axis[i2]
    same = x2 == x1
    den = torch.where(same, torch.ones_like(x1), x2 - x1)  # (no 0/0 in the branch not taken)
    return torch.where(same, (v1 + v2) / 2.0, ((x - x1) * v2 + (x2 - x) * v1) / den)


def coefficients(kwave, cols, coord):
    """(nwave, ncols): harp_np.interp1 of the table columns at every coordinate; the
    tables and the coordinate are not differentiated"""
    data = np.stack([np.asarray(c, np.float64) for c in cols], axis=1)
    return torch.as_tensor(np.stack([harp_np.interp1(x, np.asarray(kwave), data) for x in coord]))


def _wavelength(wavenumber, wavelength):
    return 1.0e4 / np.asarray(wavenumber) if wavelength is None else np.asarray(wavelength)


def attenuate(kwave, kdata, species, conc, wavenumber=None, wavelength=None):
    """harp_np.attenuate: (nwave, ncol, nlyr, 2) = (k c, ssa (k c))"""
    cf = coefficients(kwave, [kdata[:, 0], kdata[:, 1]], _wavelength(wavenumber, wavelength))
    kc = cf[:, 0, None, None] * _t(conc)[None, :, :, species]
    return torch.stack([kc, cf[:, 1, None, None] * kc], dim=-1)


def _dz(dz, ncol, nlyr):
    return _t(dz).reshape(-1, nlyr).expand(ncol, nlyr)


def band_optics(tables, conc, dz, nprop=2, wavenumber=None, wavelength=None):
    """harp_np.band_optics; tables: [(kwave, kdata, species)]"""
    conc = _t(conc)
    ncol, nlyr, _ = conc.shape
    tot = None
    for kwave, kdata, sp in tables:
        a = attenuate(kwave, kdata, sp, conc, wavenumber, wavelength)
        tot = a if tot is None else tot + a
    tot = tot * _dz(dz, ncol, nlyr)[None, :, :, None]
    has = tot[..., 0] != 0.0
    ssa = torch.where(has, tot[..., 1] / torch.where(has, tot[..., 0], torch.ones_like(tot[..., 0])),
                      torch.zeros_like(tot[..., 0]))
    rest = [torch.zeros_like(ssa)] * (nprop - 2)
    return torch.stack([tot[..., 0], ssa] + rest, dim=-1)


def band_loop_optics(tables, conc, dz, nmom, wavenumber=None, wavelength=None, ext0=None):
    """harp_np.band_loop_optics; tables: [(kwave, kdata, species, g or None)]"""
    conc = _t(conc)
    coord = _wavelength(wavenumber, wavelength)
    ncol, nlyr, _ = conc.shape
    nwave = len(coord)
    ext = torch.zeros((nwave, ncol, nlyr), dtype=F64)
    sca = torch.zeros((nwave, ncol, nlyr), dtype=F64)
    mom = [torch.zeros((nwave, ncol, nlyr), dtype=F64) for _ in range(nmom)]
    if ext0 is not None:
        ext = ext + _t(ext0).reshape(nwave, ncol, nlyr)
    for kwave, kdata, sp, g in tables:
        cf = coefficients(kwave, [kdata[:, 0], kdata[:, 1],
                                  np.zeros(len(kwave)) if g is None else g], coord)
        k, s, gw = (cf[:, i, None, None] for i in range(3))
        kc = k * conc[None, :, :, sp]
        ext = ext + kc
        sca = sca + s * kc
        if g is not None:
            chi = gw
            for l in range(nmom):
                if l:
                    chi = chi * gw
                mom[l] = mom[l] + (chi * s) * kc
    slots = [ext * _dz(dz, ncol, nlyr)[None], sca / (ext + 1e-10)]
    slots += [m / (sca + 1e-10) for m in mom]
    return torch.stack(slots, dim=-1)


def rfm_forward(wave, lnp_axis, temp_axis, ref_temp, kdata, conc, pres, temp, species):
    """harp_np.rfm_forward: (nwave, ncol, nlyr, 1)"""
    conc, pres, temp = _t(conc), _t(pres), _t(temp)
    kd = _t(kdata)
    ncol, nlyr = conc.shape[:2]
    pres, temp = pres.expand(ncol, nlyr), temp.expand(ncol, nlyr)
    lnp = torch.log(pres)
    p1, p2 = index_pair(lnp_axis, lnp)
    rt = _t(ref_temp)
    tempa = temp - lerp(lnp_axis, p1, p2, lnp, rt[p1], rt[p2])
    q1, q2 = index_pair(temp_axis, tempa)
    xw = _t(wave)
    w1, w2 = index_pair(wave, xw)

    def at_wave(iw):
        iw = iw[:, None, None]
        a = lerp(temp_axis, q1, q2, tempa, kd[iw, p1, q1], kd[iw, p1, q2])
        b = lerp(temp_axis, q1, q2, tempa, kd[iw, p2, q1], kd[iw, p2, q2])
        return lerp(lnp_axis, p1, p2, lnp, a, b)

    v = lerp(wave, w1[:, None, None], w2[:, None, None], xw[:, None, None], at_wave(w1),
             at_wave(w2))
    return (1.0e-3 * torch.exp(v) * conc[None, :, :, species])[..., None]


def band_sum(x, weight):
    """harp_np.band_flux for any per-wave field: sum_w weight_w x_w in w order"""
    x, weight = _t(x), _t(weight)
    out = torch.zeros(x.shape[1:], dtype=F64)
    for w in range(x.shape[0]):
        out = weight[w] * x[w] + out
    return out


def heating_rate(bflux, dz, rho, cp):
    """harp_np.heating_rate"""
    bflux = _t(bflux)
    df = bflux[..., 0] - bflux[..., 1]
    ncol, nlev = df.shape
    dz = _t(dz).expand(ncol, nlev - 1)
    rho = _t(rho).expand(ncol, nlev - 1)
    return -(1.0 / (rho * cp)) * (df[:, 1:] - df[:, :-1]) / dz
