"""float64 torch restatement of tests/beer_ref.py (the formulas of DESIGN.md section 3d),
with autograd doing the differentiation: the reference of the Beer-Lambert gradients.
Test infrastructure only; written from the formulas, not from the kernels.

Two pieces are not left to autograd, because their forward values come from numpy/scipy:
the Planck band value (oracle.disort_np.plkavg), whose temperature derivative is DEFINED
by Leibniz' rule on the exact band integral,
    dB/dT = (4 B - K T^4 (g(v2) - g(v1))) / T,  g(v) = v^4 e^-v / (1 - e^-v),  v = c2 nu / T,
and the alpha term A(x) = alpha Gamma(alpha, x) x^-alpha, with
    dA/dx = -alpha e^-x / x - (alpha / x) A(x).

Everything is batched over (nwave, ncol); the layer loops are those of beer_ref.
"""

import math

import numpy as np
import torch

import beer_ref
from oracle.disort_np import double_gauss, plkavg

F64 = torch.float64
SIGDPI = 5.67032e-8 / math.pi       # plkavg's constants
CONC = 15.0 / math.pi ** 4
C2 = 1.438786
BC_DEFAULTS = dict(fbeam=0.0, umu0=1.0, albedo=0.0, btemp=0.0, ttemp=0.0, temis=0.0, fisot=0.0)


def _t(x):
    return x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, np.float64))


def w1p_series(x):
    """dw1/dx below the solver's threshold x = 1/8: sum_{k>=1} (-1)^(k+1) k x^(k-1)/(k+1)!,
    eleven terms (the first one dropped is 12 x^11 / 13! < 2.3e-19 at x = 1/8); x = 0
    gives 1/2 exactly.  numpy float64, Horner."""
    x = np.asarray(x, np.float64)
    p = np.full_like(x, 11.0 / math.factorial(12))
    for k in range(10, 0, -1):
        p = k / math.factorial(k + 1) - x * p
    return p


def w1p(x):
    """dw1/dx = ((1 - w1) - t) / x, by the series where the solver uses it"""
    x = np.asarray(x, np.float64)
    big = np.where(x < 0.125, 1.0, x)
    t, w1, _ = beer_ref.coef(big)
    return np.where(x < 0.125, w1p_series(np.where(x < 0.125, x, 0.0)), ((1.0 - w1) - t) / big)


def coef(x):
    """beer_ref.coef on a tensor: (exp(-x), w1, E - w1)"""
    small = x < 0.5
    xs = torch.where(small, x, torch.zeros_like(x))
    p = torch.zeros_like(xs)
    for k in range(26, 0, -1):
        p = 1.0 / math.factorial(k + 1) - xs * p
    w1s = xs * p
    es = xs - xs * w1s
    xl = torch.where(small, torch.ones_like(x), x)
    el = -torch.expm1(-xl)
    w1l = 1.0 - el / xl
    e = torch.where(small, es, el)
    w1 = torch.where(small, w1s, w1l)
    t = torch.where(small, 1.0 - es, torch.exp(-xl))
    return t, w1, e - w1


def step(i_in, x, b_in, b_out):
    t, w1, cin = coef(x)
    return i_in * t + b_out * w1 + b_in * cin


def planck_dbdt(lo, hi, temp, b):
    """the Leibniz derivative of the band value b = plkavg(lo, hi, temp) (numpy, broadcast)"""
    temp = np.asarray(temp, np.float64)

    def g(v):
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            return np.where(v > 0.0, v ** 4 / np.expm1(np.where(v > 0.0, v, 1.0)), 0.0)

    safe = np.where(temp < 1.0e-4, 1.0, temp)
    d = (4.0 * b - SIGDPI * CONC * safe ** 4 * (g(C2 * hi / safe) - g(C2 * lo / safe))) / safe
    return np.where(temp < 1.0e-4, 0.0, d)


class _Planck(torch.autograd.Function):
    @staticmethod
    def forward(ctx, temp, lo, hi):
        tn = temp.detach().numpy()
        lo, hi = np.broadcast_to(lo, tn.shape), np.broadcast_to(hi, tn.shape)
        b = np.vectorize(plkavg, otypes=[np.float64])(lo, hi, tn)
        ctx.dbdt = torch.as_tensor(planck_dbdt(lo, hi, tn, b))
        return torch.as_tensor(b)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.dbdt, None, None


class _Alpha(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, alpha):
        a = torch.as_tensor(beer_ref.alpha_term(alpha, x.detach().numpy()))
        ctx.save_for_backward(x, a)
        ctx.alpha = alpha
        return a

    @staticmethod
    def backward(ctx, g):
        x, a = ctx.saved_tensors
        return g * (-ctx.alpha * torch.exp(-x) / x - ctx.alpha / x * a), None


def _bcs(bc, nwave, ncol):
    return {k: _t(v if (bc or {}).get(k) is None else bc[k]).to(F64).expand(nwave, ncol)
            for k, v in BC_DEFAULTS.items()}


def _planck(v, temf, nwave, ncol, nlyr, planck, wave_lower, wave_upper):
    """(B at the L+1 levels (W, C, L+1), B(btemp), temis B(ttemp))"""
    if not planck:
        z = torch.zeros(nwave, ncol, dtype=F64)
        return torch.zeros(nwave, ncol, nlyr + 1, dtype=F64), z, z
    lo = np.asarray(wave_lower, np.float64)[:, None]
    hi = np.asarray(wave_upper, np.float64)[:, None]
    blev = _Planck.apply(_t(temf).to(F64).expand(nwave, ncol, nlyr + 1), lo[..., None], hi[..., None])
    return blev, _Planck.apply(v["btemp"], lo, hi), v["temis"] * _Planck.apply(v["ttemp"], lo, hi)


def _down(tau, blev, top, mu):
    """downward intensities at the levels, a list bottom -> top of (W, C, n); mu (.., n)"""
    nlyr = tau.shape[-1]
    out = [None] * (nlyr + 1)
    out[nlyr] = top[..., None].expand(top.shape + mu.shape[-1:])
    for l in range(nlyr - 1, -1, -1):
        out[l] = step(out[l + 1], tau[..., l, None] / mu, blev[..., l + 1, None], blev[..., l, None])
    return out


def _up(tau, blev, isurf, mu):
    nlyr = tau.shape[-1]
    out = [isurf[..., None].expand(isurf.shape + mu.shape[-1:])]
    for l in range(nlyr):
        out.append(step(out[l], tau[..., l, None] / mu, blev[..., l, None], blev[..., l + 1, None]))
    return out


def _surface(v, tau, blev, bsurf, btop, cmu, cwt):
    """(total downward flux per level (W, C, L+1), I_up at the surface (W, C))"""
    idn = torch.stack(_down(tau, blev, v["fisot"] + btop, cmu), dim=2)
    fdn = 2.0 * math.pi * (idn * (cwt * cmu)).sum(-1)
    fb, mu0 = v["fbeam"], v["umu0"]
    on = fb > 0.0
    tauc = torch.cat([torch.flip(torch.cumsum(torch.flip(tau, [-1]), -1), [-1]),
                      torch.zeros_like(tau[..., :1])], -1)  # depth from the top
    m0 = torch.where(on, mu0, torch.ones_like(mu0))[..., None]
    fdn = fdn + torch.where(on[..., None], m0 * fb[..., None] * torch.exp(-tauc / m0),
                            torch.zeros_like(tauc))
    alb = v["albedo"]
    return fdn, (1.0 - alb) * bsurf + alb * fdn[..., 0] / math.pi


def _setup(prop, bc, temf, nstr, planck, wave_lower, wave_upper):
    prop = _t(prop).to(F64)
    nwave, ncol, nlyr, _ = prop.shape
    v = _bcs(bc, nwave, ncol)
    cmu, cwt = (torch.as_tensor(a) for a in double_gauss(nstr // 2))
    tau = prop[..., 0]
    blev, bsurf, btop = _planck(v, temf, nwave, ncol, nlyr, planck, wave_lower, wave_upper)
    return v, tau, blev, bsurf, btop, cmu, cwt


def beer_flux(prop, bc, temf=None, *, nstr, planck=False, wave_lower=None, wave_upper=None):
    """beer_ref.beer_flux on tensors: (W, C, L+1, 2), differentiable in prop[..., 0], temf
    and the bc entries"""
    v, tau, blev, bsurf, btop, cmu, cwt = _setup(prop, bc, temf, nstr, planck, wave_lower,
                                                 wave_upper)
    fdn, isurf = _surface(v, tau, blev, bsurf, btop, cmu, cwt)
    fup = 2.0 * math.pi * (torch.stack(_up(tau, blev, isurf, cmu), dim=2) * (cwt * cmu)).sum(-1)
    return torch.stack([fup, fdn], dim=-1)


def beer_rays(prop, bc, temf=None, *, nstr, umu, alpha=0.0, planck=False, wave_lower=None,
              wave_upper=None):
    """beer_ref.beer_rays on tensors: (W, C, nray); umu (nray,) or (C, nray), all valid"""
    v, tau, blev, bsurf, btop, cmu, cwt = _setup(prop, bc, temf, nstr, planck, wave_lower,
                                                 wave_upper)
    _, isurf = _surface(v, tau, blev, bsurf, btop, cmu, cwt)
    ncol = tau.shape[1]
    umu = _t(umu).to(F64)
    umu = umu.expand(ncol, umu.shape[-1])
    mu = umu.abs()
    rup = _up(tau, blev, isurf, mu)[-1]
    if alpha > 0.0:
        xs = tau.sum(-1, keepdim=True) / mu
        on = (xs > 0.0) & (xs < 1000.0)
        term = torch.where(on, _Alpha.apply(torch.where(on, xs, torch.ones_like(xs)), alpha),
                           torch.zeros_like(xs))
        rup = rup + ((1.0 - v["albedo"]) * bsurf)[..., None] * term
    rdn = _down(tau, blev, v["fisot"] + btop, mu)[0]
    return torch.where(umu > 0, rup, rdn)
