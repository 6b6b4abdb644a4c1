"""numpy restatement of the Beer-Lambert solver (include/hdbeer.h, the formulas of
DESIGN.md section 3d): pure-absorption fluxes, emergent ray radiances and the alpha term.
Test infrastructure only; written from the formulas, not from the kernels.

Layer transfer at slant thickness x = dtau / |mu|, E = -expm1(-x), w1 = 1 - E / x:
    I_out = I_in (1 - E) + B_out w1 + B_in (E - w1)
with B_in on the side the ray enters.  Harp layout throughout: prop (W, C, L, nprop) with
layer 0 at the bottom, temf (C, L+1) bottom -> top, flux (W, C, L+1, 2) level 0 = surface.
"""

import math

import numpy as np
from scipy.special import gamma, gammaincc

from oracle.disort_np import double_gauss, plkavg


def coef(x):
    """(exp(-x), w1, E - w1) for x >= 0; x = 0 gives (1, 0, 0)."""
    x = np.asarray(x, np.float64)
    small = x < 0.5
    xs = np.where(small, x, 0.0)
    # w1 = sum_{k>=1} (-1)^(k+1) x^k / (k+1)!  (26 terms: 0.5^27 / 28! ~ 2e-38)
    p = np.zeros_like(xs)
    for k in range(26, 0, -1):
        p = 1.0 / math.factorial(k + 1) - xs * p
    w1s = xs * p
    es = xs - xs * w1s
    xl = np.where(small, 1.0, x)
    el = -np.expm1(-xl)
    w1l = 1.0 - el / xl
    e = np.where(small, es, el)
    w1 = np.where(small, w1s, w1l)
    t = np.where(small, 1.0 - es, np.exp(-xl))
    return t, w1, e - w1


def step(i_in, x, b_in, b_out):
    t, w1, cin = coef(x)
    return i_in * t + b_out * w1 + b_in * cin


def alpha_term(alpha, x):
    """alpha Gamma(alpha, x) x^-alpha = int_x^inf (t/x)^alpha e^-t dt - e^-x."""
    return alpha * gammaincc(alpha, x) * gamma(alpha) * x ** (-alpha)


def _bcs(bc, nwave, ncol):
    d = dict(fbeam=0.0, umu0=1.0, albedo=0.0, btemp=0.0, ttemp=0.0, temis=0.0, fisot=0.0)
    out = {}
    for k, v in d.items():
        x = bc.get(k) if bc else None
        out[k] = np.broadcast_to(np.asarray(v if x is None else x, np.float64), (nwave, ncol))
    return out


def _planck(v, temf, w, c, nlyr, planck, wave_lower, wave_upper):
    """(B at the L+1 levels bottom -> top, B(btemp), temis B(ttemp))"""
    if not planck:
        return np.zeros(nlyr + 1), 0.0, 0.0
    lo, hi = wave_lower[w], wave_upper[w]
    blev = np.array([plkavg(lo, hi, t) for t in np.asarray(temf)[c]])
    te = v["temis"][w, c]
    return blev, plkavg(lo, hi, v["btemp"][w, c]), \
        (te * plkavg(lo, hi, v["ttemp"][w, c]) if te != 0.0 else 0.0)


def _down(dtau, blev, top, mu):
    """downward intensities (L+1, n) at the levels, bottom -> top order, for cosines mu"""
    nlyr = dtau.size
    out = np.zeros((nlyr + 1, mu.size))
    out[nlyr] = top
    for l in range(nlyr - 1, -1, -1):
        out[l] = step(out[l + 1], dtau[l] / mu, blev[l + 1], blev[l])
    return out


def _up(dtau, blev, isurf, mu):
    nlyr = dtau.size
    out = np.zeros((nlyr + 1, mu.size))
    out[0] = isurf
    for l in range(nlyr):
        out[l + 1] = step(out[l], dtau[l] / mu, blev[l], blev[l + 1])
    return out


def _surface(v, w, c, dtau, blev, bsurf, btop, cmu, cwt):
    """(downward intensities at the levels, total downward flux per level, I_up at the surface)"""
    idn = _down(dtau, blev, v["fisot"][w, c] + btop, cmu)
    fdn = 2.0 * math.pi * idn @ (cwt * cmu)
    fb, mu0 = v["fbeam"][w, c], v["umu0"][w, c]
    if fb > 0.0:
        tauc = np.concatenate([np.cumsum(dtau[::-1])[::-1], [0.0]])  # depth from the top
        fdn = fdn + mu0 * fb * np.exp(-tauc / mu0)
    alb = v["albedo"][w, c]
    return fdn, (1.0 - alb) * bsurf + alb * fdn[0] / math.pi


def beer_flux(prop, bc, temf=None, *, nstr, planck=False, wave_lower=None, wave_upper=None):
    prop = np.asarray(prop, np.float64)
    nwave, ncol, nlyr, _ = prop.shape
    v = _bcs(bc, nwave, ncol)
    cmu, cwt = double_gauss(nstr // 2)
    flux = np.zeros((nwave, ncol, nlyr + 1, 2))
    for w in range(nwave):
        for c in range(ncol):
            dtau = prop[w, c, :, 0]
            blev, bsurf, btop = _planck(v, temf, w, c, nlyr, planck, wave_lower, wave_upper)
            fdn, isurf = _surface(v, w, c, dtau, blev, bsurf, btop, cmu, cwt)
            flux[w, c, :, 1] = fdn
            flux[w, c, :, 0] = 2.0 * math.pi * _up(dtau, blev, isurf, cmu) @ (cwt * cmu)
    return flux


def beer_rays(prop, bc, temf=None, *, nstr, umu, alpha=0.0, planck=False, wave_lower=None,
              wave_upper=None):
    """(W, C, nray): umu (nray,) or (C, nray), all cosines valid"""
    prop = np.asarray(prop, np.float64)
    nwave, ncol, nlyr, _ = prop.shape
    v = _bcs(bc, nwave, ncol)
    cmu, cwt = double_gauss(nstr // 2)
    umu = np.broadcast_to(np.asarray(umu, np.float64), (ncol, np.shape(umu)[-1]))
    rad = np.zeros((nwave, ncol, umu.shape[1]))
    for w in range(nwave):
        for c in range(ncol):
            dtau = prop[w, c, :, 0]
            blev, bsurf, btop = _planck(v, temf, w, c, nlyr, planck, wave_lower, wave_upper)
            _, isurf = _surface(v, w, c, dtau, blev, bsurf, btop, cmu, cwt)
            mu = umu[c]
            up, dn = mu > 0, mu < 0
            if up.any():
                r = _up(dtau, blev, isurf, mu[up])[nlyr]
                if alpha > 0.0:
                    xs = dtau.sum() / mu[up]
                    on = (xs > 0.0) & (xs < 1000.0)
                    term = np.zeros_like(xs)
                    term[on] = alpha_term(alpha, xs[on])
                    r = r + (1.0 - v["albedo"][w, c]) * bsurf * term
                rad[w, c, up] = r
            if dn.any():
                rad[w, c, dn] = _down(dtau, blev, v["fisot"][w, c] + btop, -mu[dn])[0]
    return rad
