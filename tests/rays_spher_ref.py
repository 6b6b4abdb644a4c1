"""CPU reference of the pseudo-spherical ray radiances (hd_solve_rays_spher).

The model of DESIGN.md sections 3e and 3b, one column at a time: in every azimuthal mode
the beam of layer j is one exponential in tau' with the layer's secant lam_j and the
amplitude F0 exp(-ch'_top(j)) at the layer top; the factor 2 - delta_m0 and Y_l^m(mu0) at
the true mu0 are unchanged.  ``rays_spher_column`` is ``oracle.disort_rad_np``'s banded
system and source-function integration with that beam (the oracle's stages imported
read-only, the geometry from ``spher_ref``), with the Nakajima-Tanaka correction as the
library defines it: TMS on the same beam, IMS with the mean cosine of the slab above the
user depth, utau / ch(utau), in place of mu0.

``ode_rays_column`` is a check that does not use the eigen-solution: the 2N-stream
equation of mode m with the source x0_m(mu0) F0 e^{-ch'(tau)} is propagated through a fine
grid of sub-layers by the matrix exponential of the augmented system (as
``spher_ref.propagator_column``, here as a multiple-shooting system over all sub-levels),
and the ray radiance is the formal solution along the ray with Gauss-Legendre quadrature
inside each sub-layer.

Conventions as spher_ref: ``zd`` bottom -> top; the column functions take layers top ->
bottom (cdisort order), the batch driver harp's layout (layer 0 = bottom).
"""

import math

import numpy as np
import scipy.linalg

import spher_ref as S
from oracle.disort_np import DITHER, double_gauss, legendre_table, plkavg, setdis, soleig, upisot
from oracle.disort_rad_np import IMS_TINY, _seg_exp, _seg_lin, _user_taus, lepoly, xi_func


def _beam_at(chp, lam, taucpr, lc, tau):
    """e^{-ch'} at scaled depth tau of layer lc: from ch' of the layer's top level."""
    return math.exp(-chp[lc] - lam[lc] * (tau - taucpr[lc]))


def _solve_mode(m, nstr, nn, nlyr, cmu, cwt, cmu_full, cwt_full, dtaucp, taucpr, oprim, gl,
                beam, umu0, fbeam, chp, lam, albedo, fisot, planck, pkag, bplanck, tplanck):
    """disort_rad_np._solve_mode with the pseudo-spherical beam."""
    ylm = lepoly(nstr, m, cmu_full)
    ylm0 = lepoly(nstr, m, [-umu0])[:, 0] if beam else np.zeros(nstr)
    therm = planck and m == 0
    fac = (2.0 - (m == 0)) * fbeam / (4.0 * math.pi)
    kk = np.zeros((nlyr, nn))
    gc = np.zeros((nlyr, nstr, nstr))
    zb = np.zeros((nlyr, nstr))
    z0 = np.zeros((nlyr, nstr))
    z1 = np.zeros((nlyr, nstr))
    xr = np.zeros((nlyr, 2))
    for lc in range(nlyr):
        cc = 0.5 * (ylm.T * gl[lc]) @ ylm * cwt_full[None, :]
        k, gp, gm = soleig(cc, cmu)
        kk[lc] = k
        gc[lc, :nn, :nn] = gp
        gc[lc, nn:, :nn] = gm
        gc[lc, :nn, nn:] = gm
        gc[lc, nn:, nn:] = gp
        if beam:
            x0 = fac * (ylm.T @ (gl[lc] * ylm0))
            zb[lc] = np.linalg.solve(np.diag(1.0 + cmu_full * lam[lc]) - cc, x0)
        if therm:
            xr1 = (pkag[lc + 1] - pkag[lc]) / dtaucp[lc] if dtaucp[lc] > 0 else 0.0
            xr0 = pkag[lc] - xr1 * taucpr[lc]
            xr[lc] = (xr0, xr1)
            z0[lc], z1[lc] = upisot(cc, cmu_full, oprim[lc], xr0, xr1)

    def zpart(lc, tau):
        v = z0[lc] + z1[lc] * tau
        if beam:
            v = v + zb[lc] * _beam_at(chp, lam, taucpr, lc, tau)
        return v

    ee = np.exp(-kk * dtaucp[:, None])

    def top_cols(lc):
        return gc[lc] * np.concatenate([np.ones(nn), ee[lc]])[None, :]

    def bot_cols(lc):
        return gc[lc] * np.concatenate([ee[lc], np.ones(nn)])[None, :]

    ncol = nstr * nlyr
    a = np.zeros((ncol, ncol))
    b = np.zeros(ncol)
    a[:nn, :nstr] = top_cols(0)[nn:, :]
    b[:nn] = (fisot + tplanck if m == 0 else 0.0) - zpart(0, 0.0)[nn:]
    for lc in range(nlyr - 1):
        r0 = nn + lc * nstr
        a[r0:r0 + nstr, lc * nstr:(lc + 1) * nstr] = bot_cols(lc)
        a[r0:r0 + nstr, (lc + 1) * nstr:(lc + 2) * nstr] = -top_cols(lc + 1)
        tau = taucpr[lc + 1]
        b[r0:r0 + nstr] = zpart(lc + 1, tau) - zpart(lc, tau)
    r0 = nn + (nlyr - 1) * nstr
    lb = bot_cols(nlyr - 1)
    alb = albedo if m == 0 else 0.0
    refl = 2.0 * alb * (cwt * cmu)
    a[r0:r0 + nn, (nlyr - 1) * nstr:] = lb[:nn, :] - refl[None, :] @ lb[nn:, :]
    zbt = zpart(nlyr - 1, taucpr[nlyr])
    rhs = np.full(nn, (1.0 - alb) * bplanck if m == 0 else 0.0)
    if beam and m == 0:
        rhs += alb * umu0 * fbeam * math.exp(-chp[nlyr]) / math.pi
    b[r0:r0 + nn] = rhs - (zbt[:nn] - refl @ zbt[nn:])
    bw = 3 * nn - 1
    ab = np.zeros((2 * bw + 1, ncol))
    for j in range(ncol):
        lo = max(0, j - bw)
        hi = min(ncol, j + bw + 1)
        ab[bw + lo - j:bw + hi - j, j] = a[lo:hi, j]
    ll = scipy.linalg.solve_banded((bw, bw), ab, b).reshape(nlyr, nstr)

    def quad_field(lc, tau):
        """quadrature intensities (+mu_i then -mu_i) at scaled depth tau in layer lc"""
        e = np.concatenate([np.exp(-kk[lc] * (tau - taucpr[lc])),
                            np.exp(-kk[lc] * (taucpr[lc + 1] - tau))])
        return gc[lc] @ (ll[lc] * e) + zpart(lc, tau)

    return dict(kk=kk, gc=gc, zb=zb, z0=z0, z1=z1, xr=xr, ll=ll, quad_field=quad_field)


def _user_intensity(sol, m, nstr, nn, nlyr, umu, lay, utaupr, cmu, cwt, cmu_full, cwt_full,
                    taucpr, oprim, gl, beam, umu0, fbeam, chp, lam, albedo, fisot, planck,
                    bplanck, tplanck):
    """disort_rad_np._user_intensity with the beam source of layer lc on the layer's
    secant: amplitude e^{-ch'_top(lc)} at the layer top, rate lam[lc]."""
    kk, gc, zb, z0, z1, xr, ll = (sol[k] for k in ("kk", "gc", "zb", "z0", "z1", "xr", "ll"))
    ylm = lepoly(nstr, m, cmu_full)
    ylmu = lepoly(nstr, m, umu)
    ylm0 = lepoly(nstr, m, [-umu0])[:, 0] if beam else np.zeros(nstr)
    fac = (2.0 - (m == 0)) * fbeam / (4.0 * math.pi)
    therm = planck and m == 0
    ntau, numu = len(utaupr), umu.size
    res = np.zeros((ntau, numu))
    hmode = np.zeros((nlyr, numu, nstr))
    sbeam = np.zeros((nlyr, numu))
    sth0 = np.zeros((nlyr, numu))
    sth1 = np.zeros((nlyr, numu))
    for lc in range(nlyr):
        cu = 0.5 * (ylmu.T * gl[lc]) @ ylm * cwt_full[None, :]
        hmode[lc] = cu @ gc[lc]
        if beam:
            sbeam[lc] = (fac * (ylmu.T @ (gl[lc] * ylm0)) + cu @ zb[lc]) * math.exp(-chp[lc])
        if therm:
            sth0[lc] = (1.0 - oprim[lc]) * xr[lc, 0] + cu @ z0[lc]
            sth1[lc] = (1.0 - oprim[lc]) * xr[lc, 1] + cu @ z1[lc]
    tb = taucpr[nlyr]
    u_bot = sol["quad_field"](nlyr - 1, tb)
    fdn_bot = 2.0 * math.pi * u_bot[nn:] @ (cwt * cmu)
    if m == 0:
        dirb = umu0 * fbeam * math.exp(-chp[nlyr]) if beam else 0.0
        i_bot = albedo / math.pi * (fdn_bot + dirb) + (1.0 - albedo) * bplanck
        i_top = fisot + tplanck
    else:
        i_bot = i_top = 0.0

    def layer_integral(lc, iu, t1, t2, tau, mu):
        s = 0.0
        t0, tl = taucpr[lc], taucpr[lc + 1]
        for j in range(nn):
            s += _seg_exp(ll[lc, j] * hmode[lc, iu, j], kk[lc, j], t0, t1, t2, tau, mu)
            s += _seg_exp(ll[lc, nn + j] * hmode[lc, iu, nn + j], -kk[lc, j], tl, t1, t2, tau,
                          mu)
        if beam:
            s += _seg_exp(sbeam[lc, iu], lam[lc], t0, t1, t2, tau, mu)
        if therm:
            s += _seg_lin(sth0[lc, iu], sth1[lc, iu], t1, t2, tau, mu)
        return s

    for k in range(ntau):
        tau, lu = utaupr[k], lay[k]
        for iu, mu in enumerate(umu):
            if mu > 0.0:
                v = i_bot * math.exp(-(tb - tau) / mu)
                for lc in range(lu, nlyr):
                    v += layer_integral(lc, iu, max(tau, taucpr[lc]), taucpr[lc + 1], tau, mu)
            else:
                v = i_top * math.exp(tau / mu)
                for lc in range(lu, -1, -1):
                    v += layer_integral(lc, iu, min(tau, taucpr[lc + 1]), taucpr[lc], tau, mu)
            res[k, iu] = v
    return res


def _cos_theta(mu, ph, umu0, phi0):
    return -mu * umu0 + math.sqrt(max(0.0, 1 - mu * mu)) * \
        math.sqrt(max(0.0, 1 - umu0 * umu0)) * math.cos(math.radians(ph - phi0))


def _sinsca(phase, omega, taucpr, chp, lam, lay, tau, mu, fbeam):
    """disort_rad_np._sinsca on the pseudo-spherical beam."""
    nlyr = len(phase)
    s = 0.0
    if mu > 0.0:
        for lc in range(lay, nlyr):
            t1, t2 = max(tau, taucpr[lc]), taucpr[lc + 1]
            s += omega[lc] * phase[lc] * _seg_exp(math.exp(-chp[lc]), lam[lc], taucpr[lc], t1, t2,
                                                  tau, mu)
    else:
        for lc in range(lay, -1, -1):
            t1, t2 = min(tau, taucpr[lc + 1]), taucpr[lc]
            s += omega[lc] * phase[lc] * _seg_exp(math.exp(-chp[lc]), lam[lc], taucpr[lc], t1, t2,
                                                  tau, mu)
    return fbeam / (4.0 * math.pi) * s


def tms_rays(dtauc, ssalb, pmom, nstr, umu, phi, lay, utaupr, taucpr, chp, lam, umu0, phi0,
             fbeam):
    """The TMS step per paired ray, (ntau, nray): disort_rad_np.tms_correction with the
    layer's beam e^{-ch'_top(lc) - lam_lc (t - top_lc)} in place of e^{-t/mu0}; cos(Theta)
    keeps the true mu0."""
    ssalb = np.where(np.asarray(ssalb, np.float64) == 1.0, 1.0 - DITHER, ssalb)
    nlyr = len(dtauc)
    nmom = pmom.shape[1] - 1
    f = pmom[:, nstr] if nmom >= nstr else np.zeros(nlyr)
    oprim = ssalb * (1.0 - f) / (1.0 - ssalb * f)
    out = np.zeros((len(utaupr), len(umu)))
    for iu, (mu, ph) in enumerate(zip(umu, phi)):
        ct = _cos_theta(mu, ph, umu0, phi0)
        pl = legendre_table(nmom + 1, [ct])[:, 0]
        k = np.arange(nmom + 1)
        phasa = pmom @ ((2 * k + 1) * pl)
        chi = np.zeros((nlyr, nstr))
        chi[:, :min(nstr, nmom + 1)] = pmom[:, :min(nstr, nmom + 1)]
        kt = np.arange(nstr)
        plt = legendre_table(nstr, [ct])[:, 0]
        phasm = ((chi - f[:, None]) / (1.0 - f[:, None])) @ ((2 * kt + 1) * plt)
        phast = phasa / (1.0 - f * ssalb)
        for t, (lc, tau) in enumerate(zip(lay, utaupr)):
            out[t, iu] = _sinsca(phast, ssalb, taucpr, chp, lam, lc, tau, mu, fbeam) - \
                _sinsca(phasm, oprim, taucpr, chp, lam, lc, tau, mu, fbeam)
    return out


def mean_cosine(utau, lay, dtauc, ch, umu0):
    """mu0-bar = utau / ch(utau) per user depth: ch the unscaled slant depth (top -> bottom
    level values), linear in tau inside the user's layer.  In (0, 1] since every g >= 1;
    mu0 where the depth is 0 (the IMS step is off there)."""
    tauc = np.concatenate([[0.0], np.cumsum(dtauc)])
    out = np.full(len(utau), float(umu0))
    for t, (lc, u) in enumerate(zip(lay, utau)):
        frac = min(max((u - tauc[lc]) / dtauc[lc], 0.0), 1.0) if dtauc[lc] > 0.0 else 0.0
        chu = ch[lc] + (ch[lc + 1] - ch[lc]) * frac
        if chu > 0.0:
            out[t] = min(u / chu, 1.0)
    return out


def ims_rays(dtauc, ssalb, pmom, nstr, umu, phi, lay, utau, umu0, phi0, fbeam, mubar):
    """The IMS step per paired ray, (ntau, nray), to SUBTRACT: disort_rad_np.ims_correction
    with the beam cosine of the slab average replaced by ``mubar`` (per user depth);
    cos(Theta) keeps the true mu0."""
    ssalb = np.where(np.asarray(ssalb, np.float64) == 1.0, 1.0 - DITHER, ssalb)
    dtauc = np.asarray(dtauc, np.float64)
    nlyr = len(dtauc)
    nmom = pmom.shape[1] - 1
    out = np.zeros((len(utau), len(umu)))
    if nmom < nstr:
        return out
    f = pmom[:, nstr]
    tauc = np.concatenate([[0.0], np.cumsum(dtauc)])
    for t, (lc, u) in enumerate(zip(lay, utau)):
        dt = np.zeros(nlyr)
        dt[:lc] = dtauc[:lc]
        dt[lc] = max(0.0, u - tauc[lc])
        wt = ssalb * dt
        wsum, fsum, stau = wt.sum(), (wt * f).sum(), dt.sum()
        if wsum <= IMS_TINY or fsum <= IMS_TINY or stau <= IMS_TINY or fbeam <= IMS_TINY:
            continue
        gk = {k: (wt @ pmom[:, k]) / fsum for k in range(nstr, nmom + 1)}
        fw = fsum / stau
        mu0p = mubar[t] / (1.0 - fw)
        for iu, (mu, ph) in enumerate(zip(umu, phi)):
            if mu >= 0.0:
                continue
            xi = xi_func(-mu, mu0p, u)
            ct = _cos_theta(mu, ph, umu0, phi0)
            pl = legendre_table(nmom + 1, [ct])[:, 0]
            ps = 0.0
            for k in range(nmom + 1):
                wk = 1.0 if k < nstr else gk[k] * (2.0 - gk[k])
                ps += (2 * k + 1) * wk * pl[k]
            out[t, iu] = fbeam / (4.0 * math.pi) * fw * fw / (1.0 - fw) * ps * xi
    return out


def rays_spher_column(dtauc, ssalb, pmom, nstr, *, zd, radius, umu, phi, utau=None, umu0=1.0,
                      phi0=0.0, fbeam=0.0, albedo=0.0, fisot=0.0, planck=False, temper=None,
                      btemp=0.0, ttemp=0.0, temis=0.0, wvnmlo=0.0, wvnmhi=0.0, corint=False):
    """One pseudo-spherical solve with radiances along paired rays (umu[r], phi[r]), layers
    top -> bottom, zd bottom -> top.  utau None: the nlyr+1 layer boundaries (the direct
    flux then takes each level's own ch').  Returns rad (ntau, nray), uum (nmode, ntau,
    nray), flup / fdn at the depths, the per-mode solutions ``sol`` and the geometry."""
    dtauc = np.atleast_1d(np.asarray(dtauc, np.float64))
    ssalb = np.atleast_1d(np.asarray(ssalb, np.float64))
    nlyr = dtauc.size
    nn = nstr // 2
    pmom = np.asarray(pmom, np.float64).reshape(nlyr, -1)
    umu = np.atleast_1d(np.asarray(umu, np.float64))
    phi = np.atleast_1d(np.asarray(phi, np.float64))
    cmu, cwt = double_gauss(nn)
    cmu_full = np.concatenate([cmu, -cmu])
    cwt_full = np.concatenate([cwt, cwt])
    dtaucp, taucpr, tauc, oprim, gl = setdis(dtauc, ssalb, pmom, nstr)
    levels = utau is None
    utau = tauc.copy() if levels else np.atleast_1d(np.asarray(utau, np.float64))
    lay, utaupr = _user_taus(utau, dtauc, dtaucp, tauc, taucpr)
    if fbeam > 0.0 and not (0.0 < umu0 <= 1.0):
        raise ValueError(f"umu0 = {umu0} outside (0, 1] with fbeam > 0")
    beam = fbeam > 0.0
    if beam:
        chp, lam = S.layer_secants(zd, radius, umu0, dtaucp)
        ch = S.chapman(zd, radius, umu0, dtauc[::-1])[::-1]
    else:
        chp, lam, ch = np.zeros(nlyr + 1), np.zeros(nlyr), np.zeros(nlyr + 1)
    if planck:
        pkag = np.array([plkavg(wvnmlo, wvnmhi, t) for t in temper])
        bplanck = plkavg(wvnmlo, wvnmhi, btemp)
        tplanck = plkavg(wvnmlo, wvnmhi, ttemp) * temis
    else:
        pkag = np.zeros(nlyr + 1)
        bplanck = tplanck = 0.0
    nmode = nstr if beam else 1
    ntau, nray = utau.size, umu.size
    uum = np.zeros((nmode, ntau, nray))
    sols = []
    out = {}
    for m in range(nmode):
        sol = _solve_mode(m, nstr, nn, nlyr, cmu, cwt, cmu_full, cwt_full, dtaucp, taucpr, oprim,
                          gl, beam, umu0, fbeam, chp, lam, albedo, fisot, planck, pkag, bplanck,
                          tplanck)
        sols.append(sol)
        if m == 0:
            wmu = cwt * cmu
            flup, fdn = np.zeros(ntau), np.zeros(ntau)
            for k in range(ntau):
                u = sol["quad_field"](lay[k], utaupr[k])
                flup[k] = 2.0 * math.pi * u[:nn] @ wmu
                fdn[k] = 2.0 * math.pi * u[nn:] @ wmu
                if beam:
                    fdn[k] += umu0 * fbeam * (math.exp(-chp[k]) if levels else
                                              _beam_at(chp, lam, taucpr, lay[k], utaupr[k]))
            out.update(flup=flup, fdn=fdn)
        uum[m] = _user_intensity(sol, m, nstr, nn, nlyr, umu, lay, utaupr, cmu, cwt, cmu_full,
                                 cwt_full, taucpr, oprim, gl, beam, umu0, fbeam, chp, lam,
                                 albedo, fisot, planck, bplanck, tplanck)
    cosm = np.cos(np.arange(nmode)[:, None] * np.radians(phi - phi0)[None, :])  # (nmode, nray)
    rad = np.einsum("mr,mtr->tr", cosm, uum)
    if corint and beam:
        mubar = mean_cosine(utau, lay, dtauc, ch, umu0)
        rad = rad + tms_rays(dtauc, ssalb, pmom, nstr, umu, phi, lay, utaupr, taucpr, chp, lam,
                             umu0, phi0, fbeam) \
            - ims_rays(dtauc, ssalb, pmom, nstr, umu, phi, lay, utau, umu0, phi0, fbeam, mubar)
        out["mubar"] = mubar
    out.update(rad=rad, uum=uum, sol=sols, chp=chp, lam=lam, ch=ch, taucpr=taucpr, lay=lay,
               utaupr=utaupr, utau=utau)
    return out


def rays_spher_forward(prop, bc, temf=None, *, zd, radius, nstr, umu, phi, utau=None, nmom=None,
                       planck=False, wave_lower=None, wave_upper=None, corint=False,
                       beam_off=()):
    """Batch driver in harp's layout: prop (W, C, L, nprop), layer 0 = bottom; zd (L+1,) or
    (C, L+1); umu / phi (nray,) or (C, nray).  Columns in ``beam_off`` are solved without
    the beam (what the library does for a column with a bad zd).  Returns (rad (W, C, ntau,
    nray), depths in the user's order, flux (W, C, ntau, 2), index 0 = the deepest depth)."""
    prop = np.asarray(prop, np.float64)
    nwave, ncol, nlyr, nprop = prop.shape
    nmom = nstr if nmom is None else nmom
    nm = max(0, min(nmom, nprop - 2))
    zd = np.asarray(zd, np.float64)
    umu = np.asarray(umu, np.float64)
    phi = np.asarray(phi, np.float64)

    def bcv(key, default):
        if key in bc and bc[key] is not None:
            return np.broadcast_to(np.asarray(bc[key], np.float64), (nwave, ncol))
        return np.full((nwave, ncol), default)

    keys = dict(fbeam=0.0, umu0=1.0, phi0=0.0, albedo=0.0, btemp=0.0, ttemp=0.0, temis=0.0,
                fisot=0.0)
    v = {k: bcv(k, d) for k, d in keys.items()}
    rad = flux = None
    for w in range(nwave):
        for c in range(ncol):
            p = prop[w, c, ::-1]
            pm = np.zeros((nlyr, nm + 1))
            pm[:, 0] = 1.0
            if nm:
                pm[:, 1:] = p[:, 2:2 + nm]
            ssa = p[:, 1] if nprop > 1 else np.zeros(nlyr)
            kw = {}
            if planck:
                kw = dict(planck=True, temper=np.asarray(temf)[c, ::-1], btemp=v["btemp"][w, c],
                          ttemp=v["ttemp"][w, c], temis=v["temis"][w, c],
                          wvnmlo=wave_lower[w], wvnmhi=wave_upper[w])
            r = rays_spher_column(p[:, 0], ssa, pm, nstr, zd=zd[c] if zd.ndim == 2 else zd,
                                  radius=radius, umu=umu[c] if umu.ndim == 2 else umu,
                                  phi=phi[c] if phi.ndim == 2 else phi, utau=utau,
                                  umu0=v["umu0"][w, c], phi0=v["phi0"][w, c],
                                  fbeam=0.0 if c in beam_off else v["fbeam"][w, c],
                                  albedo=v["albedo"][w, c], fisot=v["fisot"][w, c],
                                  corint=corint, **kw)
            if rad is None:
                ntau = r["rad"].shape[0]
                rad = np.zeros((nwave, ncol, ntau, r["rad"].shape[1]))
                flux = np.zeros((nwave, ncol, ntau, 2))
            rad[w, c] = r["rad"]
            flux[w, c, :, 0] = r["flup"][::-1]
            flux[w, c, :, 1] = r["fdn"][::-1]
    return rad, flux


# --------------------------------------------------------------------------- #
# the check without the eigen-solution
# --------------------------------------------------------------------------- #
def ode_rays_column(dtauc, ssalb, pmom, nstr, *, zd, radius, umu, phi, umu0, phi0=0.0, fbeam,
                    albedo=0.0, nsub=4, order=24):
    """The beam-only problem of ``rays_spher_column`` (no correction) without eigenpairs.

    Per mode m the 2N-stream equation
        mu_i dI_i/dtau = I_i - sum_j CC^m_ij I_j - x0^m_i(mu0) s,   s = e^{-ch'(tau)},
    with ch' piecewise linear in tau' (slope lam per layer, ch' of the level at each layer
    top), is propagated across every sub-layer (``nsub`` equal parts per layer) by the
    matrix exponential of the system augmented with s; the sub-level intensities are the
    solution of the multiple-shooting system of those relations and the two boundary
    conditions (one linear solve, no growing exponentials carried through the column).
    The ray radiance at a sub-level is the formal solution along the ray,
        I(tau, mu) = I_b e^{-|tau_b - tau|/|mu|} + int S(t, mu) e^{-(t - tau)/mu} dt/mu,
        S = sum_j CU_j(mu) I_j(t) + xu(mu) s(t),
    by Gauss-Legendre quadrature of ``order`` nodes inside each sub-layer, the integrand
    taken from the propagator at the nodes.  Returns rad (nlyr * nsub + 1, nray) at every
    sub-level, top -> bottom, and the scaled depth of the sub-levels.
    """
    dtauc = np.atleast_1d(np.asarray(dtauc, np.float64))
    nlyr = dtauc.size
    nn = nstr // 2
    pmom = np.asarray(pmom, np.float64).reshape(nlyr, -1)
    umu = np.atleast_1d(np.asarray(umu, np.float64))
    phi = np.atleast_1d(np.asarray(phi, np.float64))
    cmu, cwt = double_gauss(nn)
    cmu_full = np.concatenate([cmu, -cmu])
    cwt_full = np.concatenate([cwt, cwt])
    dtaucp, taucpr, _, _, gl = setdis(dtauc, ssalb, pmom, nstr)
    chp, lam = S.layer_secants(zd, radius, umu0, dtaucp)
    nlev = nlyr * nsub + 1
    tsub = np.concatenate([taucpr[lc] + dtaucp[lc] * np.arange(nsub) / nsub
                           for lc in range(nlyr)] + [taucpr[nlyr:]])
    # s at the top of sub-layer n, from ch' of its layer's top level
    s_top = np.array([_beam_at(chp, lam, taucpr, n // nsub, tsub[n]) for n in range(nlev - 1)])
    s_bot = math.exp(-chp[nlyr])
    xg, wg = np.polynomial.legendre.leggauss(order)
    xg, wg = 0.5 * (xg + 1.0), 0.5 * wg  # on (0, 1)
    nray = umu.size
    rad = np.zeros((nlev, nray))
    wmu = cwt * cmu
    for m in range(nstr):
        ylm = lepoly(nstr, m, cmu_full)
        ylm0 = lepoly(nstr, m, [-umu0])[:, 0]
        ylmu = lepoly(nstr, m, umu)
        fac = (2.0 - (m == 0)) * fbeam / (4.0 * math.pi)
        alb = albedo if m == 0 else 0.0
        full, nodes, cus, xus = [], [], [], []
        for lc in range(nlyr):
            cc = 0.5 * (ylm.T * gl[lc]) @ ylm * cwt_full[None, :]
            x0 = fac * (ylm.T @ (gl[lc] * ylm0))
            mm = np.zeros((nstr + 1, nstr + 1))
            mm[:nstr, :nstr] = (np.eye(nstr) - cc) / cmu_full[:, None]
            mm[:nstr, nstr] = -x0 / cmu_full
            mm[nstr, nstr] = -lam[lc]
            h = dtaucp[lc] / nsub
            full.append(scipy.linalg.expm(mm * h))
            nodes.append([scipy.linalg.expm(mm * (h * x)) for x in xg])
            cus.append(0.5 * (ylmu.T * gl[lc]) @ ylm * cwt_full[None, :])  # (nray, nstr)
            xus.append(fac * (ylmu.T @ (gl[lc] * ylm0)))                    # (nray,)
        # multiple shooting: unknowns Y_n (nstr) at every sub-level
        nun = nlev * nstr
        a = np.zeros((nun, nun))
        b = np.zeros(nun)
        a[:nn, nn:nstr] = np.eye(nn)  # no diffuse light from above
        for n in range(nlev - 1):
            e = full[n // nsub]
            r0 = nn + n * nstr
            a[r0:r0 + nstr, n * nstr:(n + 1) * nstr] = e[:nstr, :nstr]
            a[r0:r0 + nstr, (n + 1) * nstr:(n + 2) * nstr] = -np.eye(nstr)
            b[r0:r0 + nstr] = -e[:nstr, nstr] * s_top[n]
        r0 = nn + (nlev - 1) * nstr
        refl = 2.0 * alb * wmu
        a[r0:r0 + nn, (nlev - 1) * nstr:(nlev - 1) * nstr + nn] = np.eye(nn)
        a[r0:r0 + nn, (nlev - 1) * nstr + nn:] = -np.outer(np.ones(nn), refl)
        b[r0:r0 + nn] = alb * umu0 * fbeam * s_bot / math.pi
        y = np.linalg.solve(a, b).reshape(nlev, nstr)
        # whole-sub-layer source integrals and transmissions per ray
        fdn_bot = 2.0 * math.pi * y[-1, nn:] @ wmu
        i_bot = alb / math.pi * (fdn_bot + umu0 * fbeam * s_bot)
        im = np.zeros((nlev, nray))
        for r, mu in enumerate(umu):
            amu = abs(mu)
            seg = np.zeros(nlev - 1)    # source of sub-layer n seen from its near end
            trn = np.zeros(nlev - 1)
            for n in range(nlev - 1):
                lc = n // nsub
                h = dtaucp[lc] / nsub
                ya = np.concatenate([y[n], [s_top[n]]])
                acc = 0.0
                for q in range(order):
                    yq = nodes[lc][q] @ ya
                    src = cus[lc][r] @ yq[:nstr] + xus[lc][r] * yq[nstr]
                    # distance from the node to the end the ray leaves through: the top
                    # for an upward ray, the bottom for a downward one
                    dist = h * xg[q] if mu > 0.0 else h * (1.0 - xg[q])
                    acc += wg[q] * src * math.exp(-dist / amu)
                seg[n] = acc * h / amu
                trn[n] = math.exp(-h / amu)
            if mu > 0.0:
                cur = i_bot
                im[nlev - 1, r] = cur
                for n in range(nlev - 2, -1, -1):
                    cur = cur * trn[n] + seg[n]
                    im[n, r] = cur
            else:
                cur = 0.0
                for n in range(nlev - 1):
                    cur = cur * trn[n] + seg[n]
                    im[n + 1, r] = cur
        rad += im * np.cos(m * np.radians(phi - phi0))[None, :]
    return rad, tsub
