"""Arbitrary-precision (mpmath) restatement of the flux-only DISORT solve.

TEST INFRASTRUCTURE ONLY.  Nothing in ``pyharp_amd`` imports this module; it is the
third pin of the flux solve, for the inputs on which the two
double-precision oracles (``disort_np``, ``disort_oracle.c``) themselves lose the
project's 1e-6: 1 - ssa below 1e-6, a temperature step across a layer thinner than
1e-5, a beam cosine within 1e-6 of 1/k of a layer.

Same stages and conventions as ``disort_np.disort_column`` (dither constant, delta-M,
Lambert surface, fisot, temis/ttemp, btemp, any nmom), carried out at ``dps`` decimal
digits:

* the inputs are doubles and are converted exactly; the dithered albedo is the double
  ``1.0 - DITHER`` that every double solver here uses;
* the Gauss nodes are refined by Newton's iteration to the working precision;
* the Planck level values are taken as given numbers: ``disort_np.plkavg`` in double
  (there is no mp PLKAVG; the truncation of that series is part of the contract);
* the eigenproblem is DISORT's reduced one, (alpha - beta)(alpha + beta), by the QR
  iteration of ``mpmath.eig``; the boundary system is solved dense by LU.

With ``zd`` and ``radius`` the beam is the pseudo-spherical one of DESIGN.md section 3e
(``tests/spher_ref.py`` is its double restatement): slant depths through spherical shells
and one secant per layer, formed at ``dps`` digits from the altitudes' doubles.  Without
them no expression changes.

The record (``rfldir, rfldn, flup, dfdt, uavg, uavgdn, uavgup, uavgso``) follows the
definitions of ``tests/flx_ref.py`` / ``include/hdisort.h``.
"""

from __future__ import annotations

import numpy as np
from mpmath import mp, mpf

from .disort_np import DITHER, plkavg

NFLX = 8
IRFLDIR, IRFLDN, IFLUP, IDFDT, IUAVG, IUAVGDN, IUAVGUP, IUAVGSO = range(NFLX)

_GAUSS = {}


def double_gauss(nn: int):
    """nn-point Gauss-Legendre nodes/weights on (0, 1) at the current precision."""
    key = (nn, mp.prec)
    if key in _GAUSS:
        return _GAUSS[key]
    x0, _ = np.polynomial.legendre.leggauss(nn)
    xs, ws = [], []
    for xi in x0:
        x = mpf(float(xi))
        for _ in range(12):  # quadratic from 1e-15: 4 steps reach 200 digits
            p0, p1 = mpf(1), x
            for l in range(2, nn + 1):
                p0, p1 = p1, ((2 * l - 1) * x * p1 - (l - 1) * p0) / l
            dp = nn * (x * p1 - p0) / (x * x - 1)
            dx = p1 / dp
            x -= dx
            if abs(dx) < mpf(10) ** (-mp.dps + 2):
                break
        p0, p1 = mpf(1), x
        for l in range(2, nn + 1):
            p0, p1 = p1, ((2 * l - 1) * x * p1 - (l - 1) * p0) / l
        dp = nn * (x * p1 - p0) / (x * x - 1)
        xs.append((x + 1) / 2)
        ws.append(1 / ((1 - x * x) * dp * dp))  # = (2 / ((1-x^2) P'^2)) / 2
    _GAUSS[key] = (xs, ws)
    return xs, ws


def _legendre(lmax, mus):
    """P_l(mu), l < lmax: list over l of lists over mu."""
    p = [[mpf(1)] * len(mus)]
    if lmax > 1:
        p.append(list(mus))
    for l in range(2, lmax):
        p.append([((2 * l - 1) * m * a - (l - 1) * b) / l
                  for m, a, b in zip(mus, p[l - 1], p[l - 2])])
    return p


def _solve(a, b):
    return list(mp.lu_solve(mp.matrix(a), mp.matrix(b)))


def _layer(gl, cmu, cwt, nn, nstr, ylm):
    """cc (nstr x nstr) and the eigen-solution kk, gplus, gminus of one layer."""
    cwt_full = cwt + cwt
    cc = [[sum(gl[l] * ylm[l][i] * ylm[l][j] for l in range(nstr)) * cwt_full[j] / 2
           for j in range(nstr)] for i in range(nstr)]
    apb = mp.matrix(nn, nn)
    amb = mp.matrix(nn, nn)
    for i in range(nn):
        for j in range(nn):
            al = (cc[i][j] - (1 if i == j else 0)) / cmu[i]
            be = cc[i][nn + j] / cmu[i]
            apb[i, j] = al + be
            amb[i, j] = al - be
    if nn == 1:
        evals, evecs = [amb[0, 0] * apb[0, 0]], mp.matrix([[1]])
    else:
        evals, evecs = mp.eig(amb * apb)
    tiny = mpf(10) ** (-mp.dps // 2)
    kk = []
    for e in evals:
        if abs(mp.im(e)) > tiny * max(1, abs(mp.re(e))) or mp.re(e) <= 0:
            raise ArithmeticError("disort_mp: eigenvalue not real and positive")
        kk.append(mp.sqrt(mp.re(e)))
    gp = [[None] * nn for _ in range(nn)]
    gm = [[None] * nn for _ in range(nn)]
    for j in range(nn):
        # a complex phase from the QR iteration: make the column real
        piv = max(range(nn), key=lambda i: abs(evecs[i, j]))
        ph = evecs[piv, j]
        x = [mp.re(evecs[i, j] / ph) for i in range(nn)]
        y = [sum(apb[i, m] * x[m] for m in range(nn)) / kk[j] for i in range(nn)]
        for i in range(nn):
            gp[i][j] = (x[i] + y[i]) / 2
            gm[i][j] = (x[i] - y[i]) / 2
    return cc, kk, gp, gm


def disort_column(dtauc, ssalb, pmom, nstr, *, umu0=1.0, fbeam=0.0, albedo=0.0, fisot=0.0,
                  planck=False, temper=None, btemp=0.0, ttemp=0.0, temis=0.0, wvnmlo=0.0,
                  wvnmhi=0.0, dps=50, return_mp=False, zd=None, radius=None, geom=None):
    """One flux-only DISORT solve at ``dps`` digits, cdisort conventions (top -> bottom).

    With ``zd`` (the nlyr+1 level altitudes, bottom -> top as everywhere in the library)
    and ``radius`` the beam is pseudo-spherical (the model of
    tests/spher_ref.py): it is attenuated along its true path through the shells, ch' on
    the delta-M scaled depths and ch on the unscaled ones, and inside layer lc it is one
    exponential of secant lam_lc = (ch'_{lc+1} - ch'_lc) / dtau'_lc (g(j, j) where dtau'
    = 0); the phase function keeps the true umu0.  ``geom`` = (chp, lam, ch), doubles in
    solver order (level / layer 0 = top), is a second beam path solved beside the column's
    own: its record comes back as ``flx_geom`` (the fixture generator's conditioning check:
    the slant quantities as evaluated in double against the same at ``dps`` digits).

    Returns a dict of float64 arrays over the nlyr+1 levels: the eight record entries by
    name, ``fdn`` = rfldir + rfldn, ``flx`` (nlyr+1, 8), ``scale`` (the magnitude dfdt is
    a difference of, as tests/flx_ref.py).  With ``return_mp`` also ``mp``: the record
    as mpf lists (for comparisons below double precision), ``kk``: the layers'
    eigenvalues, and ``lam``: the layers' beam secants (1 / umu0 without ``zd``).
    """
    with mp.workdps(dps):
        return _column(dtauc, ssalb, pmom, nstr, umu0, fbeam, albedo, fisot, planck, temper,
                       btemp, ttemp, temis, wvnmlo, wvnmhi, return_mp, zd, radius, geom)


def _column(dtauc, ssalb, pmom, nstr, umu0, fbeam, albedo, fisot, planck, temper, btemp,
            ttemp, temis, wvnmlo, wvnmhi, return_mp, zd=None, radius=None, geom=None):
    dtauc_d = np.atleast_1d(np.asarray(dtauc, np.float64))
    ssalb_d = np.atleast_1d(np.asarray(ssalb, np.float64))
    nlyr = dtauc_d.size
    if nstr < 2 or nstr % 2:
        raise ValueError("nstr must be even and >= 2")
    nn = nstr // 2
    pmom_d = np.asarray(pmom, np.float64).reshape(nlyr, -1)
    nmom = pmom_d.shape[1] - 1
    beam = float(fbeam) > 0.0
    if beam and not (0.0 < float(umu0) <= 1.0):
        raise ValueError(f"umu0 = {umu0} outside (0, 1] with fbeam > 0")
    umu0, fbeam, albedo, fisot = (mpf(float(v)) for v in (umu0, fbeam, albedo, fisot))
    pi = mp.pi

    cmu, cwt = double_gauss(nn)
    cmu_full = cmu + [-m for m in cmu]
    ylm = _legendre(nstr, cmu_full)

    # ---- setdis ----
    dt = [mpf(float(v)) for v in dtauc_d]
    ss = [mpf(1.0 - DITHER) if float(v) == 1.0 else mpf(float(v)) for v in ssalb_d]
    dtaucp, oprim, gls = [], [], []
    for lc in range(nlyr):
        pm = [mpf(float(v)) for v in pmom_d[lc]]
        f = pm[nstr] if nmom >= nstr else mpf(0)
        dtaucp.append((1 - ss[lc] * f) * dt[lc])
        op = ss[lc] * (1 - f) / (1 - ss[lc] * f)
        oprim.append(op)
        gls.append([(2 * k + 1) * op * ((pm[k] if k <= nmom else mpf(0)) - f) / (1 - f)
                    for k in range(nstr)])
    taucpr, tauc = [mpf(0)], [mpf(0)]
    for lc in range(nlyr):
        taucpr.append(taucpr[-1] + dtaucp[lc])
        tauc.append(tauc[-1] + dt[lc])

    if planck:
        pkag = [mpf(plkavg(wvnmlo, wvnmhi, float(t))) for t in temper]
        bplanck = mpf(plkavg(wvnmlo, wvnmhi, float(btemp)))
        tplanck = mpf(plkavg(wvnmlo, wvnmhi, float(ttemp))) * mpf(float(temis))
    else:
        pkag = [mpf(0)] * (nlyr + 1)
        bplanck = tplanck = mpf(0)

    # ---- the beam's slant depths at the levels and its secant in every layer ----
    if (zd is None) != (radius is None):
        raise ValueError("zd and radius go together")
    spher = zd is not None
    if geom is not None and not spher:
        raise ValueError("geom needs zd and radius")
    if not spher:  # plane-parallel: the expressions below keep umu0 itself
        own = ([t / umu0 for t in taucpr], [1 / umu0] * nlyr, [t / umu0 for t in tauc])
    else:
        own = _slant(zd, radius, umu0, dtaucp, dt)

    # ---- what does not depend on the beam's path: the layers' eigen-solutions, the
    #      thermal particular solutions and the boundary-condition matrix ----
    zero = [mpf(0)] * nstr
    kks, gcs, ccs, x0s, z0s, z1s = [], [], [], [], [], []
    p0 = [row[0] for row in _legendre(nstr, [-umu0])]
    for lc in range(nlyr):
        gl = gls[lc]
        cc, kk, gp, gm = _layer(gl, cmu, cwt, nn, nstr, ylm)
        kks.append(kk)
        ccs.append(cc)
        gc = [[None] * nstr for _ in range(nstr)]
        for i in range(nn):
            for j in range(nn):
                gc[i][j] = gp[i][j]
                gc[nn + i][j] = gm[i][j]
                gc[i][nn + j] = gm[i][j]
                gc[nn + i][nn + j] = gp[i][j]
        gcs.append(gc)
        x0s.append([fbeam / (4 * pi) * sum(ylm[l][i] * gl[l] * p0[l] for l in range(nstr))
                    for i in range(nstr)] if beam else zero)
        if planck:
            xr1 = (pkag[lc + 1] - pkag[lc]) / dtaucp[lc] if dtaucp[lc] > 0 else mpf(0)
            xr0 = pkag[lc] - xr1 * taucpr[lc]
            a = mp.matrix([[(1 if i == j else 0) - cc[i][j] for j in range(nstr)]
                           for i in range(nstr)])
            z1 = list(mp.lu_solve(a, mp.matrix([(1 - oprim[lc]) * xr1] * nstr)))
            z0 = list(mp.lu_solve(a, mp.matrix([(1 - oprim[lc]) * xr0 + cmu_full[i] * z1[i]
                                                for i in range(nstr)])))
            z0s.append(z0)
            z1s.append(z1)
        else:
            z0s.append(zero)
            z1s.append(zero)

    ee = [[mp.exp(-k * dtaucp[lc]) for k in kks[lc]] for lc in range(nlyr)]
    one = [mpf(1)] * nn

    def cols(lc, scal):
        return [[gcs[lc][i][j] * scal[j] for j in range(nstr)] for i in range(nstr)]

    tops = [cols(lc, one + ee[lc]) for lc in range(nlyr)]
    bots = [cols(lc, ee[lc] + one) for lc in range(nlyr)]
    ncol = nstr * nlyr
    a = mp.matrix(ncol, ncol)
    for i in range(nn):
        for j in range(nstr):
            a[i, j] = tops[0][nn + i][j]
    for lc in range(nlyr - 1):
        r0 = nn + lc * nstr
        for i in range(nstr):
            for j in range(nstr):
                a[r0 + i, lc * nstr + j] = bots[lc][i][j]
                a[r0 + i, (lc + 1) * nstr + j] = -tops[lc + 1][i][j]
    r0 = nn + (nlyr - 1) * nstr
    lb = bots[nlyr - 1]
    refl = [2 * albedo * cwt[i] * cmu[i] for i in range(nn)]
    for j in range(nstr):
        rl = sum(refl[m] * lb[nn + m][j] for m in range(nn))
        for i in range(nn):
            a[r0 + i, (nlyr - 1) * nstr + j] = lb[i][j] - rl

    # ---- per beam path: its particular solution, the right-hand side, the record ----
    def rhs_of(chp, lam):
        zbeam = []
        for lc in range(nlyr):
            # no scattering, no beam source: Z = 0 (and the matrix is singular where umu0
            # is a quadrature node exactly, 0.5 at nstr 2)
            if not beam or not any(v != 0 for v in x0s[lc]):
                zbeam.append(zero)
                continue
            m = [[(1 + (cmu_full[i] * lam[lc] if spher else cmu_full[i] / umu0)
                   if i == j else 0) - ccs[lc][i][j] for j in range(nstr)]
                 for i in range(nstr)]
            zbeam.append(_solve(m, x0s[lc]))

        def zpart(lc, tau):
            if not beam:
                att = mpf(0)
            elif spher:
                att = mp.exp(-(chp[lc] + lam[lc] * (tau - taucpr[lc])))
            else:
                att = mp.exp(-tau / umu0)
            return [z0s[lc][i] + z1s[lc][i] * tau + zbeam[lc][i] * att for i in range(nstr)]

        b = mp.matrix(ncol, 1)
        zp0 = zpart(0, mpf(0))
        for i in range(nn):
            b[i] = fisot + tplanck - zp0[nn + i]
        for lc in range(nlyr - 1):
            za = zpart(lc + 1, taucpr[lc + 1])
            zb = zpart(lc, taucpr[lc + 1])
            for i in range(nstr):
                b[nn + lc * nstr + i] = za[i] - zb[i]
        zb = zpart(nlyr - 1, taucpr[nlyr])
        rhs = (1 - albedo) * bplanck
        if beam:
            rhs += albedo * umu0 * fbeam * mp.exp(-chp[nlyr]) / pi
        rz = sum(refl[m] * zb[nn + m] for m in range(nn))
        for i in range(nn):
            b[r0 + i] = rhs - (zb[i] - rz)
        return b, zp0, zpart

    def record(chp, ch, ll, zp0, zpart):
        uu = []
        for lev in range(nlyr + 1):
            lc = max(lev - 1, 0)
            m = tops[0] if lev == 0 else bots[lc]
            zp = zp0 if lev == 0 else zpart(lc, taucpr[lev])
            uu.append([sum(m[i][j] * ll[lc * nstr + j] for j in range(nstr)) + zp[i]
                       for i in range(nstr)])
        rec = [[mpf(0)] * NFLX for _ in range(nlyr + 1)]
        scale = []
        for lev in range(nlyr + 1):
            r = rec[lev]
            up, dn = uu[lev][:nn], uu[lev][nn:]
            r[IFLUP] = 2 * pi * sum(cwt[i] * cmu[i] * up[i] for i in range(nn))
            dfdn = 2 * pi * sum(cwt[i] * cmu[i] * dn[i] for i in range(nn))
            r[IUAVGUP] = sum(cwt[i] * up[i] for i in range(nn)) / 2
            r[IUAVGDN] = sum(cwt[i] * dn[i] for i in range(nn)) / 2
            if beam:
                r[IRFLDIR] = umu0 * fbeam * mp.exp(-ch[lev])
                sdir = umu0 * fbeam * mp.exp(-chp[lev])
                r[IRFLDN] = dfdn + sdir - r[IRFLDIR]
                r[IUAVGSO] = fbeam * mp.exp(-chp[lev]) / (4 * pi)
            else:
                r[IRFLDN] = dfdn
            r[IUAVG] = r[IUAVGUP] + r[IUAVGDN] + r[IUAVGSO]
            ssa_in = mpf(float(ssalb_d[max(lev - 1, 0)]))  # the input value, not the dithered
            absl = (1 - ssa_in) * 4 * pi
            r[IDFDT] = absl * (r[IUAVG] - pkag[lev])
            scale.append(absl * max(r[IUAVG], pkag[lev]))
        return rec, scale

    paths = [own]
    if geom is not None:
        paths.append(tuple([mpf(float(v)) for v in x] for x in geom))
    parts = [rhs_of(chp, lam) for chp, lam, _ in paths]
    sols = _lu_solve_each(a, [pt[0] for pt in parts])
    recs = [record(chp, ch, list(ll), pt[1], pt[2])
            for (chp, _, ch), ll, pt in zip(paths, sols, parts)]

    rec, scale = recs[0]
    flx = np.array([[float(v) for v in r] for r in rec])
    out = {"flx": flx, "scale": np.array([float(s) for s in scale]),
           "rfldir": flx[:, IRFLDIR], "rfldn": flx[:, IRFLDN], "flup": flx[:, IFLUP],
           "dfdt": flx[:, IDFDT], "uavg": flx[:, IUAVG], "uavgdn": flx[:, IUAVGDN],
           "uavgup": flx[:, IUAVGUP], "uavgso": flx[:, IUAVGSO],
           "fdn": np.array([float(r[IRFLDIR] + r[IRFLDN]) for r in rec])}
    if geom is not None:
        out["flx_geom"] = np.array([[float(v) for v in r] for r in recs[1][0]])
    if return_mp:
        out["mp"] = rec
        out["kk"] = kks
        out["lam"] = own[1]
    return out


def _lu_solve_each(a, bs):
    """``mp.lu_solve(a, b)`` for every b of ``bs`` with one factorisation: the same
    arithmetic (ten guard bits, partial pivoting), the O(n^3) part done once."""
    prec = mp.prec
    try:
        mp.prec += 10
        lu, piv = mp.LU_decomp(a.copy(), overwrite=True)
        return [mp.U_solve(lu, mp.L_solve(lu, b, piv)) for b in bs]
    finally:
        mp.prec = prec


def _slant(zd, radius, umu0, dtaucp, dt):
    """(chp, lam, ch) in solver order (level / layer 0 = top) from the altitudes ``zd``
    (doubles, bottom -> top): with z_m the levels and layer j between z_j and z_{j+1},
        g(l, j) = (2R + z_{j+1} + z_j) / (a(l, j+1) + a(l, j)),
        a(l, m) = sqrt((z_m - z_l)(2R + z_m + z_l) + ((R + z_l) mu0)^2),
    ch(l) = sum_{j >= l} g(l, j) dtau_j."""
    z = [mpf(float(v)) for v in np.asarray(zd, np.float64).ravel()]
    nlyr = len(dt)
    if len(z) != nlyr + 1:
        raise ValueError("zd must hold nlyr + 1 levels")
    r = mpf(float(radius))

    def a(l, m):
        return mp.sqrt((z[m] - z[l]) * (2 * r + z[m] + z[l]) + ((r + z[l]) * umu0) ** 2)

    def g(l, j):
        return (2 * r + z[j + 1] + z[j]) / (a(l, j + 1) + a(l, j))

    def slant(d):  # d top -> bottom; harp layer j is solver layer nlyr - 1 - j
        return [sum((g(l, j) * d[nlyr - 1 - j] for j in range(l, nlyr)), mpf(0))
                for l in range(nlyr, -1, -1)]

    chp, ch = slant(dtaucp), slant(dt)
    lam = [(chp[lc + 1] - chp[lc]) / dtaucp[lc] if dtaucp[lc] > 0
           else g(nlyr - 1 - lc, nlyr - 1 - lc) for lc in range(nlyr)]
    return chp, lam, ch


def layer_eigenvalues(ssa, pmom, nstr, dps=50):
    """The nstr/2 eigenvalues k (mpf, ascending) of one layer after dither and delta-M."""
    with mp.workdps(dps):
        nn = nstr // 2
        pm = [mpf(float(v)) for v in np.asarray(pmom, np.float64).ravel()]
        nmom = len(pm) - 1
        s = mpf(1.0 - DITHER) if float(ssa) == 1.0 else mpf(float(ssa))
        f = pm[nstr] if nmom >= nstr else mpf(0)
        op = s * (1 - f) / (1 - s * f)
        gl = [(2 * k + 1) * op * ((pm[k] if k <= nmom else mpf(0)) - f) / (1 - f)
              for k in range(nstr)]
        cmu, cwt = double_gauss(nn)
        ylm = _legendre(nstr, cmu + [-m for m in cmu])
        _, kk, _, _ = _layer(gl, cmu, cwt, nn, nstr, ylm)
        return sorted(kk)


# --------------------------------------------------------------------------- #
# harp-level drivers (the contract of disort_np.disort_forward)
# --------------------------------------------------------------------------- #
def flx_forward(prop, bc, temf=None, *, nstr, nmom=None, planck=False, wave_lower=None,
                wave_upper=None, dps=50, zd=None, radius=None):
    """prop (W, C, L, nprop), layer / level 0 = bottom; bc: dict of (W, C) arrays; temf
    (C, L+1) bottom -> top; zd (L+1,) or (C, L+1) bottom -> top with radius: the
    pseudo-spherical beam.  Returns (flx (W, C, L+1, 8), scale (W, C, L+1))."""
    prop = np.asarray(prop, np.float64)
    nwave, ncol, nlyr, nprop = prop.shape
    nmom = nstr if nmom is None else nmom
    nm = max(0, min(nmom, nprop - 2))
    zd = None if zd is None else np.asarray(zd, np.float64)

    def bcv(key, default):
        if key in bc and bc[key] is not None:
            return np.broadcast_to(np.asarray(bc[key], np.float64), (nwave, ncol))
        return np.full((nwave, ncol), default)

    keys = dict(fbeam=0.0, umu0=1.0, albedo=0.0, btemp=0.0, ttemp=0.0, temis=0.0, fisot=0.0)
    v = {k: bcv(k, d) for k, d in keys.items()}
    flx = np.zeros((nwave, ncol, nlyr + 1, NFLX))
    scale = np.zeros((nwave, ncol, nlyr + 1))
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
            if zd is not None:
                kw.update(zd=zd[c] if zd.ndim == 2 else zd, radius=radius)
            r = disort_column(p[:, 0], ssa, pm, nstr, umu0=v["umu0"][w, c],
                              fbeam=v["fbeam"][w, c], albedo=v["albedo"][w, c],
                              fisot=v["fisot"][w, c], dps=dps, **kw)
            flx[w, c] = r["flx"][::-1]
            scale[w, c] = r["scale"][::-1]
    return flx, scale


def flux_of_record(flx):
    """(…, 8) record -> (…, 2): upward, rfldir + rfldn (the layout of Disort.forward)."""
    return np.stack([flx[..., IFLUP], flx[..., IRFLDIR] + flx[..., IRFLDN]], axis=-1)


def disort_forward(prop, bc, temf=None, *, nstr, nmom=None, planck=False, wave_lower=None,
                   wave_upper=None, dps=50, zd=None, radius=None):
    """Batch driver with the contract of ``disort_np.disort_forward``: flux
    (W, C, L+1, 2), level 0 = surface, [..., 0] = upward, [..., 1] = rfldir + rfldn."""
    flx, _ = flx_forward(prop, bc, temf, nstr=nstr, nmom=nmom, planck=planck,
                         wave_lower=wave_lower, wave_upper=wave_upper, dps=dps, zd=zd,
                         radius=radius)
    return flux_of_record(flx)
