"""CPU reference of the pseudo-spherical flux solve (hd_solve_spher / hd_solve_flx_spher).

The model of DESIGN.md section 3e: the direct beam is attenuated along its true path
through spherical shells, multiple scattering stays plane-parallel, and inside a layer
the beam is one exponential in tau' fitted to the slant depths at the layer's two
boundaries (the layer-average secant of Dahlback & Stamnes 1991 -- not cdisort 2.1.3's
exponential-linear fit).  ``spher_column`` is ``oracle.disort_np.disort_column``'s banded
system with that beam; the stage functions are imported from the oracle read-only.

Conventions: ``zd`` is always bottom -> top (the library's order, as ``temf``); the layer
arguments of ``chapman`` are bottom -> top too (harp order), those of ``spher_column`` top
-> bottom (cdisort order, as ``disort_column``).
"""

import math

import numpy as np
import scipy.linalg

from oracle.disort_np import (_cc_matrix, double_gauss, legendre_table, plkavg, setdis, soleig,
                              upisot)

IRFLDIR, IRFLDN, IFLUP, IDFDT, IUAVG, IUAVGDN, IUAVGUP, IUAVGSO = range(8)
NFLX = 8


def geometric_factors(zd, radius, umu0):
    """g[l, j] for levels l = 0..nlyr and layers j >= l (zero below the diagonal):
    g(l, j) = (2R + z_{j+1} + z_j) / (a(l, j+1) + a(l, j)),
    a(l, m) = sqrt((z_m - z_l)(2R + z_m + z_l) + ((R + z_l) mu0)^2)."""
    z = np.asarray(zd, np.float64)
    nlyr = z.size - 1
    g = np.zeros((nlyr + 1, nlyr))
    for l in range(nlyr + 1):
        a = np.sqrt((z[l:] - z[l]) * (2.0 * radius + z[l:] + z[l]) + ((radius + z[l]) * umu0) ** 2)
        for j in range(l, nlyr):
            g[l, j] = (2.0 * radius + z[j + 1] + z[j]) / (a[j + 1 - l] + a[j - l])
    return g


def chapman(zd, radius, umu0, dtau):
    """Slant optical depth ch[l] from the top of the atmosphere to level l along the beam,
    levels and layers bottom -> top (layer j between levels j and j+1); ch[nlyr] = 0."""
    return geometric_factors(zd, radius, umu0) @ np.asarray(dtau, np.float64)


def layer_secants(zd, radius, umu0, dtaucp):
    """(chp, lam) in cdisort order: chp[lc] the slant depth on the scaled layer depths
    ``dtaucp`` (top -> bottom) at solver level lc (0 = top), lam[lc] the secant of solver
    layer lc: (chp[lc+1] - chp[lc]) / dtaucp[lc], or g(j, j) for a layer of zero depth."""
    dtaucp = np.asarray(dtaucp, np.float64)
    nlyr = dtaucp.size
    g = geometric_factors(zd, radius, umu0)
    chp = (g @ dtaucp[::-1])[::-1]
    lam = np.zeros(nlyr)
    for lc in range(nlyr):
        j = nlyr - 1 - lc
        lam[lc] = (chp[lc + 1] - chp[lc]) / dtaucp[lc] if dtaucp[lc] > 0.0 else g[j, j]
    return chp, lam


def spher_column(dtauc, ssalb, pmom, nstr, *, zd, radius, umu0=1.0, fbeam=0.0, albedo=0.0,
                 fisot=0.0, planck=False, temper=None, btemp=0.0, ttemp=0.0, temis=0.0,
                 wvnmlo=0.0, wvnmhi=0.0):
    """One pseudo-spherical solve, layers and levels top -> bottom (zd bottom -> top).

    Returns a dict: flup, fdn (= the direct flux on the scaled depth + diffuse down),
    rfldir, rfldn, the full record ``flx`` (nlyr+1, 8), ``scale`` (the magnitude dfdt is a
    difference of, as tests/flx_ref.py), chp, ch (scaled / unscaled slant depths) and lam.
    """
    dtauc = np.atleast_1d(np.asarray(dtauc, np.float64))
    ssalb = np.atleast_1d(np.asarray(ssalb, np.float64))
    nlyr = dtauc.size
    nn = nstr // 2
    pmom = np.asarray(pmom, np.float64).reshape(nlyr, -1)
    cmu, cwt = double_gauss(nn)
    cmu_full = np.concatenate([cmu, -cmu])
    cwt_full = np.concatenate([cwt, cwt])
    ylm = legendre_table(nstr, cmu_full)
    dtaucp, taucpr, tauc, oprim, gl = setdis(dtauc, ssalb, pmom, nstr)
    if fbeam > 0.0 and not (0.0 < umu0 <= 1.0):
        raise ValueError(f"umu0 = {umu0} outside (0, 1] with fbeam > 0")
    beam = fbeam > 0.0
    if beam:
        chp, lam = layer_secants(zd, radius, umu0, dtaucp)
        ch = chapman(zd, radius, umu0, dtauc[::-1])[::-1]
    else:
        chp, lam, ch = np.zeros(nlyr + 1), np.zeros(nlyr), np.zeros(nlyr + 1)
    if planck:
        pkag = np.array([plkavg(wvnmlo, wvnmhi, t) for t in temper])
        bplanck = plkavg(wvnmlo, wvnmhi, btemp)
        tplanck = plkavg(wvnmlo, wvnmhi, ttemp) * temis
    else:
        pkag = np.zeros(nlyr + 1)
        bplanck = tplanck = 0.0

    kk = np.zeros((nlyr, nn))
    gc = np.zeros((nlyr, nstr, nstr))
    zbeam = np.zeros((nlyr, nstr))
    z0 = np.zeros((nlyr, nstr))
    z1 = np.zeros((nlyr, nstr))
    p0 = legendre_table(nstr, [-umu0])[:, 0]
    for lc in range(nlyr):
        cc = _cc_matrix(gl[lc], cmu_full, cwt_full, ylm)
        k, gp, gm = soleig(cc, cmu)
        kk[lc] = k
        gc[lc, :nn, :nn] = gp
        gc[lc, nn:, :nn] = gm
        gc[lc, :nn, nn:] = gm
        gc[lc, nn:, nn:] = gp
        if beam:
            x0 = fbeam / (4.0 * math.pi) * (ylm.T @ (gl[lc] * p0))
            zbeam[lc] = np.linalg.solve(np.diag(1.0 + cmu_full * lam[lc]) - cc, x0)
        if planck:
            xr1 = (pkag[lc + 1] - pkag[lc]) / dtaucp[lc] if dtaucp[lc] > 0 else 0.0
            xr0 = pkag[lc] - xr1 * taucpr[lc]
            z0[lc], z1[lc] = upisot(cc, cmu_full, oprim[lc], xr0, xr1)

    def zpart(lc, tau):
        v = z0[lc] + z1[lc] * tau
        if beam:
            v = v + zbeam[lc] * math.exp(-chp[lc] - lam[lc] * (tau - taucpr[lc]))
        return v

    ee = np.exp(-kk * dtaucp[:, None])
    ncol = nstr * nlyr
    a = np.zeros((ncol, ncol))
    b = np.zeros(ncol)

    def top_cols(lc):
        return gc[lc] * np.concatenate([np.ones(nn), ee[lc]])[None, :]

    def bot_cols(lc):
        return gc[lc] * np.concatenate([ee[lc], np.ones(nn)])[None, :]

    t0 = top_cols(0)
    a[:nn, :nstr] = t0[nn:, :]
    b[:nn] = fisot + tplanck - zpart(0, 0.0)[nn:]
    for lc in range(nlyr - 1):
        r0 = nn + lc * nstr
        a[r0:r0 + nstr, lc * nstr:(lc + 1) * nstr] = bot_cols(lc)
        a[r0:r0 + nstr, (lc + 1) * nstr:(lc + 2) * nstr] = -top_cols(lc + 1)
        tau = taucpr[lc + 1]
        b[r0:r0 + nstr] = zpart(lc + 1, tau) - zpart(lc, tau)
    r0 = nn + (nlyr - 1) * nstr
    lb = bot_cols(nlyr - 1)
    refl = 2.0 * albedo * (cwt * cmu)
    a[r0:r0 + nn, (nlyr - 1) * nstr:] = lb[:nn, :] - refl[None, :] @ lb[nn:, :]
    zb = zpart(nlyr - 1, taucpr[nlyr])
    rhs = np.full(nn, (1.0 - albedo) * bplanck)
    if beam:
        rhs += albedo * umu0 * fbeam * math.exp(-chp[nlyr]) / math.pi
    b[r0:r0 + nn] = rhs - (zb[:nn] - refl @ zb[nn:])

    bw = 3 * nn - 1
    ab = np.zeros((2 * bw + 1, ncol))
    for j in range(ncol):
        lo = max(0, j - bw)
        hi = min(ncol, j + bw + 1)
        ab[bw + lo - j:bw + hi - j, j] = a[lo:hi, j]
    ll = scipy.linalg.solve_banded((bw, bw), ab, b).reshape(nlyr, nstr)

    uu = np.zeros((nlyr + 1, nstr))
    uu[0] = top_cols(0) @ ll[0] + zpart(0, 0.0)
    for lc in range(nlyr):
        uu[lc + 1] = bot_cols(lc) @ ll[lc] + zpart(lc, taucpr[lc + 1])
    iup, idn = uu[:, :nn], uu[:, nn:]
    wmu = cwt * cmu
    flx = np.zeros((nlyr + 1, NFLX))
    flx[:, IFLUP] = 2.0 * math.pi * iup @ wmu
    dfdn = 2.0 * math.pi * idn @ wmu
    dirp = umu0 * fbeam * np.exp(-chp) if beam else np.zeros(nlyr + 1)
    flx[:, IRFLDIR] = umu0 * fbeam * np.exp(-ch) if beam else 0.0
    fdn = dfdn + dirp
    flx[:, IRFLDN] = fdn - flx[:, IRFLDIR]
    flx[:, IUAVGUP] = 0.5 * iup @ cwt
    flx[:, IUAVGDN] = 0.5 * idn @ cwt
    flx[:, IUAVGSO] = fbeam * np.exp(-chp) / (4.0 * math.pi) if beam else 0.0
    flx[:, IUAVG] = flx[:, IUAVGUP] + flx[:, IUAVGDN] + flx[:, IUAVGSO]
    ssa_in = np.concatenate([ssalb[:1], ssalb])
    absl = (1.0 - ssa_in) * 4.0 * math.pi
    flx[:, IDFDT] = absl * (flx[:, IUAVG] - pkag)
    scale = absl * np.maximum(flx[:, IUAVG], pkag)
    return {"flup": flx[:, IFLUP].copy(), "fdn": fdn, "rfldir": flx[:, IRFLDIR].copy(),
            "rfldn": flx[:, IRFLDN].copy(), "flx": flx, "scale": scale, "chp": chp, "ch": ch,
            "lam": lam, "taucpr": taucpr, "dtaucp": dtaucp}


def spher_forward(prop, bc, temf=None, *, zd, radius, nstr, nmom=None, planck=False,
                  wave_lower=None, wave_upper=None):
    """Batch driver in harp's layout: prop (W, C, L, nprop), layer / level 0 = bottom; zd
    (L+1,) or (C, L+1), bottom -> top.  Returns (flux (W, C, L+1, 2), flx (W, C, L+1, 8),
    scale (W, C, L+1))."""
    prop = np.asarray(prop, np.float64)
    nwave, ncol, nlyr, nprop = prop.shape
    nmom = nstr if nmom is None else nmom
    nm = max(0, min(nmom, nprop - 2))
    zd = np.asarray(zd, np.float64)

    def bcv(key, default):
        if key in bc and bc[key] is not None:
            return np.broadcast_to(np.asarray(bc[key], np.float64), (nwave, ncol))
        return np.full((nwave, ncol), default)

    keys = dict(fbeam=0.0, umu0=1.0, albedo=0.0, btemp=0.0, ttemp=0.0, temis=0.0, fisot=0.0)
    v = {k: bcv(k, d) for k, d in keys.items()}
    flux = np.zeros((nwave, ncol, nlyr + 1, 2))
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
            r = spher_column(p[:, 0], ssa, pm, nstr, zd=zd[c] if zd.ndim == 2 else zd,
                             radius=radius, umu0=v["umu0"][w, c], fbeam=v["fbeam"][w, c],
                             albedo=v["albedo"][w, c], fisot=v["fisot"][w, c], **kw)
            flux[w, c, :, 0] = r["flup"][::-1]
            flux[w, c, :, 1] = r["fdn"][::-1]
            flx[w, c] = r["flx"][::-1]
            scale[w, c] = r["scale"][::-1]
    return flux, flx, scale


def propagator_column(dtauc, ssalb, pmom, nstr, *, zd, radius, umu0, fbeam, albedo=0.0):
    """The same beam-only problem without the eigen-solution: the 2N-stream equation
        mu_i dI_i/dtau = I_i - sum_j CC_ij I_j - x0_i(mu0) F0/(4 pi) e^{-ch'(tau)}
    with ch' piecewise linear in tau' (slope lam in each layer), integrated exactly through
    every layer by the matrix exponential of the system augmented with s = e^{-ch'(tau)}
    (ds/dtau = -lam s), then the same two boundary conditions (no diffuse light at the top,
    Lambert surface lit by albedo mu0 F0 e^{-ch'_0} / pi).  Returns (flup, fdn), top ->
    bottom."""
    dtauc = np.atleast_1d(np.asarray(dtauc, np.float64))
    nlyr = dtauc.size
    nn = nstr // 2
    pmom = np.asarray(pmom, np.float64).reshape(nlyr, -1)
    cmu, cwt = double_gauss(nn)
    cmu_full = np.concatenate([cmu, -cmu])
    cwt_full = np.concatenate([cwt, cwt])
    ylm = legendre_table(nstr, cmu_full)
    dtaucp, taucpr, _, _, gl = setdis(dtauc, ssalb, pmom, nstr)
    chp, lam = layer_secants(zd, radius, umu0, dtaucp)
    p0 = legendre_table(nstr, [-umu0])[:, 0]
    # y = [I (nstr); s], y(level lc+1) = props[lc] y(level lc)
    props = []
    for lc in range(nlyr):
        cc = _cc_matrix(gl[lc], cmu_full, cwt_full, ylm)
        x0 = fbeam / (4.0 * math.pi) * (ylm.T @ (gl[lc] * p0))
        m = np.zeros((nstr + 1, nstr + 1))
        m[:nstr, :nstr] = (np.eye(nstr) - cc) / cmu_full[:, None]
        m[:nstr, nstr] = -x0 / cmu_full
        m[nstr, nstr] = -lam[lc]
        props.append(scipy.linalg.expm(m * dtaucp[lc]))
    # y(top) = e_s + sum_k u_k e_k over the nn unknown upward intensities (no diffuse down)
    basis = np.zeros((nstr + 1, nn + 1))
    basis[nstr, 0] = 1.0
    for k in range(nn):
        basis[k, 1 + k] = 1.0
    levels = [basis]
    for lc in range(nlyr):
        levels.append(props[lc] @ levels[-1])
    bot = levels[-1]
    refl = 2.0 * albedo * (cwt * cmu)
    # I_up - refl . I_dn - albedo mu0 F0 s / pi = 0 at the surface
    row = bot[:nn] - np.outer(np.ones(nn), refl @ bot[nn:nstr]) \
        - albedo * umu0 * fbeam / math.pi * np.outer(np.ones(nn), bot[nstr])
    u = np.linalg.solve(row[:, 1:], -row[:, 0])
    coef = np.concatenate([[1.0], u])
    wmu = cwt * cmu
    flup = np.zeros(nlyr + 1)
    fdn = np.zeros(nlyr + 1)
    for lv in range(nlyr + 1):
        y = levels[lv] @ coef
        flup[lv] = 2.0 * math.pi * y[:nn] @ wmu
        fdn[lv] = 2.0 * math.pi * y[nn:nstr] @ wmu + umu0 * fbeam * y[nstr]
    return flup, fdn, chp, lam


# --------------------------------------------------------------------------- #
# the batch of tests/test_gpu_spher.py (inputs only; the reference is run there, once)
# --------------------------------------------------------------------------- #
RADIUS = 3.39e6                       # a Mars-sized body, metres
ZD = 2.0e4 * np.arange(6.0)           # levels every 20 km up to 100 km
UMU0 = (1.0, 0.5, 0.1, 0.02)          # by column
TAU_PROFILES = {"uniform": (0.3, 0.3, 0.3, 0.3, 0.3),
                "thin_bottom": (1.0e-3, 1.0e-3, 0.5, 0.5, 0.5)}  # bottom -> top
WAVES = ((300.0, 800.0), (800.0, 1200.0))


def batch_inputs(nstr, profile, planck, per_column=False):
    """nwave 2 x ncol 4 x nlyr 5: Henyey-Greenstein moments with nmom = nstr (delta-M
    active), albedo 0.3, mu0 by column, one layer of dtau = 0 exactly in column 1.  With
    per_column every column has its own altitudes (the shared grid stretched by up to
    15 %).  Returns (prop, bc, temf, zd)."""
    nwave, ncol, nlyr = 2, len(UMU0), 5
    rng = np.random.default_rng(100 * nstr + (7 if planck else 0) +
                                list(TAU_PROFILES).index(profile))
    prop = np.zeros((nwave, ncol, nlyr, 2 + nstr))
    prop[..., 0] = np.asarray(TAU_PROFILES[profile])
    prop[:, 1, 3, 0] = 0.0
    prop[..., 1] = rng.uniform(0.3, 0.95, (nwave, ncol, nlyr))
    gg = rng.uniform(0.3, 0.8, (nwave, ncol, nlyr))
    for l in range(nstr):
        prop[..., 2 + l] = gg ** (l + 1)
    bc = {"fbeam": rng.uniform(0.5, 2.0, (nwave, ncol)),
          "umu0": np.broadcast_to(np.asarray(UMU0), (nwave, ncol)).copy(),
          "albedo": np.full((nwave, ncol), 0.3)}
    temf = None
    if planck:
        temf = np.sort(rng.uniform(200.0, 300.0, (ncol, nlyr + 1)), axis=1)[:, ::-1].copy()
        bc["btemp"] = np.broadcast_to(temf[:, 0] + 5.0, (nwave, ncol)).copy()
        bc["ttemp"] = np.full((nwave, ncol), 150.0)
        bc["temis"] = np.full((nwave, ncol), 0.5)
    zd = ZD.copy()
    if per_column:
        zd = ZD[None, :] * (1.0 + 0.05 * np.arange(ncol))[:, None]
    return prop, bc, temf, zd
