"""CPU reference of DISORT's full flux record (hd_solve_flx / Disort.forward_flx).

The record (rfldir, rfldn, flup, dfdt, uavg, uavgdn, uavgup, uavgso per level, the
order of cdisort's disort_radiant) rebuilt from the NumPy intensity oracle: the
azimuthally averaged field ``uum[0]`` of ``oracle.disort_rad_np.disort_rad_column`` at
the +-double-Gauss nodes and the layer boundaries, integrated with the quadrature
weights, plus ``setdis`` (scaled depth) and ``plkavg`` (Planck band value).  The oracle
is imported read-only; definitions as in include/hdisort.h.
"""

import math

import numpy as np

from oracle.disort_np import double_gauss, plkavg, setdis
from oracle.disort_rad_np import disort_rad_column

IRFLDIR, IRFLDN, IFLUP, IDFDT, IUAVG, IUAVGDN, IUAVGUP, IUAVGSO = range(8)
NFLX = 8


def flx_ref_column(dtauc, ssalb, pmom, nstr, *, umu0=1.0, fbeam=0.0, albedo=0.0, fisot=0.0,
                   planck=False, temper=None, btemp=0.0, ttemp=0.0, temis=0.0, wvnmlo=0.0,
                   wvnmhi=0.0):
    """One column, layers and levels top -> bottom (cdisort order).

    Returns (flx (nlyr+1, 8), scale (nlyr+1,), own) with scale = (1 - ssa_in) 4 pi
    max(uavg, B_lev), the magnitude dfdt is a difference of, and own = the oracle's own
    flup and rfldir + rfldn (for identity checks).

    Every component comes from the nodes' field: flup = 2 pi sum w mu I+ and the diffuse
    downward flux 2 pi sum w mu I- (equal to the oracle's own flup / fdn to rounding,
    tests/test_flx_ref.py, but exact zeros where the field is zero -- a black surface,
    a dark top -- where the oracle's general solution leaves 1e-14 of the field).
    rfldn = total - rfldir with the two direct terms' difference through expm1.
    """
    dtauc = np.atleast_1d(np.asarray(dtauc, np.float64))
    ssalb = np.atleast_1d(np.asarray(ssalb, np.float64))
    nlyr = dtauc.size
    nn = nstr // 2
    pmom = np.asarray(pmom, np.float64).reshape(nlyr, -1)
    cmu, cwt = double_gauss(nn)
    umu = np.concatenate([-cmu, cmu])
    utau = np.concatenate([[0.0], np.cumsum(dtauc)])
    kw = {}
    if planck:
        kw = dict(planck=True, temper=temper, btemp=btemp, ttemp=ttemp, temis=temis,
                  wvnmlo=wvnmlo, wvnmhi=wvnmhi)
    r = disort_rad_column(dtauc, ssalb, pmom, nstr, umu=umu, phi=[0.0], utau=utau, umu0=umu0,
                          fbeam=fbeam, albedo=albedo, fisot=fisot, **kw)
    u0 = r["uum"][0]                      # (nlyr+1, 2 nn), mode 0 at the nodes
    idn, iup = u0[:, :nn], u0[:, nn:]
    _, taucpr, tauc, _, _ = setdis(dtauc, ssalb, pmom, nstr)
    beam = fbeam > 0.0
    flx = np.zeros((nlyr + 1, NFLX))
    flx[:, IFLUP] = 2.0 * math.pi * (iup * cwt * cmu).sum(axis=1)
    flx[:, IRFLDIR] = umu0 * fbeam * np.exp(-tauc / umu0) if beam else 0.0
    # total down = scaled diffuse + scaled direct; minus the unscaled direct beam
    flx[:, IRFLDN] = 2.0 * math.pi * (idn * cwt * cmu).sum(axis=1) + \
        (flx[:, IRFLDIR] * np.expm1((tauc - taucpr) / umu0) if beam else 0.0)
    flx[:, IUAVGUP] = 0.5 * (iup * cwt).sum(axis=1)
    flx[:, IUAVGDN] = 0.5 * (idn * cwt).sum(axis=1)
    flx[:, IUAVGSO] = fbeam * np.exp(-taucpr / umu0) / (4.0 * math.pi) if beam else 0.0
    flx[:, IUAVG] = flx[:, IUAVGUP] + flx[:, IUAVGDN] + flx[:, IUAVGSO]
    blev = np.array([plkavg(wvnmlo, wvnmhi, t) for t in temper]) if planck \
        else np.zeros(nlyr + 1)
    # the layer directly above the level; the top level takes the top layer
    ssa_in = np.concatenate([ssalb[:1], ssalb])
    absl = (1.0 - ssa_in) * 4.0 * math.pi
    flx[:, IDFDT] = absl * (flx[:, IUAVG] - blev)
    scale = absl * np.maximum(flx[:, IUAVG], blev)
    own = np.stack([r["flup"], r["fdn"]], axis=1)
    return flx, scale, own


def flx_ref_forward(prop, bc, temf=None, *, nstr, nmom=None, planck=False, wave_lower=None,
                    wave_upper=None):
    """Batch driver in harp's layout (prop (W, C, L, nprop), layer / level 0 = bottom).
    Returns (flx (W, C, L+1, 8), scale (W, C, L+1))."""
    prop = np.asarray(prop, np.float64)
    nwave, ncol, nlyr, nprop = prop.shape
    nmom = nstr if nmom is None else nmom
    nm = max(0, min(nmom, nprop - 2))

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
            f, s, _ = flx_ref_column(p[:, 0], ssa, pm, nstr, umu0=v["umu0"][w, c],
                                     fbeam=v["fbeam"][w, c], albedo=v["albedo"][w, c],
                                     fisot=v["fisot"][w, c], **kw)
            flx[w, c] = f[::-1]
            scale[w, c] = s[::-1]
    return flx, scale


# --------------------------------------------------------------------------- #
# the parity cases of tests/test_gpu_flx.py (inputs + this helper's record, stored in
# tests/golden/flx_parity.npz by tests/golden/make_flx_golden.py: the intensity oracle
# takes 0.3 s a column at nstr 16 and 1.5 s at nstr 32, too long to run in every case)
# --------------------------------------------------------------------------- #
PARITY_NSTR = (2, 4, 8, 16, 18, 24, 32)
PARITY_NLYR = (1, 2, 5)
PARITY_SOURCES = ("beam", "planck", "beam_planck", "fisot")
PARITY_WAVES = ((300.0, 800.0), (800.0, 1200.0))


def parity_key(nstr, nlyr, source):
    return f"n{nstr}_l{nlyr}_{source}"


def parity_inputs(nstr, nlyr, source):
    """2 waves x 3 columns, every solve its own optics: Henyey-Greenstein g = 0.8 with
    nmom = nstr (delta-M active: f = g^nstr), albedo 0 / 0.5 / 1 by column, one
    conservative layer and one of tau = 1e-6 per solve.  Returns (prop, bc, temf).

    With more than one layer the conservative layer is in the columns of albedo 0 and 0.5
    and the thin one in those of albedo 0.5 and 1: a conservative layer over a surface of
    albedo 1 with nothing else but a layer of tau = 1e-6 is a cavity that loses energy only
    through the dither (1 - ssa = 4.7e-8), its thermal level is a ratio of two such
    numbers, and the repository's three CPU solvers (C restatement, NumPy flux oracle,
    this helper) then differ by 2e-6 to 1e-5 among themselves -- no reference to TOL.
    With one layer a solve has one or the other, and the thin one only without a beam:
    rfldn is the total minus rfldir, so in a beam-lit column of tau = 1e-6 (rfldn about
    1e-7 rfldir) FP64 leaves it 1e-9 relative, while the per-component metric asks
    1e-12 of the component's own scale below its floor."""
    nwave, ncol = 2, 3
    rng = np.random.default_rng(1000 * nstr + 10 * nlyr + PARITY_SOURCES.index(source))
    prop = np.zeros((nwave, ncol, nlyr, 2 + nstr))
    prop[..., 0] = 10.0 ** rng.uniform(-1.5, 0.7, (nwave, ncol, nlyr))
    prop[..., 1] = rng.uniform(0.05, 0.98, (nwave, ncol, nlyr))
    for l in range(nstr):
        prop[..., 2 + l] = 0.8 ** (l + 1)
    for w in range(nwave):
        for c in range(ncol):
            q = w * ncol + c
            if nlyr > 1:  # by column, so that temf (per column) can follow the thin layer
                if c < 2:   # albedo 0 and 0.5
                    prop[w, c, c % nlyr, 1] = 1.0
                if c > 0:   # albedo 0.5 and 1
                    prop[w, c, (c + 1) % nlyr, 0] = 1.0e-6
            elif q % 2 == 0:
                prop[w, c, 0, 1] = 1.0
            elif "beam" not in source:
                prop[w, c, 0, 0] = 1.0e-6
    bc = {"albedo": np.broadcast_to(np.array([0.0, 0.5, 1.0]), (nwave, ncol)).copy()}
    temf = None
    if "beam" in source:
        bc["fbeam"] = rng.uniform(0.5, 2.0, (nwave, ncol))
        bc["umu0"] = rng.uniform(0.2, 1.0, (nwave, ncol))
    if "planck" in source:
        temf = np.sort(rng.uniform(200.0, 300.0, (ncol, nlyr + 1)), axis=1)[:, ::-1].copy()
        if nlyr > 1:
            # no temperature step across the layer of tau = 1e-6: tens of kelvin there are
            # a Planck slope dB/dtau of 1e7 B, which no FP64 solve (the oracle's included)
            # resolves to the metric's 1e-12 of the component scale
            for c in range(1, ncol):
                k = (c + 1) % nlyr
                temf[c, k + 1] = temf[c, k]
        bc["btemp"] = np.broadcast_to(temf[:, 0] + 5.0, (nwave, ncol)).copy()
        bc["ttemp"] = np.full((nwave, ncol), 150.0)
        bc["temis"] = np.full((nwave, ncol), 0.5)
    if source == "fisot":
        bc["fisot"] = rng.uniform(0.5, 2.0, (nwave, ncol))
    return prop, bc, temf


def parity_reference(nstr, nlyr, source):
    prop, bc, temf = parity_inputs(nstr, nlyr, source)
    planck = "planck" in source
    return flx_ref_forward(prop, bc, temf, nstr=nstr, planck=planck,
                           wave_lower=[w[0] for w in PARITY_WAVES],
                           wave_upper=[w[1] for w in PARITY_WAVES])
