"""Numpy model of the HIP kernels' *formulation* (test-side only).

This mirrors, step by step, what ``pyharp_amd/csrc/hd_kernels.hip`` computes so
that a formulation error can be separated from a kernel-coding error.  It is
NOT the oracle (``oracle/disort_np.py`` is, with DISORT's own structure) and is
never imported by the product.

Formulation:
  * homogeneous solution from the symmetrised eigenproblem
      L L^T = D^1/2 (W^-1 - S-) D^1/2,   C C^T = D^1/2 (W^-1 - S+) D^1/2,
      Sym = L^T C C^T L = X X^T with X = L^T C;  the kernel's one-sided
    Jacobi rotates X's columns into B = X W (orthogonal columns), so
    k^2 = |b_j|^2, V = B K^-1 and U = L V (here V comes from eigh of X X^T)
  * layer operators in the flux-weighted basis, Omega = U Delta^1/2,
    Psi^T = L^-T V Gamma^1/2, and by Woodbury
      A- = (I + Omega Omega^T)^-1, A+ = (I + Psi^T Psi)^-1,
      R~ = A+ - A-,  T~ = A- + A+ - I,  Q~- = I - A-,  Q~+ = A+ - I
  * sources from the beam/thermal particular solutions
  * adding sweep top->bottom (R_above, S_down), scalar Lambert surface,
    back-substitution bottom->top.
"""

import math

import numpy as np

from oracle.disort_np import DITHER, double_gauss, legendre_table, plkavg

# The two cold branches of the flux layer kernels, with the
# kernels' constants (hd_device.hpp kResMove / kThinTau); scripts/hard_threshold_sweep.py
# sweeps both against the mp reference.
#
# RES_MOVE: where |1/mu0^2 - k_j^2| < RES_MOVE / mu0^2 for a mode j of the layer, the layer
# is solved for the secant 1/mu0'^2 = k_j^2 (1 +- RES_MOVE) (the side mu0 is on) wherever
# the resonant mode's amplitude goes: the denominators, the difference part of the
# particular solution and the beam's attenuation inside the layer.  RES_CLAMP is the
# earlier rule (the one denominator clamped at +-1e-9 / mu0^2, nothing else moved), kept
# for the sweep: it drops that mode's share of the beam source.
#
# With the pseudo-spherical beam (``zd``) the layer's secant lambda (any sign) stands where
# 1/mu0 does, and the move keeps its sign: lambda' = sign(lambda) k_j sqrt(1 +- RES_MOVE).
# KEEP_SIGN = False is the plain path's rule (sqrt alone) carried over as it stands, kept
# to show what it costs where lambda < 0 (tests/test_kernel_model.py).
RES_MOVE = 3.0e-8
RES_CLAMP = None
KEEP_SIGN = True
E0_CAP = 600.0  # hd_device.hpp kE0Cap
# THIN_TAU: in a layer of scaled depth 0 < tau' < THIN_TAU the slope part of the thermal
# source, x = g 2 (dB / tau') h, goes through Q~- = A- Omega Omega^T (products only)
# instead of Q~- = I - A- (a difference of O(1) numbers for an O(tau') result, which under
# dB / tau' leaves an error eps dB / tau').  0: the difference form everywhere, the
# earlier rule.  tau' = 0 carries the top level's value through, as before.
THIN_TAU = 1.0e-3


def layer_ops(dtau, ssa, chi, nstr, umu0, fbeam, b_top, b_bot, tauc_top, lam=None, ch=None):
    """lam, ch (pseudo-spherical beam): the layer's secant in place of 1/mu0 and the slant
    depths ch' at its top and bottom in place of tauc_top / mu0."""
    nn = nstr // 2
    mu, w = double_gauss(nn)
    if ssa == 1.0:
        ssa = 1.0 - DITHER
    nmom = len(chi)
    f = chi[nstr - 1] if nmom >= nstr else 0.0
    taup = (1.0 - ssa * f) * dtau
    om = ssa * (1.0 - f) / (1.0 - ssa * f)
    gl = np.array([(2 * l + 1) * om * ((1.0 if l == 0 else (chi[l - 1] if l - 1 < nmom else 0.0)) - f) / (1.0 - f)
                   for l in range(nstr)])
    pt = legendre_table(nstr, mu)  # (nstr, nn)
    ev = np.arange(nstr) % 2 == 0
    splus = (pt[ev].T * gl[ev]) @ pt[ev]
    sminus = (pt[~ev].T * gl[~ev]) @ pt[~ev]
    d = w / mu
    sd = np.sqrt(d)
    am = np.diag(1.0 / mu) - sd[:, None] * sminus * sd[None, :]
    ap = np.diag(1.0 / mu) - sd[:, None] * splus * sd[None, :]
    lch = np.linalg.cholesky(am)
    # one-sided Jacobi view (hd_layer_kernel): C C^T = -A+, X = L^T C, Sym = X X^T;
    # the rotations give B = X W with k^2 = |b_j|^2, V = B K^-1 and U = L V
    cch = np.linalg.cholesky(ap)
    x = lch.T @ cch
    _, wv = np.linalg.eigh(x.T @ x)
    bcols = x @ wv
    k2 = np.sum(bcols * bcols, axis=0)
    k = np.sqrt(k2)
    u = lch @ (bcols / k[None, :])            # U = L V = L B K^-1
    # ---- layer operators in the flux-weighted basis (g = sqrt(w mu)) ----
    e = np.exp(-k * taup)
    m = -np.expm1(-k * taup)
    th = m / (1.0 + e)                        # tanh(k tau'/2)
    delta = np.where(k * taup > 1e-8, th / np.where(k > 0, k, 1.0), 0.5 * taup)
    gamma = k * th
    omega = u * np.sqrt(delta)[None, :]       # Omega = U Delta^1/2
    vv = np.linalg.solve(lch, u)              # V = L^-1 U
    psit = np.linalg.solve(lch.T, vv) * np.sqrt(gamma)[None, :]   # Psi^T = L^-T V Gamma^1/2
    # Woodbury: Q~- = I - A-, Q~+ = A+ - I with A- = (I + Omega Omega^T)^-1,
    # A+ = (I + Psi^T Psi)^-1 (two SPD inverses from Cholesky factors)
    aminus = np.linalg.inv(np.eye(nn) + omega @ omega.T)
    aplus = np.linalg.inv(np.eye(nn) + psit @ psit.T)
    qtm = np.eye(nn) - aminus
    qtp = aplus - np.eye(nn)
    g = np.sqrt(w * mu)
    rt = aplus - aminus                       # R~ (symmetric)
    tt_ = aminus + aplus - np.eye(nn)         # T~ (symmetric)

    def linv(vec):   # W^-1 D^1/2 L^-T L^-1 D^1/2 vec
        z = np.linalg.solve(lch, sd * vec)
        z = np.linalg.solve(lch.T, z)
        return sd * z / w

    zp = np.zeros(nn)
    zm = np.zeros(nn)
    e0 = 1.0
    if fbeam > 0 and umu0 > 0:
        rl = 1.0 / umu0 if lam is None else lam
        r2 = 1.0 / umu0 ** 2 if lam is None else rl * rl
        den = r2 - k2
        rmu0 = rl
        moved = False
        if RES_CLAMP is not None:
            small = np.abs(den) < RES_CLAMP * r2
            den = np.where(small, np.where(den < 0.0, -RES_CLAMP * r2, RES_CLAMP * r2), den)
        else:
            j = int(np.argmin(np.abs(r2 - k2)))  # the mode nearest the resonance
            if abs(r2 - k2[j]) < RES_MOVE * r2:
                r2m = k2[j] * (1.0 - RES_MOVE if r2 < k2[j] else 1.0 + RES_MOVE)
                rmu0 = math.sqrt(r2m)
                if lam is not None and KEEP_SIGN:
                    rmu0 = math.copysign(rmu0, rl)
                moved = True
                den = r2m - k2
        e0_cap = None
        if lam is None:
            e0 = math.exp(-taup * rmu0)
        else:
            # off resonance the layer's transmission is the difference of its two depths.
            # Under a much thicker layer the slant depth falls through the layer; where it
            # falls by more than E0_CAP the transmission is held at exp(E0_CAP) and the
            # amplitude at the top lowered to match, so that the bottom's, exp(-ch'_bottom),
            # is right and the top's (below exp(-E0_CAP) of it) is merely small
            d = 0.0 if not taup > 0.0 else (-taup * rmu0 if moved else ch[0] - ch[1])
            if d > E0_CAP:
                d, e0_cap = E0_CAP, math.exp(-((ch[1] if taup > 0.0 else ch[0]) + E0_CAP))
            e0 = math.exp(d) if taup > 0.0 else 1.0
        p0 = legendre_table(nstr, [umu0])[:, 0]
        xs = fbeam / (2 * math.pi) * (pt[ev].T @ (gl[ev] * p0[ev]))
        xd = -fbeam / (2 * math.pi) * (pt[~ev].T @ (gl[~ev] * p0[~ev]))
        rv = -(1.0 / (mu * sd)) * (lch @ (lch.T @ (sd * xs))) + (xd / (mu * umu0) if lam is None else xd * rl / mu)
        ttv = u.T @ np.linalg.solve(lch.T, np.linalg.solve(lch, (w / sd) * rv))   # V^T y2 = U^T L^-T y2
        ttv = ttv / den
        svec = (sd / w) * (u @ ttv)           # X tt, X = W^-1 D^1/2 L V = W^-1 D^1/2 U
        dd = linv(xd - mu * svec * rmu0)
        att = math.exp(-tauc_top / umu0) if lam is None else math.exp(-ch[0])
        if e0_cap is not None:
            att = e0_cap
        zp = 0.5 * (svec + dd) * att
        zm = 0.5 * (svec - dd) * att
    if not taup > 0.0:
        b_bot = b_top
    db = b_bot - b_top
    bsum = b_top + b_bot
    thin = 0.0 < taup < THIN_TAU
    cslope = np.zeros(nn)
    if b_top != 0.0 or b_bot != 0.0:
        b1 = db / taup if taup > 0 else 0.0
        cslope = 2.0 * b1 * linv(mu)
    avec = zm - zp * e0
    bvec = zm + zp * e0
    if thin:
        # Q~- = I - A- = A- Omega Omega^T: no difference of O(1) numbers under dB / tau'
        pv = qtm @ (g * (db - avec)) + aminus @ (omega @ (omega.T @ (g * cslope)))
    else:
        pv = qtm @ (g * (db + cslope - avec))
    qv = qtp @ (g * (bvec + bsum))
    splus_src = g * (zp * (1 - e0) - db) + pv - qv
    sminus_src = g * (-zm * (1 - e0) + db) - pv - qv
    # back to the unscaled basis for the sweep in this model
    r = rt * (1 / g)[:, None] * g[None, :]
    t = tt_ * (1 / g)[:, None] * g[None, :]
    splus_src = splus_src / g
    sminus_src = sminus_src / g
    return dict(r=r, t=t, sp=splus_src, sm=sminus_src, taup=taup)


def solve_column(dtauc, ssalb, chis, nstr, umu0=1.0, fbeam=0.0, albedo=0.0,
                 fisot=0.0, planck=False, temper=None, btemp=0.0, ttemp=0.0, temis=0.0,
                 wvnmlo=0.0, wvnmhi=0.0, zd=None, radius=None):
    """Layers top->bottom; returns (flup, fdn) at nlyr+1 levels top->bottom.  zd (bottom ->
    top) and radius: the pseudo-spherical beam, its slant depths and secants evaluated in
    double as the prologue kernel does (tests/spher_ref.py layer_secants)."""
    nn = nstr // 2
    mu, w = double_gauss(nn)
    nlyr = len(dtauc)
    beam = fbeam > 0 and umu0 > 0
    pk = [plkavg(wvnmlo, wvnmhi, tt) for tt in temper] if planck else [0.0] * (nlyr + 1)
    ops = []
    tauc = 0.0
    chp = lamv = None
    if zd is not None and beam:
        from spher_ref import layer_secants
        tp = []
        for lc in range(nlyr):
            s_ = ssalb[lc] if ssalb[lc] != 1.0 else 1.0 - DITHER
            f_ = chis[lc][nstr - 1] if len(chis[lc]) >= nstr else 0.0
            tp.append((1.0 - s_ * f_) * dtauc[lc])
        chp, lamv = layer_secants(zd, radius, umu0, np.array(tp))

    def direct(lev, tt):  # the direct beam's flux at a level
        if not beam:
            return 0.0
        return umu0 * fbeam * (math.exp(-tt / umu0) if chp is None else math.exp(-chp[lev]))
    for lc in range(nlyr):
        o = layer_ops(dtauc[lc], ssalb[lc], chis[lc], nstr, umu0, fbeam if beam else 0.0,
                      pk[lc], pk[lc + 1], tauc, None if chp is None else lamv[lc],
                      None if chp is None else (chp[lc], chp[lc + 1]))
        o["tauc_top"] = tauc
        tauc += o["taup"]
        ops.append(o)
    c = 2 * math.pi * w * mu
    ra = np.zeros((nn, nn))
    sd = np.full(nn, fisot + (temis * plkavg(wvnmlo, wvnmhi, ttemp) if planck else 0.0))
    store = []
    for o in ops:
        w1 = np.eye(nn) - o["r"] @ ra
        zt = np.linalg.solve(w1, o["t"])
        t_ = np.linalg.solve(w1, o["r"] @ sd + o["sp"])
        store.append((zt, t_, ra.T @ c, c @ sd))
        u = ra @ t_ + sd
        p = ra @ zt
        ra = o["r"] + o["t"] @ p
        sd = o["t"] @ u + o["sm"]
    e_surf = 0.0
    if beam:
        e_surf += albedo * direct(nlyr, tauc) / math.pi
    if planck:
        e_surf += (1 - albedo) * plkavg(wvnmlo, wvnmhi, btemp)
    wm = w * mu
    xs = (2 * albedo * wm @ sd + e_surf) / (1 - 2 * albedo * wm @ (ra @ np.ones(nn)))
    ip = np.full(nn, xs)
    flup = np.zeros(nlyr + 1)
    fdn = np.zeros(nlyr + 1)
    flup[nlyr] = c @ ip
    fdn[nlyr] = c @ (ra @ ip + sd) + direct(nlyr, tauc)
    for lc in range(nlyr - 1, -1, -1):
        zt, t_, rc, cs = store[lc]
        ip = zt @ ip + t_
        flup[lc] = c @ ip
        fdn[lc] = rc @ ip + cs + direct(lc, ops[lc]["tauc_top"])
    return flup, fdn
