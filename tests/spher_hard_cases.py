"""The hard-regime cases of the pseudo-spherical flux path (tests/test_gpu_spher_hard.py),
judged against ``oracle/disort_mp.py`` with ``zd`` / ``radius`` at 50 digits.

The families of tests/hard_cases.py restated with a slant beam, and two of their own:

* ``resonance``: a layer's beam secant lambda on one of its eigenvalues, lambda = +-k_j (1 +
  delta).  lambda differs in every layer of a pseudo-spherical solve, and under a thicker
  layer it is negative.  ``scat`` / ``abs``: the middle layer of the flux family's column,
  mu0 tuned; ``top``: the top layer, whose lambda = g(j, j) is pure geometry; ``negative``:
  the bottom layer of a two-layer column at lambda = -k_j (1 + delta), its depth tuned.
* ``low_sun``: mu0 down to 1e-6 over shells from 1 mm to 2 R thick and over layers of tau'
  1e-9 and 1e-12 under a thick one (lambda about -1e8 and -5e12).
* ``depth``, ``conservative``, ``thin_thermal``, ``phase``: the flux family's columns with
  the slant beam; ``depth`` adds layers of tau = 0 exactly at the top, in the middle and
  at the bottom and a column of no optical depth at all.

Every batch is one Disort configuration with at most 5 layers and 24 columns; ``zd`` is
shared by the columns (L+1,) or per column (C, L+1), both in every family.  Inputs and the
mp record are stored in tests/golden/spher_hard.npz by tests/golden/
make_spher_hard_golden.py; tests/test_mp_oracle.py recomputes a sample.

Everything is written top -> bottom and flipped to harp's layout by ``hard_cases._batch``;
``zd`` is bottom -> top, as in the library.
"""

import functools

import numpy as np

import spher_ref
from hard_cases import (CONS_G, DELTAS, DEPTH_STACKS, NSTR, ONE_MINUS_SSA, THIN_TAU, WAVE,
                        _batch, _phase, bc_keys, dfdt_scale, hg, key, resonance_k)
from oracle import disort_mp
from oracle.disort_np import DITHER

FAMILIES = ("resonance", "low_sun", "depth", "conservative", "thin_thermal", "phase")
RADIUS = 3.39e6                                   # a Mars-sized body, metres
ZD3 = np.array([0.0, 10.0e3, 25.0e3, 45.0e3])     # the three-layer columns
ZD2 = np.array([0.0, 20.0e3, 40.0e3])
TOP_DELTAS = (0.0, 1e-13, -1e-13, 1e-10, -1e-10, 4e-10, -4e-10, 1e-8, -1e-8)
NEG_DELTAS = (0.0, 1e-10, -1e-10, 4e-10, -4e-10, 1e-8, -1e-8, 1e-6, -1e-6)
LOW_MU0 = (0.5, 0.1, 0.02, 1e-3, 1e-6)
DELTA_TOL = 1e-12  # realised delta (50 digits, from the stored doubles) against the asked


def _spher(b, cols, shared=None):
    """Attach the geometry: ``shared`` (L+1,), or every column's own ``zd``."""
    if shared is not None:
        b["zd"] = np.asarray(shared, np.float64).copy()
    else:
        b["zd"] = np.array([np.asarray(c["zd"], np.float64) for c in cols])
    assert b["zd"].shape[-1] == b["nlyr"] + 1 and np.all(np.diff(b["zd"], axis=-1) > 0.0)
    b["radius"] = RADIUS
    return b


def scaled_depths(tau, ssa, chi, nstr):
    """dtau' of delta-M in double, as every double solver here forms it."""
    out = []
    for t, s, c in zip(tau, ssa, chi):
        s = 1.0 - DITHER if s == 1.0 else s
        f = c[nstr - 1] if len(c) >= nstr else 0.0
        out.append((1.0 - s * f) * t)
    return np.array(out)


def _bisect(fn, lo, hi, target):
    """x in [lo, hi] with fn(x) = target to the last double; fn increasing."""
    assert fn(lo) < target < fn(hi), (fn(lo), target, fn(hi))
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if fn(mid) < target:
            lo = mid
        else:
            hi = mid
    return lo if abs(fn(lo) - target) <= abs(fn(hi) - target) else hi


def _target(k, delta):
    with disort_mp.mp.workdps(50):
        return float(k * (1 + disort_mp.mpf(delta)))


def _tune_mu0(zd, tp, layer, target):
    """mu0 at which solver layer ``layer``'s secant is ``target`` (it falls as mu0 rises)."""
    return _bisect(lambda u: -spher_ref.layer_secants(zd, RADIUS, u, tp)[1][layer], 0.02, 1.0,
                   -target)


@functools.lru_cache(maxsize=None)
def _resonance(nstr):
    out = []
    for scattering in (True, False):  # the flux family's column, the middle layer's secant
        ssa, k = resonance_k(nstr, scattering)
        tau, ss = [0.4, 1.0, 0.8], [0.6, ssa, 0.6]
        chi = [hg(0.5, nstr), hg(0.7, nstr), hg(0.5, nstr)]
        tp = scaled_depths(tau, ss, chi, nstr)
        cols = [dict(tau=tau, ssa=ss, chi=chi, fbeam=1.0, albedo=0.3, delta=d, layer=1, sign=1,
                     umu0=_tune_mu0(ZD3, tp, 1, _target(k, d))) for d in DELTAS]
        out.append(_res_batch("scat" if scattering else "abs", nstr, cols, shared=ZD3))
    # the top layer: lambda = g(j, j), every column on altitudes of its own
    ssa, k = resonance_k(nstr, True)
    tau, ss = [1.0, 0.4, 0.8], [ssa, 0.6, 0.6]
    chi = [hg(0.7, nstr), hg(0.5, nstr), hg(0.5, nstr)]
    tp = scaled_depths(tau, ss, chi, nstr)
    cols = []
    for i, d in enumerate(TOP_DELTAS):
        zd = ZD3 * (1.0 + 0.02 * i)
        cols.append(dict(tau=tau, ssa=ss, chi=chi, fbeam=1.0, albedo=0.3, delta=d, layer=0,
                         sign=1, zd=zd, umu0=_tune_mu0(zd, tp, 0, _target(k, d))))
    out.append(_res_batch("top", nstr, cols))
    # under a thicker layer: lambda_bottom = -k (1 + delta), by the bottom layer's depth
    ss, chi = [0.6, ssa], [hg(0.5, nstr), hg(0.7, nstr)]
    cols = []
    for d in NEG_DELTAS:
        def lam(x):
            return spher_ref.layer_secants(ZD2, RADIUS, 0.3,
                                           scaled_depths([1.0, x], ss, chi, nstr))[1][1]
        x = _bisect(lam, 1e-6, 10.0, -_target(k, d))
        cols.append(dict(tau=[1.0, x], ssa=ss, chi=chi, fbeam=1.0, albedo=0.3, umu0=0.3,
                         delta=d, layer=1, sign=-1))
    out.append(_res_batch("negative", nstr, cols, shared=ZD2))
    return out


def _res_batch(name, nstr, cols, shared=None):
    b = _spher(_batch(name, nstr, nstr, cols), cols, shared)
    b["delta"] = np.array([c["delta"] for c in cols])
    b["res_layer"], b["res_sign"] = cols[0]["layer"], cols[0]["sign"]
    return b


def _realised_delta(b, r):
    """sign lambda / k_j - 1 of the column's resonant layer at 50 digits, from a
    ``return_mp`` solve of its stored doubles (k_j: the eigenvalue nearest |lambda|)."""
    with disort_mp.mp.workdps(50):
        lam = b["res_sign"] * r["lam"][b["res_layer"]]
        k = min(r["kk"][b["res_layer"]], key=lambda v: abs(v - lam))
        return float(lam / k - 1)


def _planck_kw(nlyr, btemp=285.0):
    return dict(temper=list(np.linspace(200.0, 280.0, nlyr + 1)), btemp=btemp, ttemp=150.0,
                temis=0.5)


def _low_sun(nstr):
    out = []
    zd5 = spher_ref.ZD
    for planck in (False, True):
        tag = "_planck" if planck else ""

        def col(tau, u, **kw):
            n = len(tau)
            c = dict(tau=list(tau), ssa=[0.9] * n, chi=[hg(0.7, nstr)] * n, fbeam=1.0, umu0=u,
                     albedo=0.3, **kw)
            if planck:
                c.update(_planck_kw(n))
            return c

        thin_bottom = spher_ref.TAU_PROFILES["thin_bottom"][::-1]
        cols = [col([0.3] * 5, u) for u in LOW_MU0] + [col(thin_bottom, u) for u in LOW_MU0]
        out.append(_spher(_batch("layers20km" + tag, nstr, nstr, cols, planck), cols, zd5))
        cols = []
        for zd in (1.0 * np.arange(6.0), 1.0e-3 * np.arange(6.0),
                   np.array([0.0, 1e4, 1e5, 1e6, 3e6, 6.78e6])):
            cols += [col([0.3] * 5, u, zd=zd) for u in LOW_MU0]
        out.append(_spher(_batch("shells" + tag, nstr, nstr, cols, planck), cols))
        cols = [col([3.0, 1e-9, 1e-12, 0.5], u) for u in LOW_MU0]
        out.append(_spher(_batch("thin_under_thick" + tag, nstr, nstr, cols, planck), cols,
                          2.0e4 * np.arange(5.0)))
    return out


ZERO_STACKS = ((0.0, 1.0, 0.5, 2.0), (1.0, 0.5, 0.0, 2.0), (1.0, 0.5, 2.0, 0.0),
               (0.0, 0.0, 0.0, 0.0))


def _depth(nstr):
    out = []
    zd = 2.0e4 * np.arange(5.0)
    for planck in (False, True):
        cols = []
        for stack in DEPTH_STACKS:
            for umu0 in (0.05, 0.6):
                for albedo in (0.0, 1.0):
                    cols.append(dict(tau=list(stack), umu0=umu0, albedo=albedo))
        for i, stack in enumerate(ZERO_STACKS):
            cols.append(dict(tau=list(stack), umu0=(0.05, 0.6)[i % 2], albedo=0.5))
        for i, c in enumerate(cols):
            c.update(ssa=[0.9, 0.9, 0.5, 0.9], chi=[hg(0.7, nstr)] * 4, fbeam=1.0,
                     zd=zd * (1.0 + 0.03 * i))
            if planck:  # isothermal: the family isolates the depths
                c.update(temper=[250.0] * 5, btemp=250.0, ttemp=0.0, temis=0.0)
        b = _batch("beam_planck" if planck else "beam", nstr, nstr, cols, planck)
        out.append(_spher(b, cols, None if planck else zd))
    return out


def _conservative(nstr):
    out = []
    for planck in (False, True):
        cols = []
        for x in ONE_MINUS_SSA:
            for g in CONS_G:
                col = dict(tau=[0.5, 2.0, 1.0], ssa=[1.0 - x] * 3, chi=[hg(g, nstr)] * 3,
                           fbeam=1.0, umu0=0.1, albedo=0.2)
                if planck:
                    col.update(temper=[200.0, 220.0, 245.0, 260.0], btemp=265.0, ttemp=150.0,
                               temis=0.5)
                cols.append(col)
        if not planck:  # a cavity that loses energy only through 1 - ssa and the top
            cols.append(dict(tau=[0.5, 2.0, 1.0], ssa=[1.0 - 1e-6] * 3, chi=[hg(0.85, nstr)] * 3,
                             fbeam=1.0, umu0=0.1, albedo=1.0))
        for i, c in enumerate(cols):
            c["zd"] = ZD3 * (1.0 + 0.01 * i)
        b = _batch("beam_planck" if planck else "beam", nstr, nstr, cols, planck)
        out.append(_spher(b, cols, None if planck else ZD3))
    return out


def _thin_thermal(nstr):
    top, mid = [], []
    for i, t in enumerate(THIN_TAU):
        for ssa in (0.0, 0.5):
            top.append(dict(tau=[t, 1.0], ssa=[ssa, 0.5], chi=[hg(0.7, nstr)] * 2,
                            temper=[200.0, 210.0, 230.0], btemp=230.0, albedo=0.1, fbeam=1.0,
                            umu0=0.1))
            mid.append(dict(tau=[0.5, t, 1.0], ssa=[0.3, ssa, 0.5], chi=[hg(0.7, nstr)] * 3,
                            temper=[200.0, 215.0, 225.0, 240.0], btemp=240.0, albedo=0.1,
                            fbeam=1.0, umu0=0.1, zd=ZD3 * (1.0 + 0.05 * i)))
    return [_spher(_batch("top2", nstr, nstr, top, True), top, ZD2),
            _spher(_batch("mid3", nstr, nstr, mid, True), mid)]


def _phase_spher(nstr):
    """hard_cases' ``full`` batch and nmom 0, nstr - 1, nstr + 4, every column at mu0 = 0.1:
    delta-M (nmom >= nstr) separates ch' from ch, and rfldn is their difference."""
    out = []
    keep = {"full"} | {f"nmom{n}" for n in (0, nstr - 1, nstr + 4)}
    for b in _phase(nstr):
        if b["name"] not in keep:
            continue
        b["bc"]["umu0"][:] = 0.1
        ncol = b["prop"].shape[1]
        cols = [dict(zd=ZD3 * (1.0 + 0.04 * c)) for c in range(ncol)]
        out.append(_spher(b, cols, ZD3 if b["name"] == "full" else None))
    return out


_BUILD = dict(resonance=_resonance, low_sun=_low_sun, depth=_depth, conservative=_conservative,
              thin_thermal=_thin_thermal, phase=_phase_spher)


def batches(family, nstr):
    return _BUILD[family](nstr)


def column_zd(b, c):
    return b["zd"][c] if b["zd"].ndim == 2 else b["zd"]


def column_kwargs(b, c):
    """Column c of a batch in cdisort's order (top -> bottom): positional and keyword
    arguments of ``disort_mp.disort_column`` / ``spher_ref.spher_column``."""
    p = b["prop"][0, c, ::-1]
    pm = np.concatenate([np.ones((b["nlyr"], 1)), p[:, 2:2 + b["nmom"]]], axis=1)
    kw = {k: float(v[0, c]) for k, v in b["bc"].items()}
    if b["planck"]:
        kw.update(planck=True, temper=b["temf"][c, ::-1], wvnmlo=WAVE[0], wvnmhi=WAVE[1])
    kw.update(zd=column_zd(b, c), radius=b["radius"])
    return (p[:, 0], p[:, 1], pm, b["nstr"]), kw


def double_geometry(b, c):
    """(chp, lam, ch) of column c as evaluated in double (spher_ref), solver order."""
    (tau, ssa, pm, nstr), kw = column_kwargs(b, c)
    tp = scaled_depths(tau, ssa, [list(r[1:]) for r in pm], nstr)
    chp, lam = spher_ref.layer_secants(kw["zd"], kw["radius"], kw["umu0"], tp)
    ch = spher_ref.chapman(kw["zd"], kw["radius"], kw["umu0"], tau[::-1])[::-1]
    return chp, lam, ch


def reference(b, cols=None, dps=50, admission=False):
    """The mp record of a batch (or of its columns ``cols``): (flx (1, C, L+1, 8), scale
    (1, C, L+1)).  With ``admission`` (the generator's checks) two more: the record of the
    same solve fed the double-evaluated slant depths and secants, and the realised delta of
    every column (zeros outside the resonance family)."""
    cols = range(b["prop"].shape[1]) if cols is None else list(cols)
    flx = np.zeros((1, len(cols), b["nlyr"] + 1, 8))
    scale = np.zeros((1, len(cols), b["nlyr"] + 1))
    alt, delta = np.zeros_like(flx), np.zeros(len(cols))
    for i, c in enumerate(cols):
        args, kw = column_kwargs(b, c)
        if admission:
            kw.update(geom=double_geometry(b, c), return_mp=True)
        r = disort_mp.disort_column(*args, dps=dps, **kw)
        flx[0, i], scale[0, i] = r["flx"][::-1], r["scale"][::-1]
        if admission:
            alt[0, i] = r["flx_geom"][::-1]
            if "delta" in b:
                delta[i] = _realised_delta(b, r)
    return (flx, scale, alt, delta) if admission else (flx, scale)


def load(golden_dir):
    """{(family, nstr): [batch dicts with 'ref', 'scale', 'zd', 'radius' (and 'delta' in
    the resonance family)]} from spher_hard.npz."""
    import os
    z = np.load(os.path.join(golden_dir, "spher_hard.npz"))
    tree = {}
    for k in z.files:
        fam, n, name, field = k.split("/")
        tree.setdefault((fam, int(n[1:])), {}).setdefault(name, {})[field] = z[k]
    out = {}
    for fk, bs in tree.items():
        lst = []
        for name, d in bs.items():
            b = dict(name=name, nstr=fk[1], nlyr=d["prop"].shape[2],
                     nmom=d["prop"].shape[3] - 2, planck="temf" in d, prop=d["prop"],
                     temf=d.get("temf"), ref=d["ref"], zd=d["zd"], radius=float(d["radius"]))
            b["bc"] = dict(zip(bc_keys(b), d["bc"]))
            b["scale"] = dfdt_scale(b, b["ref"])
            if "delta" in d:
                b["delta"], b["delta_realised"] = d["delta"], d["delta_realised"]
                b["res_layer"], b["res_sign"] = (0 if name == "top" else 1), \
                    (-1 if name == "negative" else 1)
            lst.append(b)
        out[fk] = lst
    return out


__all__ = ["FAMILIES", "NSTR", "RADIUS", "batches", "key", "reference", "load", "column_kwargs",
           "double_geometry"]
