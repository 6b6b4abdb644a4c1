"""The hard-regime flux cases of tests/test_gpu_hard.py: inputs the random generators of
the other parity tests never produce, judged against the arbitrary-precision solver
``oracle/disort_mp.py`` (the two double oracles lose the project's 1e-6 on part of them;
DESIGN.md section 4).

Five families, each a list of batches (one Disort configuration each: nlyr, nmom,
planck), for nstr in ``NSTR``.  Inputs and the mp record are stored in
tests/golden/flux_hard.npz by tests/golden/make_hard_golden.py; tests/test_mp_oracle.py
recomputes a sample, so a stale file fails.

Everything here is written top -> bottom (cdisort's order) and flipped to harp's layout
(layer / level 0 = bottom) at the end of ``_batch``.
"""

import numpy as np

from oracle import disort_mp

NSTR = (2, 4, 8, 16, 18, 32)
FAMILIES = ("phase", "conservative", "depth", "thin_thermal", "resonance")
WAVE = (500.0, 800.0)  # cm^-1, the one band of every Planck batch

DELTAS = (0.0,) + tuple(s * d for d in (1e-13, 1e-11, 1e-10, 4e-10, 6e-10, 1e-8, 1e-6, 1e-4,
                                         2e-4, 1e-3) for s in (1.0, -1.0))
ONE_MINUS_SSA = (1e-4, 1e-6, 1e-8, 1e-10, 1e-12, 0.0)
CONS_G = (0.0, 0.85, 0.97)
THIN_TAU = (1e-3, 1e-6, 1e-9, 1e-12, 1e-15)
DEPTH_STACKS = ((1e-12, 1e4, 0.0, 1e2), (1e-8, 1e-3, 30.0, 1e3))


# ---- phase functions: chi_1 .. chi_n ----
def hg(g, n):
    return [g ** l for l in range(1, n + 1)]


def rayleigh(n):
    return [0.0, 0.1] + [0.0] * (n - 2) if n >= 2 else [0.0] * n


def double_hg(n):
    return [0.7 * 0.8 ** l + 0.3 * (-0.6) ** l for l in range(1, n + 1)]


def _batch(name, nstr, nmom, cols, planck=False):
    """cols: list of dicts with tau, ssa (nlyr,), chi (nlyr lists of >= nmom moments), and
    the boundary values; temper (nlyr+1,) with planck.  All top -> bottom."""
    ncol = len(cols)
    nlyr = len(cols[0]["tau"])
    prop = np.zeros((1, ncol, nlyr, 2 + nmom))
    bc = {k: np.zeros((1, ncol)) for k in ("fbeam", "umu0", "albedo")}
    if planck:
        bc.update({k: np.zeros((1, ncol)) for k in ("btemp", "ttemp", "temis")})
    bc["umu0"][:] = 1.0
    temf = np.zeros((ncol, nlyr + 1)) if planck else None
    for c, col in enumerate(cols):
        for lc in range(nlyr):
            k = nlyr - 1 - lc  # harp: layer 0 = bottom
            prop[0, c, k, 0] = col["tau"][lc]
            prop[0, c, k, 1] = col["ssa"][lc]
            prop[0, c, k, 2:] = col["chi"][lc][:nmom]
        for key in bc:
            if key in col:
                bc[key][0, c] = col[key]
        if planck:
            temf[c] = np.asarray(col["temper"], np.float64)[::-1]
    return dict(name=name, nstr=nstr, nlyr=nlyr, nmom=nmom, planck=planck, prop=prop, bc=bc,
                temf=temf)


def _phase(nstr):
    out = []
    tau, ssa = [0.3, 1.0, 2.0], [0.9, 0.99, 0.7]

    def cols(n, kinds):
        table = {"hg-0.8": hg(-0.8, n), "hg-0.5": hg(-0.5, n), "hg-0.2": hg(-0.2, n),
                 "rayleigh": rayleigh(n), "dhg": double_hg(n), "hg0.8": hg(0.8, n)}
        res = []
        for i, kind in enumerate(kinds):
            chi = [table["hg-0.5"], table["rayleigh"], table["dhg"]] if kind == "mixed" \
                else [table[kind]] * 3
            res.append(dict(tau=tau, ssa=ssa, chi=chi, fbeam=1.0 + 0.1 * i,
                            umu0=(0.6, 0.25, 0.9)[i % 3], albedo=(0.0, 0.3, 0.8)[i % 3]))
        return res

    out.append(_batch("full", nstr, nstr, cols(nstr, ["hg-0.8", "hg-0.5", "hg-0.2", "rayleigh",
                                                      "dhg", "mixed"])))
    for nmom in sorted({0, 1, nstr // 2, nstr - 1, nstr + 4}):
        out.append(_batch(f"nmom{nmom}", nstr, nmom,
                          cols(max(nmom, 1), ["hg-0.5", "dhg", "mixed", "hg0.8"])))
    return out


def _conservative(nstr):
    out = []
    for planck in (False, True):
        cols = []
        for x in ONE_MINUS_SSA:
            for g in CONS_G:
                col = dict(tau=[0.5, 2.0, 1.0], ssa=[1.0 - x] * 3, chi=[hg(g, nstr)] * 3,
                           fbeam=1.0, umu0=0.6, albedo=0.2)
                if planck:
                    col.update(temper=[200.0, 220.0, 245.0, 260.0], btemp=265.0, ttemp=150.0,
                               temis=0.5)
                cols.append(col)
        if not planck:  # a cavity that loses energy only through 1 - ssa and the top
            cols.append(dict(tau=[0.5, 2.0, 1.0], ssa=[1.0 - 1e-6] * 3, chi=[hg(0.85, nstr)] * 3,
                             fbeam=1.0, umu0=0.6, albedo=1.0))
        out.append(_batch("beam_planck" if planck else "beam", nstr, nstr, cols, planck))
    return out


def _depth(nstr):
    out = []
    for planck in (False, True):
        cols = []
        for stack in DEPTH_STACKS:
            for umu0 in (0.05, 0.6):
                for albedo in (0.0, 1.0):
                    col = dict(tau=list(stack), ssa=[0.9, 0.9, 0.5, 0.9],
                               chi=[hg(0.7, nstr)] * 4, fbeam=1.0, umu0=umu0, albedo=albedo)
                    if planck:  # isothermal: the family isolates the depths
                        col.update(temper=[250.0] * 5, btemp=250.0, ttemp=0.0, temis=0.0)
                    cols.append(col)
        out.append(_batch("beam_planck" if planck else "beam", nstr, nstr, cols, planck))
    return out


def _thin_thermal(nstr):
    top, mid = [], []
    for t in THIN_TAU:
        for ssa in (0.0, 0.5):
            top.append(dict(tau=[t, 1.0], ssa=[ssa, 0.5], chi=[hg(0.7, nstr)] * 2,
                            temper=[200.0, 210.0, 230.0], btemp=230.0, albedo=0.1))
            mid.append(dict(tau=[0.5, t, 1.0], ssa=[0.3, ssa, 0.5], chi=[hg(0.7, nstr)] * 3,
                            temper=[200.0, 215.0, 225.0, 240.0], btemp=240.0, albedo=0.1))
    return [_batch("top2", nstr, nstr, top, True), _batch("mid3", nstr, nstr, mid, True)]


def resonance_k(nstr, scattering):
    """(ssa of the middle layer, the eigenvalue k_j (mpf) the beam is laid on): the
    smallest k > 1.01 of the layer, so that umu0 = (1 + delta) / k < 1."""
    for ssa in ((0.9, 0.7, 0.5, 0.3) if scattering else (0.0,)):
        ks = [k for k in disort_mp.layer_eigenvalues(ssa, [1.0] + hg(0.7, nstr), nstr)
              if k > 1.01]
        if ks:
            return ssa, ks[0]
    raise ValueError("no eigenvalue above 1")


def _resonance(nstr):
    out = []
    for scattering in (True, False):
        ssa, k = resonance_k(nstr, scattering)
        with disort_mp.mp.workdps(50):  # umu0 is the double nearest to (1 + delta) / k
            umu0 = [float((1 + disort_mp.mpf(d)) / k) for d in DELTAS]
        cols = [dict(tau=[0.4, 1.0, 0.8], ssa=[0.6, ssa, 0.6],
                     chi=[hg(0.5, nstr), hg(0.7, nstr), hg(0.5, nstr)], fbeam=1.0,
                     umu0=u, albedo=0.3) for u in umu0]
        out.append(_batch("scat" if scattering else "abs", nstr, nstr, cols))
    return out


_BUILD = dict(phase=_phase, conservative=_conservative, depth=_depth,
              thin_thermal=_thin_thermal, resonance=_resonance)


def batches(family, nstr):
    return _BUILD[family](nstr)


def key(family, nstr, name):
    return f"{family}/n{nstr}/{name}"


def reference(b, cols=None, dps=50):
    """The mp record of a batch (or of its columns ``cols``): (flx (1, C, L+1, 8),
    scale (1, C, L+1))."""
    sel = slice(None) if cols is None else list(cols)
    bc = {k: v[:, sel] for k, v in b["bc"].items()}
    temf = None if b["temf"] is None else b["temf"][sel]
    return disort_mp.flx_forward(b["prop"][:, sel], bc, temf, nstr=b["nstr"], nmom=b["nmom"],
                                 planck=b["planck"], wave_lower=[WAVE[0]], wave_upper=[WAVE[1]],
                                 dps=dps)


def bc_keys(b):
    return ("fbeam", "umu0", "albedo") + (("btemp", "ttemp", "temis") if b["planck"] else ())


def dfdt_scale(b, ref):
    """(1 - ssa_in) 4 pi max(uavg, B_lev) per level (the magnitude dfdt is a difference
    of, tests/flx_ref.py), from a batch's inputs and its record; harp layout, where the
    layer directly above level j is layer j and the top level takes the top layer."""
    import math
    from oracle.disort_np import plkavg
    ssa = b["prop"][..., 1]
    ssa_in = np.concatenate([ssa, ssa[..., -1:]], axis=-1)
    blev = np.zeros(ref.shape[:3])
    if b["planck"]:
        blev[0] = [[plkavg(WAVE[0], WAVE[1], t) for t in row] for row in b["temf"]]
    return (1.0 - ssa_in) * 4.0 * math.pi * np.maximum(ref[..., 4], blev)


def load(golden_dir):
    """{(family, nstr): [batch dicts with 'ref' and 'scale']} from flux_hard.npz."""
    import os
    z = np.load(os.path.join(golden_dir, "flux_hard.npz"))
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
                     temf=d.get("temf"), ref=d["ref"])
            b["bc"] = dict(zip(bc_keys(b), d["bc"]))
            b["scale"] = dfdt_scale(b, b["ref"])
            lst.append(b)
        out[fk] = lst
    return out
