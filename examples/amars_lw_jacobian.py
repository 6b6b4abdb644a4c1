"""Jacobians of an amars LW band radiance with respect to the atmosphere, from one backward.

    python examples/amars_lw_jacobian.py [--nstr 8] [--ngpoint 16] [--nlyr 40] [--table FILE.nc]

The amars LW chain of examples/amars_lw.py with the Beer-Lambert solver in place of DISORT
(pure absorption: omega = 0 in this case), every link differentiable:

    state (conc, temp, pres)
      -> RFM CO2 + RFM H2O          pyharp_amd.opacity.RFM        (hd_rfm_attenuate_bwd)
      -> prop = prop1 + prop2       torch
      -> temf = layer2level(temp)   torch
      -> band radiance at the top   BeerLambert.forward_rays_band (hd_beer_rays_bwd), planck

``radiance.backward()`` then leaves d(band radiance)/d(conc) and d/d(temp) per layer in
``conc.grad`` and ``temp.grad``; the temperature gradient arrives through the Planck source
(temf) and through the absorption's temperature dependence (the RFM anomaly axis) at once.

With ``--table`` the RFM tables and the ck weights come from an RFM ck file in netCDF
(amarsw-ck-B1.nc, as examples/amars_lw.py); without it from a synthetic table of the same
layout (the real file is git-ignored upstream).
"""

from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pyharp_amd import BeerLambert, BeerLambertOptions, layer2level  # noqa: E402
from pyharp_amd.opacity import RFM, AttenuatorOptions, read_weights_rfm  # noqa: E402


def synthetic_modules(ngpoint, seed=20250217):
    """CO2 and H2O tables of the RFM layout: ln(m^2/kmol) falling with g-point rank and
    rising gently with pressure and temperature"""
    rng = np.random.default_rng(seed)
    pres = np.logspace(6.2, 1, 20)
    tgrid = np.linspace(-40.0, 40.0, 5)
    tref = np.linspace(320.0, 150.0, 20)
    wave = np.linspace(1.0, 150.0, ngpoint)
    mods = []
    for sp, level in ((0, -9.0), (1, -11.0)):
        k = (level + 6.0 * np.linspace(0, 1, ngpoint)[:, None, None]
             + 0.3 * np.log(pres / 1e5)[None, :, None] + 0.01 * tgrid[None, None, :]
             + rng.uniform(-0.2, 0.2, (ngpoint, 20, 5)))
        mods.append(RFM.from_arrays(wave, pres, tgrid, tref, k, species=sp))
    x, w = np.polynomial.legendre.leggauss(ngpoint)
    return mods, torch.as_tensor(0.5 * w)


def run(nstr=8, ngpoint=16, nlyr=40, ncol=1, table=None, device=0):
    dev = torch.device("cuda", device)
    if table:
        op = AttenuatorOptions().species_names(["CO2", "H2O"]).species_weights([44.0e-3, 18.0e-3])
        mods = [RFM(op.copy().species_ids([i]).opacity_files([table])) for i in (0, 1)]
        weights = read_weights_rfm(table)
    else:
        mods, weights = synthetic_modules(ngpoint)
    nwave = mods[0].kshape[0]
    # the state: a 6 mbar CO2 atmosphere with a little water, 1 km layers, layer 0 = bottom
    pres = torch.logspace(np.log10(600.0), 0.0, nlyr, dtype=torch.float64, device=dev) \
        .expand(ncol, nlyr).contiguous()
    temp = torch.linspace(220.0, 150.0, nlyr, dtype=torch.float64, device=dev) \
        .expand(ncol, nlyr).contiguous()
    ntot = pres / (8.314472 * temp) * 1.0e3  # mol/m^3 x 1 km layers: column amounts per layer
    conc = torch.stack([0.95 * ntot, 3.0e-4 * ntot], dim=-1)
    conc, temp, pres = (x.requires_grad_() for x in (conc, temp, pres))
    kwargs = {"pres": pres, "temp": temp}
    prop = mods[0].forward(conc, kwargs) + mods[1].forward(conc, kwargs)
    temf = layer2level(temp)
    bop = BeerLambertOptions().nstr(nstr).nlyr(nlyr).nwave(nwave).ncol(ncol).planck(True)
    bop.wave_lower([1.0] * nwave).wave_upper([150.0] * nwave).device(device)
    bc = {"albedo": torch.zeros((nwave, ncol), dtype=torch.float64, device=dev),
          "btemp": torch.full((nwave, ncol), 220.0, dtype=torch.float64, device=dev)}
    umu = torch.tensor([1.0], dtype=torch.float64, device=dev)  # the nadir radiance at the top
    rad = BeerLambert(bop).forward_rays_band(prop, bc, temf, umu=umu, weights=weights.to(dev))
    rad.sum().backward()
    return {"rad": rad.detach(), "prop": prop.detach(), "dconc": conc.grad, "dtemp": temp.grad,
            "dpres": pres.grad}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nstr", type=int, default=8)
    ap.add_argument("--ngpoint", type=int, default=16)
    ap.add_argument("--nlyr", type=int, default=40)
    ap.add_argument("--table", default=None)
    a = ap.parse_args()
    r = run(a.nstr, a.ngpoint, a.nlyr, table=a.table)
    print("band radiance =", r["rad"].cpu().numpy().ravel())
    print("layer (0 = bottom)  dI/dCO2        dI/dH2O        dI/dT          dI/dp")
    dc, dt, dp = (r[k][0].cpu().numpy() for k in ("dconc", "dtemp", "dpres"))
    for k in range(a.nlyr):
        print(f"{k:5d}            {dc[k, 0]: .6e} {dc[k, 1]: .6e} {dt[k]: .6e} {dp[k]: .6e}")


if __name__ == "__main__":
    main()
