"""Throughput of the ray radiances (hd_solve_rays) beside the grid call, in one process.

    python scripts/bench_rays.py [--ncol 1000] [--ngpoint 16] [--nstr 16] [--nlyr 80]
                                 [--steps 5] [--warmup 2] [--out FILE] [--spher [--rounds 5]]

Workload: scripts/bench_rad.py's (the C4 column statistics with a beam, TOA) with its
8 x 4 directions taken as 32 (cosine, azimuth) pairs, jittered per column (every
column its own emission angles and azimuths).  One JSON line per leg:

  grid_8x4            the grid call of bench_rad.py (8 user-angle integrations per
                      unit): context only -- the ray legs do 32
  grid_32x32          the grid call that covers 32 arbitrary directions (column 0's 32
                      cosines x its 32 azimuths, shared by every column): what a
                      caller without rays pays
  rays_shared         forward_rays, column 0's 32 pairs shared by every column
  rays_per_column     forward_rays, each column its own 32 pairs
  rays_band           forward_rays_band, per-column pairs, band sum fused, no rad stored

--spher adds one more line, rays_spher_vs_plain: forward_rays(zd=) (the pseudo-spherical
beam, hd_solve_rays_spher; a Mars-sized radius, levels evenly up to 100 km) beside the plain
per-column call on the same inputs in the same run, `rounds` alternated rounds of `steps`
calls each, the median time of each side and their ratio (nstr <= 16).

Times are a host clock around `steps` calls that end in a device synchronise, after
`warmup` calls of the same leg.  The per-column leg is checked on a subsample against
the radiance oracle (the checker only).  `--out` appends the lines to a file.
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=1000)
    ap.add_argument("--ngpoint", type=int, default=16)
    ap.add_argument("--nstr", type=int, default=16)
    ap.add_argument("--nlyr", type=int, default=80)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="grid_8x4,grid_32x32,rays_shared,rays_per_column,rays_band")
    ap.add_argument("--out", default=None)
    ap.add_argument("--spher", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    from pyharp_amd import Disort, DisortOptions
    if not torch.cuda.is_available():
        raise SystemExit("bench_rays: no HIP device (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    G, C, L, n = a.ngpoint, a.ncol, a.nlyr, a.nstr
    rng = np.random.default_rng(20250217)  # bench_rad.py's inputs
    prop = np.zeros((G, C, L, 2 + n))
    prop[..., 0] = 10.0 ** rng.uniform(-5, np.log10(5.0), (G, C, L))
    prop[..., 1] = rng.uniform(0.0, 0.99, (G, C, L))
    g = rng.uniform(0.0, 0.85, (G, C, L))
    for l in range(n):
        prop[..., 2 + l] = g ** (l + 1)
    bc = {"fbeam": np.ones((G, C)), "umu0": rng.uniform(0.05, 1.0, (G, C)),
          "phi0": rng.uniform(0, 360, (G, C)), "albedo": rng.uniform(0, 1, (G, C))}
    umu8 = np.concatenate([-np.linspace(1, 0.1, 4), np.linspace(0.1, 1, 4)])
    phi4 = np.linspace(0, 180, 4)
    # the 8 x 4 directions as 32 pairs; per column: cosines jittered by up to 0.03 (kept
    # inside 0.05 <= |mu| <= 1), azimuths by up to 5 degrees
    mu32 = np.repeat(umu8, 4)
    ph32 = np.tile(phi4, 8)
    jr = np.random.default_rng(7)
    mu_col = mu32[None, :] + jr.uniform(-0.03, 0.03, (C, 32))
    mu_col = np.sign(mu32)[None, :] * np.clip(np.abs(mu_col), 0.05, 1.0)
    ph_col = ph32[None, :] + jr.uniform(-5.0, 5.0, (C, 32))
    weights = jr.uniform(0.5, 1.5, G) / G
    utau = [0.0]

    def module(flags, umu=None, phi=None):
        op = DisortOptions().flags(flags).nwave(G).ncol(C).user_tau(utau).radius(3.39e6)
        if umu is not None:
            op.user_mu(list(map(float, umu))).user_phi(list(map(float, phi)))
        op.ds().nlyr, op.ds().nstr, op.ds().nmom = L, n, n
        return Disort(op)

    p = torch.as_tensor(prop, device=dev)
    b = {k: torch.as_tensor(v, device=dev) for k, v in bc.items()}
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev)  # noqa: E731
    rays = module("usrtau,lamber,quiet")
    # 32 x 32: the grid spanned by the cosines and azimuths of column 0's 32 directions;
    # the shared-ray leg takes the same 32
    legs = {
        "grid_8x4": (module("usrtau,usrang,lamber,quiet", umu8, phi4).forward, (p, b), {}),
        "grid_32x32": (module("usrtau,usrang,lamber,quiet", mu_col[0], ph_col[0]).forward,
                       (p, b), {}),
        "rays_shared": (rays.forward_rays, (p, b), dict(umu=t(mu_col[0]), phi=t(ph_col[0]))),
        "rays_per_column": (rays.forward_rays, (p, b), dict(umu=t(mu_col), phi=t(ph_col))),
        "rays_band": (rays.forward_rays_band, (p, b),
                      dict(umu=t(mu_col), phi=t(ph_col), weights=t(weights))),
    }
    lines = []
    for name in a.legs.split(","):
        fn, args, kw = legs[name]
        for _ in range(a.warmup):
            res = fn(*args, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            res = fn(*args, **kw)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.steps
        line = {"leg": name, "metric": "radiance solves/s (all azimuthal modes)",
                "value": G * C / dt, "unit": "solves/s", "ms_per_step": dt * 1e3,
                "config": {"ncol": C, "ngpoint": G, "nstr": n, "nlyr": L, "ntau": 1,
                           "directions": 32 if name != "grid_8x4" else "8x4"}}
        if name == "rays_per_column":
            from oracle.disort_rad_np import disort_rad_forward
            rad = res.cpu().numpy()
            err = 0.0
            for s in rng.choice(G * C, 3, replace=False):
                w, c = divmod(int(s), C)
                sub = {k: v[w:w + 1, c:c + 1] for k, v in bc.items()}
                _, ur = disort_rad_forward(prop[w:w + 1, c:c + 1], sub, nstr=n, umu=mu_col[c],
                                           phi=ph_col[c], utau=utau)
                r = np.arange(32)
                ref = ur[0, 0, r, 0, r]
                err = max(err, np.abs(rad[w, c, 0] - ref).max() / np.abs(ref).max())
            line["max_rel_err_subsample"] = err
        del res
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.spher:
        zd = t(np.linspace(0.0, 1.0e5, L + 1))
        kw = dict(umu=t(mu_col), phi=t(ph_col))
        sides = {"plain": lambda: rays.forward_rays(p, b, **kw),
                 "spher": lambda: rays.forward_rays(p, b, zd=zd, **kw)}
        ms = {k: [] for k in sides}
        for fn in sides.values():
            for _ in range(a.warmup):
                fn()
        for _ in range(a.rounds):  # alternated: plain, spher, plain, spher, ...
            for k, fn in sides.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    fn()
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) / a.steps * 1e3)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        line = {"leg": "rays_spher_vs_plain", "metric": "ms per call, median of alternated rounds",
                "plain_ms": med["plain"], "spher_ms": med["spher"],
                "spher_over_plain_throughput": med["plain"] / med["spher"],
                "plain_ms_rounds": ms["plain"], "spher_ms_rounds": ms["spher"],
                "config": {"ncol": C, "ngpoint": G, "nstr": n, "nlyr": L, "ntau": 1,
                           "directions": 32, "rounds": a.rounds, "steps": a.steps}}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
