"""BeerLambert beside Disort on identical pure-absorption (omega = 0) thermal inputs, in
one process.

    python scripts/bench_beer.py [--shapes c1,c3,batch] [--rounds 7] [--calls 0]
                                 [--warmup 3] [--out-dir profiles/beer]

Shapes: C1 and C3 of bench.py (make_lw_inputs: ncol 1, 16 / 19 990 waves, nstr 8,
nlyr 40, nprop 10) and one batched shape, 10 000 columns x 64 waves x nlyr 80 at
nstr 16 (nprop 18).  Legs per shape, each a Disort call and the BeerLambert call on the
same tensors:

  forward        Disort.forward        / BeerLambert.forward
  forward_band   Disort.forward_band   / BeerLambert.forward_band   (no per-wave fluxes stored)
  forward_rays   Disort.forward_rays   / BeerLambert.forward_rays   (32 upward rays at the
                 top of the atmosphere; the batched shape takes 1 000 of its columns: the
                 Disort radiance path's scratch is sized per solve)

Method: after `warmup` calls of each leg, `rounds` rounds alternate the two solvers
(D B D B ...); a round times `calls` back-to-back calls of one solver with a host clock
around work that ends in a device synchronise (calls = 0: as many as fill about 0.2 s,
from the warm-up's time).  Reported: the median round of each solver, the spread
(min..max), the ratio of the medians.  One JSON line per leg into
<out-dir>/bench_<shape>.jsonl, which also states the bytes the BeerLambert call has to
move -- the tau slot of prop (8 B per layer), the boundary arrays it is given, temf, and
its output -- and the rate that implies at its median time; `beer_tau_line_bytes` counts every
128-byte line that holds a tau instead (what the cache hierarchy fetches when nprop > 1).
The outputs are compared on the spot (max relative difference, TOL 1e-6).  Nothing is
measured without a HIP device.
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

SHAPES = {
    "c1": dict(ncol=1, nwave=16, nstr=8, nlyr=40, tau=(1e-4, 20.0), band=(1.0, 150.0), ck=True),
    "c3": dict(ncol=1, nwave=19990, nstr=8, nlyr=40, tau=(1e-5, 5.0), band=(1.0, 2000.0),
               ck=False),
    "batch": dict(ncol=10000, nwave=64, nstr=16, nlyr=80, tau=(1e-5, 5.0), band=(1.0, 2000.0),
                  ck=False, ray_cols=1000),
}


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        res = fn()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / calls
    return dt, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c1,c3,batch")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "beer"))
    a = ap.parse_args()
    import bench
    from pyharp_amd import BeerLambert, BeerLambertOptions, Disort, DisortOptions
    if not torch.cuda.is_available():
        raise SystemExit("bench_beer: no HIP device (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    os.makedirs(a.out_dir, exist_ok=True)
    for name in a.shapes.split(","):
        sh = SHAPES[name]
        W, C, L, n = sh["nwave"], sh["ncol"], sh["nlyr"], sh["nstr"]
        wl, wu = bench.wave_bounds(W, sh["band"], ck=sh["ck"])
        prop, bc, temf = bench.make_lw_inputs(list(range(W)), W, C, L, n, sh["band"], sh["tau"],
                                              dev)
        weights = torch.as_tensor(bench.gpoint_weights(W), device=dev)
        umu = torch.linspace(0.05, 1.0, 32, dtype=torch.float64, device=dev)
        nprop = prop.shape[-1]

        def solvers(nwave, ncol):
            bop = BeerLambertOptions().nstr(n).nwave(nwave).ncol(ncol).nlyr(L).planck(True)
            bop.wave_lower(list(wl)).wave_upper(list(wu))

            def disort(flags):
                op = DisortOptions().flags(flags).nwave(nwave).ncol(ncol)
                op.wave_lower(list(wl)).wave_upper(list(wu)).user_tau([0.0])
                op.ds().nlyr, op.ds().nstr, op.ds().nmom = L, n, n
                return Disort(op)
            return BeerLambert(bop), disort

        beer, disort = solvers(W, C)
        dflux = disort("lamber,quiet,onlyfl,planck")
        rc = sh.get("ray_cols", C)  # columns of the ray leg
        rprop, rbc, rtemf = prop[:, :rc].contiguous(), {k: v[:, :rc].contiguous() for k, v in bc.items()}, \
            temf[:rc].contiguous()
        rbeer, rdis = solvers(W, rc)
        drays = rdis("usrtau,lamber,quiet,planck")
        phi = torch.zeros_like(umu)
        legs = [
            ("forward", W * C, lambda: dflux.forward(prop, bc, temf),
             lambda: beer.forward(prop, bc, temf), 2 * (L + 1), C),
            ("forward_band", W * C, lambda: dflux.forward_band(prop, bc, temf, weights=weights),
             lambda: beer.forward_band(prop, bc, temf, weights=weights), 0, C),
            ("forward_rays", W * rc,
             lambda: drays.forward_rays(rprop, rbc, rtemf, umu=umu, phi=phi)[:, :, 0, :],
             lambda: rbeer.forward_rays(rprop, rbc, rtemf, umu=umu), 32, rc),
        ]
        path = os.path.join(a.out_dir, f"bench_{name}.jsonl")
        with open(path, "a") as f:
            for leg, nsolve, dfn, bfn, out_per_solve, ncol_leg in legs:
                est = {}
                for key, fn in (("disort", dfn), ("beer", bfn)):
                    for _ in range(a.warmup):
                        fn()
                    est[key], _ = timed(fn, 2)
                calls = {k: a.calls or max(2, min(2000, int(0.2 / v))) for k, v in est.items()}
                t = {"disort": [], "beer": []}
                res = {}
                for _ in range(a.rounds):
                    for key, fn in (("disort", dfn), ("beer", bfn)):
                        dt, res[key] = timed(fn, calls[key])
                        t[key].append(dt)
                d, b = res["disort"], res["beer"]
                scale = d.abs().reshape(d.shape[0], -1).amax(dim=1).reshape((-1,) + (1,) * (d.dim() - 1))
                diff = float(((b - d).abs() / scale.clamp_min(1e-300)).max())
                med = {k: float(np.median(v)) for k, v in t.items()}
                # bytes BeerLambert.<leg> must move: tau, the bc arrays given, temf, output
                out_bytes = 8 * (nsolve * out_per_solve if out_per_solve else
                                 ncol_leg * 2 * (L + 1))
                must = 8 * nsolve * L + 8 * nsolve * len(bc) + 8 * ncol_leg * (L + 1) + out_bytes
                lines = nsolve * -(-(L * nprop * 8) // 128) * 128  # every line holding a tau
                line = {"shape": name, "leg": leg,
                        "config": {"nwave": W, "ncol": ncol_leg, "nlyr": L, "nstr": n,
                                   "nprop": nprop, "rays": 32 if leg == "forward_rays" else 0},
                        "solves": nsolve, "rounds": a.rounds, "calls_per_round": calls,
                        "disort_ms": {"median": med["disort"] * 1e3, "min": min(t["disort"]) * 1e3,
                                      "max": max(t["disort"]) * 1e3},
                        "beer_ms": {"median": med["beer"] * 1e3, "min": min(t["beer"]) * 1e3,
                                    "max": max(t["beer"]) * 1e3},
                        "speedup_median": med["disort"] / med["beer"],
                        "beer_solves_per_s": nsolve / med["beer"],
                        "disort_solves_per_s": nsolve / med["disort"],
                        "beer_must_move_bytes": must, "beer_must_move_GBps": must / med["beer"] / 1e9,
                        "beer_tau_line_bytes": lines,
                        "beer_tau_line_GBps": lines / med["beer"] / 1e9,
                        "max_rel_diff_vs_disort": diff}
                print(json.dumps(line), flush=True)
                f.write(json.dumps(line) + "\n")
                if not diff < 1e-6:
                    raise SystemExit(f"bench_beer: {name} {leg}: BeerLambert differs from Disort "
                                     f"by {diff:.3e}")
        del prop, bc, temf, rprop, rbc, rtemf


if __name__ == "__main__":
    main()
