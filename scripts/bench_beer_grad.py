"""The Beer-Lambert gradients beside their forward calls, in one process.

    python scripts/bench_beer_grad.py [--shapes c1,c3,batch] [--rounds 7] [--calls 0]
                                      [--warmup 3] [--out-dir profiles/beer_grad]

Shapes: those of scripts/bench_beer.py (C1, C3, and 10 000 columns x 64 waves x nlyr 80 at
nstr 16; the ray leg of the batched shape on 1 000 columns, 32 upward rays), with prop
reduced to its optical-depth slot (nprop 1, a view of the tau leaf: no prop-sized
gradient is ever formed).  Legs: forward_band and forward_rays_band with the scalar loss
sum(result); tau, temf and every boundary condition require grad.

Method: after `warmup` calls, `rounds` rounds alternate the forward alone (no input
requires grad: the plain path) and forward + backward; a round times `calls` back-to-back
calls with a host clock around work that ends in a device synchronise (calls = 0: as many
as fill about 0.2 s).  Reported per leg, one JSON line into <out-dir>/bench_<shape>.jsonl:
the medians, backward = (forward + backward) - forward, the ratio backward / forward, and
the bytes the backward must move -- tau twice, the scratch between the adjoint's two sweeps
written and read once (2 NN nlyr doubles per solve), dL/dB per level written, scaled and
read, and the gradients -- with the rate that implies.  Nothing is measured without a HIP
device.
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c1,c3,batch")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "beer_grad"))
    a = ap.parse_args()
    import bench
    from bench_beer import SHAPES
    from pyharp_amd import BeerLambert, BeerLambertOptions
    if not torch.cuda.is_available():
        raise SystemExit("bench_beer_grad: no HIP device (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    os.makedirs(a.out_dir, exist_ok=True)
    for name in a.shapes.split(","):
        sh = SHAPES[name]
        W, C, L, n = sh["nwave"], sh["ncol"], sh["nlyr"], sh["nstr"]
        wl, wu = bench.wave_bounds(W, sh["band"], ck=sh["ck"])
        prop, bc, temf = bench.make_lw_inputs(list(range(W)), W, C, L, n, sh["band"], sh["tau"],
                                              dev)
        tau = prop[..., 0].contiguous()
        del prop
        weights = torch.as_tensor(bench.gpoint_weights(W), device=dev)
        umu = torch.linspace(0.05, 1.0, 32, dtype=torch.float64, device=dev)

        def solver(ncol):
            op = BeerLambertOptions().nstr(n).nwave(W).ncol(ncol).nlyr(L).planck(True)
            return BeerLambert(op.wave_lower(list(wl)).wave_upper(list(wu)))

        rc = sh.get("ray_cols", C)
        legs = [("forward_band", C, {}), ("forward_rays_band", rc, dict(umu=umu))]
        path = os.path.join(a.out_dir, f"bench_{name}.jsonl")
        with open(path, "a") as f:
            for leg, ncol, kws in legs:
                b = solver(ncol)
                t0 = tau[:, :ncol].contiguous()
                bc0 = {k: v[:, :ncol].contiguous() for k, v in bc.items()}
                tf0 = temf[:ncol].contiguous()
                call = getattr(b, leg)

                def fwd():
                    return call(t0.unsqueeze(-1), bc0, tf0, weights=weights, **kws)

                def fwd_bwd():
                    t = t0.detach().requires_grad_(True)
                    bcs = {k: v.detach().requires_grad_(True) for k, v in bc0.items()}
                    tf = tf0.detach().requires_grad_(True)
                    call(t.unsqueeze(-1), bcs, tf, weights=weights, **kws).sum().backward()
                    return t.grad

                est = {}
                for key, fn in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
                    for _ in range(a.warmup):
                        fn()
                    est[key] = timed(fn, 2)
                calls = {k: a.calls or max(2, min(2000, int(0.2 / v))) for k, v in est.items()}
                t = {"fwd": [], "fwd_bwd": []}
                for _ in range(a.rounds):
                    for key, fn in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
                        t[key].append(timed(fn, calls[key]))
                med = {k: float(np.median(v)) for k, v in t.items()}
                bwd = med["fwd_bwd"] - med["fwd"]
                S, nn = W * ncol, n // 2
                parts = {"tau_twice": 2 * 8 * S * L, "sweep_scratch_write_read": 2 * 8 * S * 2 * nn * L,
                         "dLdB_write_scale_read": 4 * 8 * S * (L + 3),
                         "gradients": 8 * S * L + 8 * S * len(bc0) + 8 * ncol * (L + 1)}
                must = sum(parts.values())
                line = {"shape": name, "leg": leg,
                        "config": {"nwave": W, "ncol": ncol, "nlyr": L, "nstr": n, "nprop": 1,
                                   "rays": 32 if kws else 0},
                        "solves": S, "rounds": a.rounds, "calls_per_round": calls,
                        "fwd_ms": {"median": med["fwd"] * 1e3, "min": min(t["fwd"]) * 1e3,
                                   "max": max(t["fwd"]) * 1e3},
                        "fwd_bwd_ms": {"median": med["fwd_bwd"] * 1e3, "min": min(t["fwd_bwd"]) * 1e3,
                                       "max": max(t["fwd_bwd"]) * 1e3},
                        "bwd_ms": bwd * 1e3, "bwd_over_fwd": bwd / med["fwd"],
                        "bwd_must_move_bytes": must, "bwd_must_move_parts": parts,
                        "bwd_must_move_GBps": must / bwd / 1e9}
                print(json.dumps(line), flush=True)
                f.write(json.dumps(line) + "\n")
        del tau, bc, temf


if __name__ == "__main__":
    main()
