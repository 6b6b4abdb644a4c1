"""hd_solve_flx against hd_solve on the same inputs and context: HIP-event time per call.

    python scripts/bench_flx.py [--config c4|c5] [--steps 5] [--warmup 2] [--ncol N]

bench.py's C4 (nstr 16, nlyr 80, 640 000 solves) or C5 (nstr 32, 64 000 solves, the
aerosol band-loop optics) inputs; per-point outputs of both entries (forward: (.., 2),
forward_flx: (.., 8)), alternating calls on one stream and one context.  Prints one
JSON line: solves/s of each and their ratio.
"""

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=("c4", "c5"), default="c4")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ncol", type=int, default=None)
    a = ap.parse_args()
    from pyharp_amd import Disort, DisortOptions
    cfg = bench.CONFIGS[a.config]
    ncol = a.ncol or cfg["ncol"]
    W, nstr, nlyr = cfg["ngpoint"], cfg["nstr"], cfg["nlyr"]
    dev = torch.device("cuda", 0)
    gp = list(range(W))
    if cfg.get("aerosol"):
        prop, bc, _ = bench.make_aerosol_inputs(gp, W, ncol, nlyr, nstr, dev, umu0=cfg["umu0"])
    else:
        prop, bc, _ = bench.make_inputs(gp, ncol, nlyr, nstr, False, dev, ssa=cfg["ssa"],
                                        gasym=cfg["g"], umu0=cfg["umu0"])
    op = DisortOptions().flags("lamber,quiet,onlyfl").nwave(W).ncol(ncol)
    op.ds().nlyr, op.ds().nstr, op.ds().nmom = nlyr, nstr, nstr
    d = Disort(op)
    flux = torch.empty((W, ncol, nlyr + 1, 2), dtype=torch.float64, device=dev)
    flx = torch.empty((W, ncol, nlyr + 1, 8), dtype=torch.float64, device=dev)
    st = torch.zeros(W * ncol, dtype=torch.int32, device=dev)
    ms = {"hd_solve": [], "hd_solve_flx": []}
    for it in range(a.warmup + a.steps):
        for name, call in (("hd_solve", lambda: d.forward(prop, bc, status=st, out=flux)),
                           ("hd_solve_flx", lambda: d.forward_flx(prop, bc, status=st, out=flx))):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                ms[name].append(e0.elapsed_time(e1))
    n = W * ncol
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    up = (flx[..., 2] - flux[..., 0]).abs().max().item() / flux[..., 0].abs().max().item()
    print(json.dumps({
        "config": a.config, "nstr": nstr, "nlyr": nlyr, "solves": n, "steps": a.steps,
        "hd_solve_ms": [round(x, 3) for x in ms["hd_solve"]],
        "hd_solve_flx_ms": [round(x, 3) for x in ms["hd_solve_flx"]],
        "hd_solve_solves_per_s": n / mean["hd_solve"] * 1e3,
        "hd_solve_flx_solves_per_s": n / mean["hd_solve_flx"] * 1e3,
        "flx_over_solve": mean["hd_solve"] / mean["hd_solve_flx"],
        "flup_max_diff_over_max": up,
        "status_errors": int((st & 0x0F).ne(0).sum().item())}))


if __name__ == "__main__":
    main()
