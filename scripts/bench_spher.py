"""hd_solve_spher against hd_solve on the same inputs and context: HIP-event time per call.

    python scripts/bench_spher.py [--config c4|c5] [--steps 5] [--warmup 2] [--ncol N]

bench.py's C4 (nstr 16, nlyr 80, 640 000 solves) or C5 (nstr 32, 64 000 solves, the
aerosol band-loop optics) inputs; `forward(..., zd=)` of a module with the 'spher' flag
(a Mars-sized body, levels evenly up to 100 km) beside the plain `forward` on the same
tensors, stream and context, calls alternating.  Prints one JSON line: solves/s of each
and their ratio.  The prologue's own time (hd_spher_kernel, the O(nlyr^2) slant depths)
is read from a kernel trace of this script:

    rocprofv3 --kernel-trace --stats -d DIR -o kt --output-format csv -- \
        python scripts/bench_spher.py --config c4 --steps 3
"""

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

RADIUS, ZTOP = 3.39e6, 1.0e5


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

    def module(flags):
        op = DisortOptions().flags(flags).nwave(W).ncol(ncol).radius(RADIUS)
        op.ds().nlyr, op.ds().nstr, op.ds().nmom = nlyr, nstr, nstr
        return Disort(op)

    plain, spher = module("lamber,quiet,onlyfl"), module("lamber,quiet,onlyfl,spher")
    zd = torch.linspace(0.0, ZTOP, nlyr + 1, dtype=torch.float64, device=dev)
    f_pp = torch.empty((W, ncol, nlyr + 1, 2), dtype=torch.float64, device=dev)
    f_sp = torch.empty_like(f_pp)
    st = torch.zeros(W * ncol, dtype=torch.int32, device=dev)
    ms = {"hd_solve": [], "hd_solve_spher": []}
    errors = 0
    for it in range(a.warmup + a.steps):
        for name, call in (
                ("hd_solve", lambda: plain.forward(prop, bc, status=st, out=f_pp)),
                ("hd_solve_spher", lambda: spher.forward(prop, bc, status=st, out=f_sp, zd=zd))):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            errors += int((st & 0x0F).ne(0).sum().item())
            if it >= a.warmup:
                ms[name].append(e0.elapsed_time(e1))
    n = W * ncol
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    print(json.dumps({
        "config": a.config, "nstr": nstr, "nlyr": nlyr, "solves": n, "steps": a.steps,
        "hd_solve_ms": [round(x, 3) for x in ms["hd_solve"]],
        "hd_solve_spher_ms": [round(x, 3) for x in ms["hd_solve_spher"]],
        "hd_solve_solves_per_s": n / med["hd_solve"] * 1e3,
        "hd_solve_spher_solves_per_s": n / med["hd_solve_spher"] * 1e3,
        "spher_over_solve": med["hd_solve"] / med["hd_solve_spher"],
        "surface_down_spher_over_plane": (f_sp[:, :, 0, 1].mean() / f_pp[:, :, 0, 1].mean()).item(),
        "status_errors": errors}))


if __name__ == "__main__":
    main()
