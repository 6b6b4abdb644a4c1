"""The optics gradients beside their forward calls, in one process.

    python scripts/bench_optics_grad.py [--shapes batch,c3,c1] [--rounds 7] [--calls 0]
                                        [--warmup 3] [--out-dir profiles/optics_grad]

Shapes (nwave x ncol x nlyr): batch 64 x 10 000 x 80, c3 19 990 x 1 x 40, c1 16 x 1 x 40.
Legs: RFM.forward (a synthetic table of 12 pressures x 5 anomalies; conc with 2 species, pres
and temp require grad) and band_loop_optics (two table attenuators with asymmetry tables on
two species, nmom 8, the RFM extinction as ext0; conc, dz and ext0 require grad), each with
the scalar loss sum(result).

Method (that of scripts/bench_beer_grad.py): after `warmup` calls, `rounds` rounds alternate
the forward alone (no input requires grad: the plain path) and forward + backward; a round
times `calls` back-to-back calls with a host clock around work that ends in a device
synchronise (calls = 0: as many as fill about 0.2 s).  Reported per leg, one JSON line into
<out-dir>/bench_<shape>.jsonl: the medians, backward = (forward + backward) - forward, the
ratio backward / forward, and the bytes each must move with the rate that implies.  Forward:
inputs read, output written.  Backward: the cotangent read once, the inputs read, the
gradients written, the block partials of the few-column route written and read (per-wave
coefficient scratch and the RFM table's touched corners are left out: kilobytes, cached).
The backward figure includes what autograd adds around the kernel: the loss's expand of the
cotangent to the output's size (written once: counted) and the accumulation into .grad.
Nothing is measured without a HIP device.
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

SHAPES = {"batch": (64, 10000, 80), "c3": (19990, 1, 40), "c1": (16, 1, 40)}
WB, DIRECT = 32, 8192  # kWaveBlock, kDirectLanes of pyharp_amd/csrc/hd_harp_grad.hip
NMOM = 8


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def attenuators(tmp):
    from pyharp_amd.opacity import AttenuatorOptions, H2SO4Simple, S8Fuller
    rng = np.random.default_rng(11)
    out = []
    for i, cls in enumerate((S8Fuller, H2SO4Simple)):
        wl = np.linspace(0.2, 60.0, 200)
        path = os.path.join(tmp, f"bench_att_{i}.txt")
        with open(path, "w") as f:
            for x in wl:
                f.write(f"{float(x)!r} {float(rng.uniform(0.5, 3.0))!r} "
                        f"{float(rng.uniform(0.1, 0.95))!r}\n")
        op = AttenuatorOptions().opacity_files([path]).species_ids([i]).species_weights([1.0, 1.0])
        out.append(cls(op).set_asymmetry(rng.uniform(-0.8, 0.8, 200)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="batch,c3,c1")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "optics_grad"))
    a = ap.parse_args()
    import tempfile
    from pyharp_amd.opacity import RFM, band_loop_optics
    if not torch.cuda.is_available():
        raise SystemExit("bench_optics_grad: no HIP device (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    os.makedirs(a.out_dir, exist_ok=True)
    tmp = tempfile.mkdtemp()
    atts = attenuators(tmp)
    for name in a.shapes.split(","):
        W, C, L = SHAPES[name]
        rng = np.random.default_rng(W)
        ptab = np.logspace(5, 0, 12)
        rfm = RFM.from_arrays(np.linspace(10.0, 2500.0, W), ptab, np.linspace(-40.0, 40.0, 5),
                              np.linspace(300.0, 160.0, 12), rng.uniform(-4.0, 2.0, (W, 12, 5)))
        t = lambda x: torch.as_tensor(x, dtype=torch.float64, device=dev)  # noqa: E731
        conc = t(rng.uniform(0.05, 2.0, (C, L, 2)))
        pres = t(np.exp(rng.uniform(np.log(2.0), np.log(5.0e4), (C, L))))
        temp = t(rng.uniform(170.0, 290.0, (C, L)))
        dz = t(rng.uniform(100.0, 2000.0, (C, L)))
        kw = {"wavenumber": t(np.linspace(200.0, 2500.0, W))}
        with torch.no_grad():
            ext0 = rfm.forward(conc, {"pres": pres, "temp": temp})[..., 0].contiguous()
        n, ncl = W * C * L, C * L
        nwb = -(-W // WB)
        few = ncl < DIRECT and 1 < nwb <= 65535

        def leaf(x):
            return x.detach().requires_grad_(True)

        def rfm_fwd():
            return rfm.forward(conc, {"pres": pres, "temp": temp})

        def rfm_fwd_bwd():
            c, p, T = leaf(conc), leaf(pres), leaf(temp)
            rfm.forward(c, {"pres": p, "temp": T}).sum().backward()
            return c.grad

        def loop_fwd():
            return band_loop_optics(atts, conc, dz, kw, NMOM, ext0)

        def loop_fwd_bwd():
            c, d, e = leaf(conc), leaf(dz), leaf(ext0)
            band_loop_optics(atts, c, d, kw, NMOM, e).sum().backward()
            return c.grad

        nprop = 2 + NMOM
        legs = (
            ("RFM.forward", rfm_fwd, rfm_fwd_bwd,
             {"inputs": 8 * ncl * 4, "out": 8 * n},
             {"gout_expand_write": 8 * n, "gout_read": 8 * n, "inputs": 8 * ncl * 4,
              "gradients": 8 * ncl * 4, "partials_write_read": 2 * 8 * nwb * 3 * ncl if few else 0}),
            ("band_loop_optics", loop_fwd, loop_fwd_bwd,
             {"inputs": 8 * ncl * 3 + 8 * n, "out": 8 * n * nprop},
             {"gout_expand_write": 8 * n * nprop, "gout_read": 8 * n * nprop,
              "inputs": 8 * ncl * 3 + 8 * n, "gradients": 8 * ncl * 3 + 8 * n,
              "partials_write_read": 2 * 8 * nwb * 3 * ncl if few else 0}))
        path = os.path.join(a.out_dir, f"bench_{name}.jsonl")
        with open(path, "a") as f:
            for leg, fwd, fwd_bwd, fparts, bparts in legs:
                est = {}
                for key, fn in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
                    for _ in range(a.warmup):
                        fn()
                    est[key] = timed(fn, 2)
                calls = {k: a.calls or max(2, min(2000, int(0.2 / v))) for k, v in est.items()}
                tt = {"fwd": [], "fwd_bwd": []}
                for _ in range(a.rounds):
                    for key, fn in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
                        tt[key].append(timed(fn, calls[key]))
                med = {k: float(np.median(v)) for k, v in tt.items()}
                bwd = med["fwd_bwd"] - med["fwd"]
                fmust, bmust = sum(fparts.values()), sum(bparts.values())
                line = {"shape": name, "leg": leg,
                        "config": {"nwave": W, "ncol": C, "nlyr": L, "nspecies": 2,
                                   "nmom": NMOM if leg != "RFM.forward" else 0,
                                   "route": "few columns: partials" if few else "a lane per (col, lyr)"},
                        "rounds": a.rounds, "calls_per_round": calls,
                        "fwd_ms": {"median": med["fwd"] * 1e3, "min": min(tt["fwd"]) * 1e3,
                                   "max": max(tt["fwd"]) * 1e3},
                        "fwd_bwd_ms": {"median": med["fwd_bwd"] * 1e3, "min": min(tt["fwd_bwd"]) * 1e3,
                                       "max": max(tt["fwd_bwd"]) * 1e3},
                        "bwd_ms": bwd * 1e3, "bwd_over_fwd": bwd / med["fwd"],
                        "fwd_must_move_bytes": fmust, "fwd_must_move_parts": fparts,
                        "fwd_must_move_GBps": fmust / med["fwd"] / 1e9,
                        "bwd_must_move_bytes": bmust, "bwd_must_move_parts": bparts,
                        "bwd_must_move_GBps": bmust / bwd / 1e9}
                print(json.dumps(line), flush=True)
                f.write(json.dumps(line) + "\n")
        del conc, pres, temp, dz, ext0


if __name__ == "__main__":
    main()
