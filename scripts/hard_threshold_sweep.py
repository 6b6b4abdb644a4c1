#!/usr/bin/env python3
"""Sweep the two cold-branch constants of the flux layer kernels against the mp reference.

    python scripts/hard_threshold_sweep.py > profiles/hard/threshold_sweep.txt
    python scripts/hard_threshold_sweep.py --device-logs BEFORE.log AFTER.log \
        > profiles/hard/threshold_sweep_gpu.txt

Without arguments, on the CPU: tests/kernel_model.py over the resonance and thin_thermal
families of tests/golden/flux_hard.npz for a range of RES_MOVE (kResMove) and THIN_TAU
(kThinTau), plus the earlier rules (clamp at 1e-9, Q~- = I - A- at every depth); worst
helpers.rel_err per setting.  The sweep over the constants is this CPU model's alone: the
constants are compile-time in the kernels, and the device was measured at two points only,
the parent commit's library and the chosen values.

--device-logs: the tables of those two device runs, from the output of
`pytest tests/test_gpu_hard.py -m gpu -v -s` on the parent's library (HD_LIB_PATH) and on
this tree's.
"""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hard_cases  # noqa: E402
import kernel_model  # noqa: E402
from helpers import GOLDEN, rel_err  # noqa: E402
from oracle.disort_mp import flux_of_record  # noqa: E402
from test_kernel_model import _model_batch  # noqa: E402

NSTR = (2, 4, 8, 16)


def worst(fix, family, names=None, all_families=False):
    out = []
    for nstr in NSTR:
        fams = hard_cases.FAMILIES if all_families else (family,)
        e = 0.0
        for fam in fams:
            for b in fix[fam, nstr]:
                if names and b["name"] not in names:
                    continue
                e = max(e, rel_err(_model_batch(b), flux_of_record(b["ref"])).max())
        out.append(e)
    return out


def device_tables(before, after):
    import collections
    import re
    nstrs = hard_cases.NSTR
    print("tests/test_gpu_hard.py on an MI355X: Disort.forward against oracle/disort_mp.py,")
    print("helpers.rel_err.  Two points only: the parent commit's library (clamp at 1e-9,")
    print("Q~- = I - A- at every depth) and this tree's (kResMove = 3e-8, kThinTau = 1e-3); the")
    print("sweep over the constants is the CPU model's (threshold_sweep.txt).")
    print()
    logs = {}
    for tag, path in (("parent", before), ("this tree", after)):
        log = logs[tag] = open(path).read()
        worst = collections.defaultdict(float)
        for m in re.finditer(r"(\w+) n(\d+) (\w+): worst ([0-9.e+-]+)", log):
            key = (m.group(1), int(m.group(2)))
            worst[key] = max(worst[key], float(m.group(4)))
        print(f"{tag}: worst per family; columns: nstr " + ", ".join(map(str, nstrs)))
        for fam in hard_cases.FAMILIES:
            print(f"  {fam:14s}  " + "  ".join(f"{worst[fam, n]:9.2e}" for n in nstrs))
        print()

    def columns(log, fam, n, name):
        m = re.search(rf"{fam} n{n} {name}: worst \S+ \(column \d+\)\s+per column \[([^\]]*)\]", log)
        return m.group(1).split()

    for n in (8, 32):
        print(f"resonance, scattering layer, nstr {n}: per delta, parent | this tree")
        cols = [columns(logs[t], "resonance", n, "scat") for t in ("parent", "this tree")]
        order = sorted(range(len(hard_cases.DELTAS)),
                       key=lambda i: (abs(hard_cases.DELTAS[i]), hard_cases.DELTAS[i]))
        for i in order:
            print(f"  delta {hard_cases.DELTAS[i]:9.1e}: {cols[0][i]:>8s} | {cols[1][i]:>8s}")
        print()
    for n in (8, 32):
        print(f"thin_thermal, top layer of two, nstr {n}: per (tau, ssa), parent | this tree")
        cols = [columns(logs[t], "thin_thermal", n, "top2") for t in ("parent", "this tree")]
        k = 0
        for t in hard_cases.THIN_TAU:
            for ssa in (0.0, 0.5):
                print(f"  tau {t:6.0e} ssa {ssa}: {cols[0][k]:>8s} | {cols[1][k]:>8s}")
                k += 1
        print()


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--device-logs":
        return device_tables(sys.argv[2], sys.argv[3])
    fix = hard_cases.load(GOLDEN)
    fmt = lambda es: "  ".join(f"{e:9.2e}" for e in es)  # noqa: E731
    print("kernel model (tests/kernel_model.py) vs oracle/disort_mp.py, helpers.rel_err, worst")
    print("over the family's columns; columns: nstr " + ", ".join(map(str, NSTR)))
    print()
    print("resonance family (|delta| from 0 to 1e-3 on a scattering and an absorbing layer)")
    saved = kernel_model.RES_MOVE, kernel_model.RES_CLAMP, kernel_model.THIN_TAU
    kernel_model.RES_CLAMP = 1.0e-9
    print(f"  clamp 1e-9 (earlier rule)   {fmt(worst(fix, 'resonance'))}")
    kernel_model.RES_CLAMP = None
    for mv in (1e-10, 1e-9, 1e-8, 3e-8, 1e-7, 3e-7, 1e-6, 1e-5):
        kernel_model.RES_MOVE = mv
        print(f"  secant moved by {mv:7.0e}     {fmt(worst(fix, 'resonance'))}")
    kernel_model.RES_MOVE = saved[0]
    print()
    print(f"per delta with kResMove = {saved[0]:g} (scattering layer; the window is")
    print("|delta| < kResMove / 2 in umu0), the fixture's deltas and the window's outer edge")
    for nstr in (8, 16):
        b = hard_cases.batches("resonance", nstr)[0]
        _, k = hard_cases.resonance_k(nstr, True)
        extra = [s * d for d in (1.6e-8, 2e-8, 3e-8, 1e-7) for s in (1.0, -1.0)]
        n = len(extra)
        e = dict(b, prop=b["prop"][:, :n].copy(), bc={kk: v[:, :n].copy() for kk, v in b["bc"].items()})
        with hard_cases.disort_mp.mp.workdps(50):
            e["bc"]["umu0"][0] = [float((1 + hard_cases.disort_mp.mpf(d)) / k) for d in extra]
        ref, _ = hard_cases.reference(e)
        err = list(rel_err(_model_batch(e), flux_of_record(ref)).max(axis=(0, 2, 3)))
        fb = [x for x in fix["resonance", nstr] if x["name"] == "scat"][0]
        err += list(rel_err(_model_batch(fb), flux_of_record(fb["ref"])).max(axis=(0, 2, 3)))
        for d, x in sorted(zip(extra + list(hard_cases.DELTAS), err), key=lambda t: (abs(t[0]), t[0])):
            print(f"  nstr {nstr:2d} delta {d:9.1e}: {x:9.2e}")
    print()
    print("thin_thermal family (10 K across a layer of tau 1e-3 .. 1e-15)")
    for th in (0.0, 1e-8, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1.0):
        kernel_model.THIN_TAU = th
        label = "I - A- everywhere (earlier)" if th == 0.0 else f"A- Om Om^T below {th:6.0e}"
        print(f"  {label:28s}  {fmt(worst(fix, 'thin_thermal'))}")
    print()
    print("between the fixture's depths: the two-layer column of the family, nstr 8 and 16,")
    print("10 K across a top layer of depth tau; Q~- x as I - A- | as A- Omega Omega^T")
    for nstr in (8, 16):
        for tau in (1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7):
            b = hard_cases.batches("thin_thermal", nstr)[0]
            b["prop"] = b["prop"][:, :2].copy()
            b["prop"][0, :, 1, 0] = tau  # the top layer (harp: last)
            b["bc"] = {k: v[:, :2] for k, v in b["bc"].items()}
            b["temf"] = b["temf"][:2]
            ref, _ = hard_cases.reference(b)
            kernel_model.THIN_TAU = 0.0
            diff = rel_err(_model_batch(b), flux_of_record(ref)).max()
            kernel_model.THIN_TAU = 10.0
            prod = rel_err(_model_batch(b), flux_of_record(ref)).max()
            print(f"  nstr {nstr:2d} tau {tau:6.0e}:  {diff:9.2e} | {prod:9.2e}")
    kernel_model.RES_MOVE, kernel_model.RES_CLAMP, kernel_model.THIN_TAU = saved
    print()
    print(f"chosen: kResMove = {saved[0]:g}, kThinTau = {saved[2]:g}; every family with them:")
    for fam in hard_cases.FAMILIES:
        print(f"  {fam:14s}  {fmt(worst(fix, fam))}")


if __name__ == "__main__":
    main()
