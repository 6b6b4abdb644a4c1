"""Regenerate tests/golden/spher_hard.npz: inputs (prop, bc, temf, zd, radius) and the
arbitrary-precision record (oracle/disort_mp.py with zd / radius, 50 digits) of every
pseudo-spherical hard-regime case of tests/spher_hard_cases.py.

    python tests/golden/make_spher_hard_golden.py [nproc [NSTR,NSTR,...]]

(with a list of nstr: a dry run of those, every check made, nothing written).

Admission.  Every column is solved for two beam paths that share one factorisation: its
own geometry at 50 digits, and the slant depths and secants as tests/spher_ref.py
evaluates them in double.  The two records must agree to ADMIT in helpers.rel_err, or the
generator stops: an input whose answer depends on how its geometry was rounded cannot
tell a wrong kernel from an ill-conditioned column.  No column is ever left out.  The
resonance family's realised delta (50 digits, from the stored doubles) is stored beside the
one asked for and must be within spher_hard_cases.DELTA_TOL of it.

CPU only: 1314 columns (219 per nstr), 34 CPU-minutes in all with both beam paths (12 s a
column of five layers at nstr 32, 4 s one of three, 0.1 s at nstr 8: the dense LU of the
boundary system is the cost, and it is shared), 6 minutes of wall clock on 8 processes
(the default is min(8, cpu count)).  The worst admission gap was 7.4e-16.

tests/test_mp_oracle.py recomputes a sample of the stored cases, so a stale file fails.
"""

import multiprocessing
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import spher_hard_cases as cases  # noqa: E402
from hard_cases import bc_keys  # noqa: E402
from helpers import rel_err  # noqa: E402
from oracle.disort_mp import flux_of_record  # noqa: E402

ADMIT = 1.0e-8


def _job(args):
    family, nstr, ib, c = args
    t = time.process_time()
    b = cases.batches(family, nstr)[ib]
    ref, _, alt, delta = cases.reference(b, [c], admission=True)
    gap = float(rel_err(flux_of_record(alt), flux_of_record(ref)).max())
    return args, ref[:, 0], gap, float(delta[0]), time.process_time() - t


def main():
    nproc = int(sys.argv[1]) if len(sys.argv) > 1 else min(8, os.cpu_count() or 1)
    only = [int(n) for n in sys.argv[2].split(",")] if len(sys.argv) > 2 else cases.NSTR
    t0 = time.time()
    out, jobs = {}, []
    for nstr in reversed(only):  # the long columns first
        for family in cases.FAMILIES:
            for ib, b in enumerate(cases.batches(family, nstr)):
                k = cases.key(family, nstr, b["name"])
                ncol = b["prop"].shape[1]
                out[k + "/prop"] = b["prop"]
                out[k + "/bc"] = np.stack([b["bc"][name] for name in bc_keys(b)])
                if b["temf"] is not None:
                    out[k + "/temf"] = b["temf"]
                out[k + "/zd"] = b["zd"]
                out[k + "/radius"] = np.float64(b["radius"])
                if "delta" in b:
                    out[k + "/delta"] = b["delta"]
                    out[k + "/delta_realised"] = np.zeros(ncol)
                out[k + "/ref"] = np.zeros((1, ncol, b["nlyr"] + 1, 8))
                jobs += [(family, nstr, ib, c) for c in range(ncol)]
    names = {(f, n): [b["name"] for b in cases.batches(f, n)]
             for f in cases.FAMILIES for n in only}
    worst, cpu = 0.0, 0.0
    with multiprocessing.Pool(nproc) as pool:
        for done, ((family, nstr, ib, c), ref, gap, delta, sec) in enumerate(
                pool.imap_unordered(_job, jobs, chunksize=1)):
            k = cases.key(family, nstr, names[family, nstr][ib])
            # the admission rule: a failure, never a column dropped
            assert gap <= ADMIT, f"{k} column {c}: double geometry moves the answer by {gap:.2e}"
            out[k + "/ref"][:, c] = ref
            if k + "/delta" in out:
                asked = out[k + "/delta"][c]
                assert abs(delta - asked) <= cases.DELTA_TOL, (k, c, asked, delta)
                out[k + "/delta_realised"][c] = delta
            worst, cpu = max(worst, gap), cpu + sec
            if done % 50 == 0:
                print(f"{done} / {len(jobs)}", flush=True)
    print(f"{len(jobs)} columns, {cpu / 60:.1f} CPU-minutes, {(time.time() - t0) / 60:.1f} "
          f"minutes of wall clock; admission: worst gap {worst:.2e}")
    if tuple(only) == tuple(cases.NSTR):
        np.savez_compressed(os.path.join(HERE, "spher_hard.npz"), **out)
    else:
        print("a subset of nstr: nothing written")


if __name__ == "__main__":
    main()
