"""Regenerate tests/golden/flux_hard.npz: inputs and the arbitrary-precision record
(oracle/disort_mp.py, 50 digits) of every hard-regime case of tests/hard_cases.py.

    python tests/golden/make_hard_golden.py [nproc]

CPU only: 838 columns, 16 CPU-minutes in all (6 s a column at nstr 32, 0.2 s at nstr 8),
2 minutes of wall clock on 8 processes (the default is min(8, cpu count)).

tests/test_mp_oracle.py recomputes a sample of the stored cases, so a stale file fails.
"""

import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import hard_cases  # noqa: E402


def _job(args):
    family, nstr, ib, c = args
    b = hard_cases.batches(family, nstr)[ib]
    ref, scale = hard_cases.reference(b, [c])
    return args, ref[:, 0], scale[:, 0]


def main():
    nproc = int(sys.argv[1]) if len(sys.argv) > 1 else min(8, os.cpu_count() or 1)
    out, jobs = {}, []
    for nstr in reversed(hard_cases.NSTR):  # the long columns first
        for family in hard_cases.FAMILIES:
            for ib, b in enumerate(hard_cases.batches(family, nstr)):
                k = hard_cases.key(family, nstr, b["name"])
                ncol = b["prop"].shape[1]
                # nmom is prop's last extent - 2; dfdt's scale is rebuilt from the record
                # (hard_cases.load): few, large entries keep the file small
                out[k + "/prop"] = b["prop"]
                out[k + "/bc"] = np.stack([b["bc"][name] for name in hard_cases.bc_keys(b)])
                if b["temf"] is not None:
                    out[k + "/temf"] = b["temf"]
                out[k + "/ref"] = np.zeros((1, ncol, b["nlyr"] + 1, 8))
                jobs += [(family, nstr, ib, c) for c in range(ncol)]
    names = {(f, n): [b["name"] for b in hard_cases.batches(f, n)]
             for f in hard_cases.FAMILIES for n in hard_cases.NSTR}
    with multiprocessing.Pool(nproc) as pool:
        for done, ((family, nstr, ib, c), ref, scale) in enumerate(
                pool.imap_unordered(_job, jobs, chunksize=1)):
            k = hard_cases.key(family, nstr, names[family, nstr][ib])
            out[k + "/ref"][:, c] = ref
            if done % 50 == 0:
                print(f"{done} / {len(jobs)}", flush=True)
    np.savez_compressed(os.path.join(HERE, "flux_hard.npz"), **out)


if __name__ == "__main__":
    main()
