"""Regenerate tests/golden/flx_parity.npz: inputs and the CPU reference record
(tests/flx_ref.py) of every parity case of tests/test_gpu_flx.py.

    python tests/golden/make_flx_golden.py        (a few minutes, CPU only)

tests/test_flx_ref.py recomputes a sample of the stored cases, so a stale file fails.
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import flx_ref  # noqa: E402


def main():
    out = {}
    for nstr in flx_ref.PARITY_NSTR:
        for nlyr in flx_ref.PARITY_NLYR:
            for source in flx_ref.PARITY_SOURCES:
                key = flx_ref.parity_key(nstr, nlyr, source)
                prop, bc, temf = flx_ref.parity_inputs(nstr, nlyr, source)
                ref, scale = flx_ref.parity_reference(nstr, nlyr, source)
                out[key + "/prop"] = prop
                for k, v in bc.items():
                    out[key + "/bc_" + k] = v
                if temf is not None:
                    out[key + "/temf"] = temf
                out[key + "/ref"] = ref
                out[key + "/scale"] = scale
                print(key, flush=True)
    np.savez_compressed(os.path.join(HERE, "flx_parity.npz"), **out)


if __name__ == "__main__":
    main()
