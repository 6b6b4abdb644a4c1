"""The nstr <= 16 layer kernel's Jacobi after its per-rotation bookkeeping was trimmed.

The FP32-angle rotation no longer skips a pair on a relative test of its coupling: every
pair of a lane that is still rotating rotates, and a converged lane gets t = 0 through the
angle's numerator.  Two properties that this could break and that no other test isolates:

* a lane's result does not depend on the solves that share its wave (a converged lane
  performs exact no-ops while its wave-mates go on sweeping);
* couplings that are exactly zero, with equal or zero column norms, give t = 0 and not a
  0 * inf (layers without scattering, of zero depth, conservative, identical).
"""

import numpy as np
import pytest
import torch

from helpers import TOL, margin, rel_err
from test_gpu_parity import _disort, _run

pytestmark = pytest.mark.gpu


def _hg(prop, g):
    for l in range(prop.shape[-1] - 2):
        prop[..., 2 + l] = g ** (l + 1)


@pytest.mark.parametrize("nstr", [4, 6, 16])
def test_wave_mates_do_not_matter(nstr):
    """One wave of 64 columns; lanes 0 and 37 hold a fixed solve, the other 62 once
    converge in the first sweep (omega = 0) and once take the most sweeps."""
    ncol, nlyr = 64, 3
    targets = [0, 37]
    tau = np.array([0.3, 1.0, 3.0])
    bc = {"albedo": np.full((1, ncol), 0.3), "fbeam": np.ones((1, ncol)),
          "umu0": np.full((1, ncol), 0.6)}
    d = _disort(nstr, nlyr, 1, ncol)
    dev = torch.device("cuda", 0)
    res = []
    for ssa, g in ((0.0, 0.0), (0.9999, 0.9)):
        prop = np.zeros((1, ncol, nlyr, 2 + nstr))
        prop[..., 0] = tau
        prop[..., 1] = ssa
        _hg(prop, np.full((1, ncol, nlyr), g))
        tgt = prop[:, targets]
        tgt[..., 1] = 0.9
        _hg(tgt, np.full((1, len(targets), nlyr), 0.7))
        prop[:, targets] = tgt
        st = torch.zeros(ncol, dtype=torch.int32, device=dev)
        f = _run(d, prop, bc, status=st)
        res.append((f[0, targets], st.cpu().numpy()[targets]))
    assert np.isfinite(res[0][0]).all()
    assert np.array_equal(res[0][0], res[1][0])
    assert np.array_equal(res[0][1], res[1][1])


def _degenerate_columns(nstr, ncol=16, nlyr=4):
    """Columns of five kinds, cycled: no scattering at all (every coupling exactly zero);
    one layer of zero depth among ordinary ones; conservative isotropic; conservative
    forward-peaked; four identical layers.  The beam angle and the depth scale vary
    from one cycle to the next.

    oracle/disort_np.py and the C oracle agree to 1e-13 on these inputs except on the
    omega = 1 columns: there disort_np stands up to 2.1e-7 from the C oracle, and the C
    oracle up to 5.0e-8 from oracle/disort_mp.py at 50 digits (nstr 16 with Planck) --
    the dithered conservative layer is ill-conditioned in the references too, at any
    depth tried (profiles/layerdiet/parity.txt)."""
    prop = np.zeros((1, ncol, nlyr, 2 + nstr))
    umu0 = np.zeros((1, ncol))
    for c in range(ncol):
        kind, rep = c % 5, c // 5
        scale = (0.5, 1.0, 2.0, 0.1)[rep]
        umu0[0, c] = (1.0, 0.6, 0.3, 0.85)[rep]
        tau = scale * np.array([0.2, 0.5, 1.0, 2.0])
        ssa = np.array([0.5, 0.8, 0.95, 0.3])
        g = np.array([0.2, 0.5, 0.8, 0.0])
        if kind == 0:
            ssa = np.zeros(nlyr)
        elif kind == 1:
            tau[rep % nlyr] = 0.0
        elif kind == 2:
            ssa, g = np.ones(nlyr), np.zeros(nlyr)
        elif kind == 3:
            ssa, g = np.ones(nlyr), np.full(nlyr, 0.9)
        else:
            tau, ssa, g = np.full(nlyr, scale), np.full(nlyr, 0.7), np.full(nlyr, 0.6)
        prop[0, c, :, 0] = tau
        prop[0, c, :, 1] = ssa
        for l in range(nstr):
            prop[0, c, :, 2 + l] = g ** (l + 1)
    bc = {"albedo": np.full((1, ncol), 0.2), "fbeam": np.ones((1, ncol)), "umu0": umu0}
    return prop, bc


def _planck_kw(ncol, nlyr):
    from oracle.disort_np import layer2level
    tl = np.linspace(290.0, 210.0, nlyr)[None, :] + np.arange(ncol)[:, None]
    return {"temf": layer2level(tl), "wave_lower": np.array([600.0]),
            "wave_upper": np.array([700.0])}


@pytest.mark.parametrize("planck", [False, True])
@pytest.mark.parametrize("nstr", [4, 8, 16])
def test_degenerate_couplings(oracle_c, nstr, planck):
    ncol, nlyr = 16, 4
    prop, bc = _degenerate_columns(nstr, ncol, nlyr)
    kw = {}
    if planck:
        kw = _planck_kw(ncol, nlyr)
        bc["btemp"] = np.full((1, ncol), 295.0)
    ref = oracle_c.forward(prop, bc, kw.get("temf"), nstr=nstr, planck=planck,
                           wave_lower=kw.get("wave_lower"), wave_upper=kw.get("wave_upper"))
    d = _disort(nstr, nlyr, 1, ncol, planck=planck, wl=kw.get("wave_lower"),
                wu=kw.get("wave_upper"))
    st = torch.zeros(ncol, dtype=torch.int32, device=torch.device("cuda", 0))
    f = _run(d, prop, bc, kw.get("temf"), status=st)
    assert np.isfinite(f).all()
    assert ((st.cpu().numpy() & 0x0F) == 0).all()
    err = rel_err(f, ref)
    print(f"nstr {nstr} planck {planck}: max rel err {err.max():.3e} "
          f"(column {int(err.max(axis=(0, 2, 3)).argmax())})")
    assert margin(err) < TOL
