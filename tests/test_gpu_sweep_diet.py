"""The nstr <= 16 adding sweep and layer kernel after their instruction diet.

The sweep reads Ra through its upper triangle (no full copy), keeps M1 = Ra W1^-1 as the
symmetric matrix it is (upper triangle only, the row solves stopping at the diagonal) and
forms P = M1 T~ and Ra <- R~ + T~ P one column at a time (nstr > 8); the layer kernel takes
1 - exp(-k tau') from hd_m_expm1_neg (tests/test_expm1_cpu.py) and 1/k from the value it
already holds.  What that could break and no other test isolates:

* M1's symmetry is exact only in exact arithmetic: where W1 = I - R~ Ra is badly
  conditioned (thick, nearly conservative layers over a bright surface) the dropped half
  differed from the kept one by the most (test_w1_conditioning);
* the loop's first and last trips, and lanes at wave and chunk boundaries, are where a
  reordered load or store goes wrong (test_wave_and_chunk_boundaries, test_one_and_two_layers);
* the flx and spher sweeps instantiate the same body (test_flx_instantiation_flup_bitwise,
  test_spher_instantiation);
* k tau' from 1e-9 to 700 in one column walks the new helper's small-x, reduced and
  saturated ranges inside the kernel (test_operator_block_range).

Measured on one MI355X (profiles/sweepdiet/parity.txt), worst rel_err against the C oracle:
test_w1_conditioning 4.650e-10 / 1.303e-9 / 9.020e-10 at nstr 4 / 6 / 16, and the same three
figures with the parent's library on the same inputs (they are the oracle's own distance from
the 50-digit reference); test_operator_block_range 1.6e-10 / 1.7e-10 at nstr 4 / 16 (parent
3.0e-11 / 2.7e-10); test_one_and_two_layers at most 3.1e-10; test_spher_instantiation 4.7e-12.
"""

import functools

import numpy as np
import pytest
import torch

import spher_ref as S
from helpers import TOL, margin, rel_err
from test_gpu_parity import _disort, _run

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _hg(prop, g):
    for l in range(prop.shape[-1] - 2):
        prop[..., 2 + l] = g ** (l + 1)


def _chunked(chunk, fn):
    from pyharp_amd.disort import _context
    ctx = _context(0)
    ctx.set_chunk(chunk)
    try:
        return fn()
    finally:
        ctx.set_chunk(0)


# ------------------------------------------------------------------ conditioning of W1
UMU0 = (1.0, 0.6, 0.3, 0.85, 0.1, 0.45, 0.95, 0.2)
ALBEDO = (0.0, 1.0, 0.5, 1.0, 0.9, 0.0, 1.0, 0.3)


def conditioning_inputs(nstr):
    """nlyr 6, 8 columns of four kinds, cycled; HG moments; fbeam 1.  umu0 = 0.5 is kept
    out: it is a quadrature node at nstr 6."""
    nlyr, ncol = 6, 8
    kinds = (
        (np.full(nlyr, 20.0), np.full(nlyr, 0.999999), np.full(nlyr, 0.85)),
        (np.array([1e-5, 30.0, 1e-4, 50.0, 1e-3, 10.0]),
         np.array([0.999999, 0.99999, 0.5, 0.999999, 0.0, 0.9999]),
         np.array([0.9, 0.0, 0.5, 0.85, 0.0, 0.7])),
        (np.full(nlyr, 5.0), np.array([0.9999, 0.0] * 3), np.array([0.8, 0.0] * 3)),
        (10.0 ** np.linspace(-5.0, 1.5, nlyr), np.full(nlyr, 0.99999),
         np.linspace(0.0, 0.9, nlyr)),
    )
    prop = np.zeros((1, ncol, nlyr, 2 + nstr))
    for c in range(ncol):
        tau, ssa, g = kinds[c % 4]
        prop[0, c, :, 0] = tau
        prop[0, c, :, 1] = ssa
        _hg(prop[0, c], g)
    bc = {"umu0": np.array([UMU0]), "albedo": np.array([ALBEDO]), "fbeam": np.ones((1, ncol))}
    return prop, bc


@pytest.mark.parametrize("nstr", [4, 6, 16])
def test_w1_conditioning(oracle_c, nstr):
    """Against the C oracle, which on these inputs stands at most 1.3e-9 from
    oracle/disort_mp.py at 50 digits (nstr 4: 4.6e-10, 6: 1.3e-9, 16: 9.1e-10)."""
    prop, bc = conditioning_inputs(nstr)
    ref = oracle_c.forward(prop, bc, nstr=nstr)
    st = torch.zeros(prop.shape[1], dtype=torch.int32, device=DEV)
    f = _run(_disort(nstr, prop.shape[2], 1, prop.shape[1]), prop, bc, status=st)
    assert np.isfinite(f).all()
    assert ((st.cpu().numpy() & 0x0F) == 0).all()
    err = rel_err(f, ref)
    print(f"nstr {nstr}: max rel err {err.max():.3e} by column {err.max(axis=(0, 2, 3))}")
    assert margin(err) < TOL


# ------------------------------------------------------------------ wave and chunk boundaries
def _boundary_batch(ncol, nstr=16, nlyr=3):
    rng = np.random.default_rng(4100 + ncol)
    prop = np.zeros((1, ncol, nlyr, 2 + nstr))
    prop[..., 0] = 10.0 ** rng.uniform(-2.0, 0.7, (1, ncol, nlyr))
    prop[..., 1] = rng.uniform(0.1, 0.999, (1, ncol, nlyr))
    _hg(prop, rng.uniform(0.0, 0.85, (1, ncol, nlyr)))
    bc = {"umu0": rng.uniform(0.1, 1.0, (1, ncol)), "albedo": rng.uniform(0.0, 1.0, (1, ncol)),
          "fbeam": np.ones((1, ncol))}
    return prop, bc


@pytest.mark.parametrize("ncol", [65, 130])
def test_wave_and_chunk_boundaries(ncol):
    """One wave plus one lane, and two waves plus a partial third: as one chunk and in
    chunks of 64 the fluxes are the same bit for bit, and the solve in column 64 (lane 0
    of the second wave, or of the second chunk) equals the same solve placed in column 0."""
    nstr, nlyr = 16, 3
    prop, bc = _boundary_batch(ncol)
    d = _disort(nstr, nlyr, 1, ncol)
    whole = _run(d, prop, bc)
    parts = _chunked(64, lambda: _run(d, prop, bc))
    assert np.isfinite(whole).all()
    assert np.array_equal(whole, parts)
    moved = prop.copy()
    moved[0, 0] = prop[0, 64]
    bcm = {k: v.copy() for k, v in bc.items()}
    for v in bcm.values():
        v[0, 0] = v[0, 64]
    first = _run(d, moved, bcm)
    assert np.array_equal(first[0, 0], whole[0, 64])
    assert np.array_equal(first[0, 1:64], whole[0, 1:64])


# ------------------------------------------------------------------ first and last trips
@pytest.mark.parametrize("planck", [False, True])
@pytest.mark.parametrize("nstr", [4, 16])
@pytest.mark.parametrize("nlyr", [1, 2])
def test_one_and_two_layers(oracle_c, nlyr, nstr, planck):
    ncol = 4
    prop = np.zeros((1, ncol, nlyr, 2 + nstr))
    prop[..., 0] = np.array([0.7, 2.5])[:nlyr]
    prop[..., 1] = np.array([0.95, 0.6])[:nlyr]
    _hg(prop, np.broadcast_to(np.array([0.75, 0.3])[:nlyr], (1, ncol, nlyr)))
    bc = {"albedo": np.array([[0.0, 1.0, 0.0, 1.0]]), "fbeam": np.ones((1, ncol)),
          "umu0": np.array([[0.8, 0.8, 0.25, 0.25]])}
    kw = {}
    if planck:
        kw = {"temf": np.linspace(280.0, 240.0, nlyr + 1)[None, :] + np.arange(ncol)[:, None],
              "wave_lower": np.array([500.0]), "wave_upper": np.array([900.0])}
        bc["btemp"] = np.full((1, ncol), 290.0)
    ref = oracle_c.forward(prop, bc, kw.get("temf"), nstr=nstr, planck=planck,
                           wave_lower=kw.get("wave_lower"), wave_upper=kw.get("wave_upper"))
    d = _disort(nstr, nlyr, 1, ncol, planck=planck, wl=kw.get("wave_lower"),
                wu=kw.get("wave_upper"))
    st = torch.zeros(ncol, dtype=torch.int32, device=DEV)
    f = _run(d, prop, bc, kw.get("temf"), status=st)
    assert np.isfinite(f).all()
    assert ((st.cpu().numpy() & 0x0F) == 0).all()
    err = rel_err(f, ref)
    print(f"nlyr {nlyr} nstr {nstr} planck {planck}: max rel err {err.max():.3e}")
    assert margin(err) < TOL


# ------------------------------------------------------------------ flx and spher sweeps
def test_flx_instantiation_flup_bitwise():
    """hd_solve_flx's sweep shares the body: its flup is forward's, to the bit."""
    nstr, nlyr, ncol = 16, 3, 65
    prop, bc = _boundary_batch(ncol)
    d = _disort(nstr, nlyr, 1, ncol)
    flux = _run(d, prop, bc)
    p = torch.as_tensor(prop, dtype=torch.float64, device=DEV)
    b = {k: torch.as_tensor(v, dtype=torch.float64, device=DEV) for k, v in bc.items()}
    flx = d.forward_flx(p, b).cpu().numpy()
    assert np.isfinite(flx).all()
    assert np.array_equal(flx[..., 2], flux[..., 0])


@functools.lru_cache(maxsize=None)
def _spher_case():
    nstr, nlyr, ncol = 16, 3, 65
    prop, bc = _boundary_batch(ncol)
    zd = 2.0e4 * np.arange(nlyr + 1.0)
    ref, _, _ = S.spher_forward(prop, bc, None, zd=zd, radius=S.RADIUS, nstr=nstr)
    for a in (prop, zd, ref, *bc.values()):
        a.setflags(write=False)
    return prop, bc, zd, ref


def test_spher_instantiation():
    from test_gpu_spher import _disort as _spher_disort
    prop, bc, zd, ref = _spher_case()
    d = _spher_disort(16, prop.shape[2], 1, prop.shape[1])
    t = lambda x: torch.tensor(np.array(x), dtype=torch.float64, device=DEV)  # noqa: E731
    st = torch.zeros(prop.shape[1], dtype=torch.int32, device=DEV)
    f = d.forward(t(prop), {k: t(v) for k, v in bc.items()}, None, zd=t(zd),
                  status=st).cpu().numpy()
    assert not (st.cpu().numpy() & 0x0F).any()
    err = rel_err(f, ref)
    print(f"spher nstr 16: max rel err {err.max():.3e}")
    assert margin(err) < TOL


# ------------------------------------------------------------------ the operator block
@pytest.mark.parametrize("nstr", [4, 16])
def test_operator_block_range(oracle_c, nstr):
    """One column whose layers run from tau = 1e-10 to 300 at omega = 0.5: k tau' from
    ~1e-9 (below the kernel's 1e-8 guard) through the series' n = 0 range and the reduced
    range to past 700, where 1 - exp(-k tau') is 1 to the last bit."""
    tau = np.array([1e-10, 1e-9, 1e-8, 1e-6, 1e-3, 0.05, 0.4, 3.0, 30.0, 300.0])
    nlyr, ncol = len(tau), 2
    prop = np.zeros((1, ncol, nlyr, 2 + nstr))
    prop[0, 0, :, 0] = tau
    prop[0, 1, :, 0] = tau[::-1]
    prop[..., 1] = 0.5
    _hg(prop, np.full((1, ncol, nlyr), 0.5))
    bc = {"umu0": np.full((1, ncol), 0.6), "albedo": np.full((1, ncol), 0.3),
          "fbeam": np.ones((1, ncol))}
    ref = oracle_c.forward(prop, bc, nstr=nstr)
    st = torch.zeros(ncol, dtype=torch.int32, device=DEV)
    f = _run(_disort(nstr, nlyr, 1, ncol), prop, bc, status=st)
    assert np.isfinite(f).all()
    assert ((st.cpu().numpy() & 0x0F) == 0).all()
    err = rel_err(f, ref)
    print(f"nstr {nstr}: max rel err {err.max():.3e} by column {err.max(axis=(0, 2, 3))}")
    assert margin(err) < TOL
