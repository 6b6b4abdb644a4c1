"""The per-kernel timing of a context (hd_context_set_timing / hd_context_get_timing): one
timing quadruple -- layer kernel start / end, sweep start / end -- per chunk on every path
of the solve launcher: one chunk on the caller's stream and the multi-stream pipelines, on
the register path (nstr 8) and the team path (nstr 20), for forward, forward_flx and the
fused band sum."""

import math

import numpy as np
import pytest
import torch

from test_gpu_parity import _disort, _random_batch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
NWAVE, NCOL, NLYR = 3, 37, 12  # 111 solves


def _timed(chunk, call):
    """the context's timing totals of call() alone, under set_chunk(chunk)"""
    from pyharp_amd.disort import _context
    ctx = _context(0)
    try:
        ctx.set_chunk(chunk)
        ctx.set_timing(True)  # (re)starts the totals
        call()
        torch.cuda.synchronize()
        return ctx.timing()
    finally:
        ctx.set_chunk(0)
        ctx.set_timing(False)


def _check(t, chunk):
    want = 1 if chunk == 0 else math.ceil(NWAVE * NCOL / chunk)
    print(f"chunk {chunk}: layer {t.layer_launches} x, {t.layer_ms:.4f} ms; "
          f"sweep {t.sweep_launches} x, {t.sweep_ms:.4f} ms")
    assert t.layer_launches == want and t.sweep_launches == want
    assert math.isfinite(t.layer_ms) and t.layer_ms > 0
    assert math.isfinite(t.sweep_ms) and t.sweep_ms > 0


def _batch(nstr):
    rng = np.random.default_rng(4100 + nstr)
    prop, bc, _ = _random_batch(rng, NWAVE, NCOL, NLYR, nstr, False, beam=True)
    p = torch.as_tensor(prop, dtype=torch.float64, device=DEV)
    b = {k: torch.as_tensor(v, dtype=torch.float64, device=DEV) for k, v in bc.items()}
    return _disort(nstr, NLYR, NWAVE, NCOL), p, b, rng


@pytest.mark.parametrize("chunk", [0, 17])
@pytest.mark.parametrize("nstr", [8, 20])
@pytest.mark.parametrize("method", ["forward", "forward_flx"])
def test_one_quadruple_per_chunk(method, nstr, chunk):
    d, p, b, _ = _batch(nstr)
    _check(_timed(chunk, lambda: getattr(d, method)(p, b)), chunk)


@pytest.mark.parametrize("nstr", [8, 20])
def test_one_quadruple_per_chunk_band(nstr):
    d, p, b, rng = _batch(nstr)
    w = torch.as_tensor(rng.uniform(0.1, 1.0, NWAVE), dtype=torch.float64, device=DEV)
    _check(_timed(17, lambda: d.forward_band(p, b, weights=w)), 17)
