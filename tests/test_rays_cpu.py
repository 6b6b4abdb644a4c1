"""The host side of the ray radiances, without a GPU: harp's `outdirs` string
(pyharp_amd.parse_radiation_directions) and the argument checks of
Disort.forward_rays / forward_rays_band that fire before the library is touched."""

import math

import pytest
import torch


def test_parse_radiation_directions():
    from pyharp_amd import parse_radiation_directions
    mu, phi = parse_radiation_directions("(0,0)")
    assert mu.dtype == phi.dtype == torch.float64
    assert mu.tolist() == [1.0] and phi.tolist() == [0.0]
    mu, phi = parse_radiation_directions("(60,90) (120,270)")
    assert mu.dtype == phi.dtype == torch.float64 and mu.shape == phi.shape == (2,)
    assert mu.tolist() == pytest.approx([0.5, -0.5], abs=1e-15)
    assert phi.tolist() == [90.0, 270.0]  # degrees, as cdisort takes them
    # the format's whitespace: between pairs and around the numbers
    mu, phi = parse_radiation_directions("  ( 30 , 45.5 )\t(1e1,-20)\n")
    assert mu.tolist() == pytest.approx([math.cos(math.radians(30)), math.cos(math.radians(10))],
                                        abs=1e-15)
    assert phi.tolist() == [45.5, -20.0]


@pytest.mark.parametrize("bad", ["", "   ", "60,90", "(60,90", "(60;90)", "(60,90) x", "(a,b)",
                                 "(60,90,1)", "(60)", "(60,90)(", "(nan,0)", "(0,inf)"])
def test_parse_radiation_directions_malformed(bad):
    from pyharp_amd import parse_radiation_directions
    with pytest.raises(ValueError, match="parse_radiation_directions"):
        parse_radiation_directions(bad)


def test_parse_radiation_directions_needs_a_string():
    from pyharp_amd import parse_radiation_directions
    with pytest.raises(ValueError):
        parse_radiation_directions([(0, 0)])


def _module(flags="lamber,quiet", nlyr=3, nstr=4, nwave=2, ncol=3):
    from pyharp_amd import Disort, DisortOptions
    op = DisortOptions().flags(flags).nwave(nwave).ncol(ncol)
    op.ds().nlyr, op.ds().nstr, op.ds().nmom = nlyr, nstr, nstr
    return Disort(op)


def test_forward_rays_python_level_errors():
    """shape, dtype and flag errors are raised before a device or the library is needed"""
    d = _module()
    prop = torch.zeros((2, 3, 3, 6), dtype=torch.float64)
    mu = torch.tensor([0.5, -0.5], dtype=torch.float64)
    ph = torch.tensor([0.0, 90.0], dtype=torch.float64)
    with pytest.raises(RuntimeError, match="float64"):
        d.forward_rays(prop, umu=mu.float(), phi=ph)
    with pytest.raises(RuntimeError, match="float64"):
        d.forward_rays(prop, umu=mu, phi=ph.float())
    with pytest.raises(RuntimeError, match="float64"):
        d.forward_rays(prop, umu=[0.5, -0.5], phi=ph)
    with pytest.raises(RuntimeError, match="umu must be"):  # (ncol, nray) with another ncol
        d.forward_rays(prop, umu=mu.expand(2, 2).contiguous(), phi=ph.expand(2, 2).contiguous())
    with pytest.raises(RuntimeError, match="umu must be"):
        d.forward_rays(prop, umu=mu.reshape(1, 1, 2), phi=ph.reshape(1, 1, 2))
    with pytest.raises(RuntimeError, match="umu must be"):
        d.forward_rays(prop, umu=mu[:0], phi=ph[:0])
    with pytest.raises(RuntimeError, match="must have umu's shape"):
        d.forward_rays(prop, umu=mu, phi=ph[:1])
    with pytest.raises(RuntimeError, match="prop must be"):
        d.forward_rays(prop[0], umu=mu, phi=ph)
    with pytest.raises(RuntimeError, match="weights for 2 waves"):
        d.forward_rays_band(prop, umu=mu, phi=ph, weights=torch.ones(3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="onlyfl"):
        _module("lamber,onlyfl").forward_rays(prop, umu=mu, phi=ph)
    with pytest.raises(RuntimeError, match="onlyfl"):
        _module("lamber,onlyfl").forward_rays_band(prop, umu=mu, phi=ph, weights=torch.ones(2))


def test_forward_rays_checks_the_batch_like_forward():
    d = _module()
    mu = torch.tensor([0.5], dtype=torch.float64)
    with pytest.raises(RuntimeError, match="layers"):
        d.forward_rays(torch.zeros((2, 3, 4, 6), dtype=torch.float64), umu=mu, phi=mu)
    with pytest.raises(RuntimeError, match="unknown boundary condition"):
        d.forward_rays(torch.zeros((2, 3, 3, 6), dtype=torch.float64), {"nope": mu}, umu=mu, phi=mu)
