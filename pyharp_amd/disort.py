"""Drop-in DISORT flux module (pydisort ``disort::Disort`` contract) on MI355X.

Mirrors the API pyharp uses at its call sites
(``examples/amars_sw.cpp:43-65,216,280``, ``examples/amars_lw.cpp:18-38,60,80``,
``tests/test_disort.cpp:13-55``, ``src/radiation/radiation_band.cpp:57-69,123-128``)::

    op = DisortOptions().header("...").flags("lamber,quiet,onlyfl")
    op.nwave(500).ncol(1)
    op.ds().nlyr = 40; op.ds().nstr = 8; op.ds().nmom = 8
    disort = Disort(op)
    flux = disort.forward(prop, bc)            # or forward(prop, bc, temf)

``prop`` (nwave, ncol, nlyr, nprop) f64, layer 0 = bottom; ``bc`` dict of
(nwave, ncol) tensors; ``temf`` (ncol, nlyr+1) level temperatures bottom->top.
Returns ``flux`` (nwave, ncol, nlyr+1, 2): level 0 = surface, [...,0] upward,
[...,1] downward (rfldir + rfldn).  CPU tensors are staged through the GPU and
the result is returned on the input's device; CUDA tensors stay on device.

Intensity path (``tests/test_disort.cpp:13-55``): without ``onlyfl`` the module
also computes radiances -- at ``user_mu`` x ``user_phi`` with ``usrang``, else at
the quadrature cosines and ``user_phi`` (default [0]) -- at ``user_tau`` with
``usrtau`` (else at the level depths); ``get_rad()`` returns them as
(nwave, ncol, nphi, ntau, numu).  With ``usrtau`` the fluxes are at the user
depths, (nwave, ncol, ntau, 2), index 0 = the deepest.  Every nstr 2..32.

The arithmetic runs in libhdisort.so (HIP, gfx950) through the C-ABI in
include/hdisort.h.  There is no CPU fallback: without a HIP device or without
the built library, ``forward`` raises.
"""

from __future__ import annotations

import math
import re
import threading
from typing import Dict, Optional

import torch

from . import _lib
from .index import IEX, ISS, IPM  # noqa: F401  (re-exported like disort::index)
from .index import NFLX
from .rtsolver import RTSolver

# cdisort's disort_flag fields as pydisort's flag string names them (the Disort-flags
# block of examples/amarsw-ck.yaml:74-90, tests/test_disort.cpp:16-18)
_KNOWN_FLAGS = {
    "lamber", "quiet", "onlyfl", "planck", "usrtau", "usrang", "intensity_correction",
    "old_intensity_correction", "print-input", "print-fluxes", "print-intensity",
    "print-transmissivity", "print-phase-function", "ibcnd", "spher", "general_source",
    "output_uum",
}
# cdisort flags this solver does not implement: rejected, never silently ignored
# (spher: honoured by Disort.reset with a configured radius, onlyfl and no usrtau)
_UNSUPPORTED_FLAGS = {
    "general_source": "general (user-supplied) sources are not implemented",
    "output_uum": "per-mode intensities (uum) are not output",
}


def check_flags(flags: set) -> None:
    """The flag semantics of the boundary, shared by reset():
    unknown names raise; ``ibcnd`` raises as harp's DISORT driver does
    (rt_solver_disort.cpp_:67-68, ``ValueError("RTSolverDisort::CalRadtranFlux",
    "ibcnd", ds_.flag.ibcnd, 0)``: the albedo/transmissivity mode of cdisort is not
    harp's); cdisort's new (Buras-Emde-Dowling) intensity correction --
    ``intensity_correction`` without ``old_intensity_correction`` -- raises when
    radiances are requested (with ``onlyfl`` cdisort applies no correction, so the
    flag has no effect there, as in examples/amarsw-ck.yaml:79-82).  ``spher`` is checked
    by ``Disort.reset`` (it needs ``DisortOptions.radius``)."""
    unknown = flags - _KNOWN_FLAGS
    if unknown:
        raise RuntimeError(f"Disort: unknown flags {sorted(unknown)}")
    if "ibcnd" in flags:
        raise RuntimeError("RTSolverDisort::CalRadtranFlux: ibcnd = 1, expected 0 (the "
                           "special-case albedo/transmissivity mode is not supported)")
    for f in sorted(flags & set(_UNSUPPORTED_FLAGS)):
        raise RuntimeError(f"Disort: flag '{f}': {_UNSUPPORTED_FLAGS[f]}")
    if ("intensity_correction" in flags and "old_intensity_correction" not in flags
            and "onlyfl" not in flags):
        raise RuntimeError("Disort: intensity_correction without old_intensity_correction "
                           "selects cdisort's new (Buras-Emde-Dowling) correction, which is "
                           "not implemented; add old_intensity_correction for the "
                           "Nakajima-Tanaka correction (TMS + IMS) or use onlyfl")
_BC_KEYS = ("fbeam", "umu0", "albedo", "btemp", "ttemp", "temis", "fisot")
_BC_IGNORED = ("phi0",)  # azimuth of the beam: used by the radiances only


def night_side_beam(bc: Dict[str, torch.Tensor], mode: str = "dark",
                    umu0_min: float = 1.0e-3) -> Dict[str, torch.Tensor]:
    """Boundary conditions a GCM-style caller can pass for a whole globe.

    The solver takes umu0 as given, as pydisort's forward hands it to cdisort, whose
    input check (c_chekin) rejects a beam (fbeam > 0) with umu0 outside (0, 1]: such a
    solve is flagged HD_STATUS_BAD_INPUT and a synchronous call fails.  A caller that
    passes one fbeam with cos(zenith) over day and night side picks a convention here:

      mode="dark"  -- fbeam = 0 where umu0 <= 0 (no direct beam on the night side;
                      umu0 there is then not read);
      mode="clamp" -- umu0 = max(umu0, umu0_min) where fbeam > 0 (harp's legacy driver
                      floored umu0 at 1e-3 before calling cdisort,
                      src/rtsolver/rt_solver_disort.cpp_:80).

    Returns a new dict (the caller's tensors are not modified); umu0 > 1 stays an
    error in both modes."""
    if mode not in ("dark", "clamp"):
        raise ValueError(f"night_side_beam: mode must be 'dark' or 'clamp', got {mode!r}")
    out = dict(bc)
    if "fbeam" not in bc or "umu0" not in bc or bc["fbeam"] is None or bc["umu0"] is None:
        return out
    fb = torch.as_tensor(bc["fbeam"])
    mu = torch.as_tensor(bc["umu0"])
    if mode == "dark":
        fb, mu = torch.broadcast_tensors(fb, mu)
        out["fbeam"] = torch.where(mu > 0.0, fb, torch.zeros_like(fb))
    else:
        fb, mu = torch.broadcast_tensors(fb, mu)
        out["umu0"] = torch.where(fb > 0.0, torch.clamp(mu, min=umu0_min), mu)
    return out


_DIRECTION = re.compile(r"\(\s*([^\s,()]+)\s*,\s*([^\s,()]+)\s*\)")


def parse_radiation_directions(s: str):
    """harp's ``outdirs`` string, ``"(zenith,azimuth) (zenith,azimuth) ..."`` with both
    angles in degrees (RadiationOptions / RadiationBandOptions, src/radiation/
    radiation.hpp:31, radiation_band.hpp:30), as the ``umu`` / ``phi`` arguments of
    ``Disort.forward_rays``: two float64 tensors (nray,), ``mu = cos(zenith)`` and the
    azimuth in DEGREES.  The reference's parser returns one float32 (nray, 2) tensor
    with the azimuth converted to radians; cdisort and this library take phi in
    degrees, and float32 would cost the cosine its last nine digits.  A string that is
    not a whitespace-separated list of ``(number,number)`` pairs raises ValueError."""
    if not isinstance(s, str):
        raise ValueError(f"parse_radiation_directions: expected a string, got {type(s).__name__}")
    pairs = _DIRECTION.findall(s)
    if not pairs or _DIRECTION.sub("", s).strip():
        raise ValueError(f"parse_radiation_directions: {s!r} is not a list of "
                         "'(zenith,azimuth)' pairs")
    try:
        zen = [float(a) for a, _ in pairs]
        azi = [float(b) for _, b in pairs]
    except ValueError:
        raise ValueError(f"parse_radiation_directions: {s!r} holds a pair that is not two "
                         "numbers") from None
    if not all(math.isfinite(v) for v in zen + azi):
        raise ValueError(f"parse_radiation_directions: {s!r} holds a non-finite angle")
    mu = torch.tensor([math.cos(math.radians(z)) for z in zen], dtype=torch.float64)
    return mu, torch.tensor(azi, dtype=torch.float64)


def _beam_hint(bc) -> str:
    """After a failed synchronous call: name the beam inputs cdisort's c_chekin rejects."""
    try:
        if not bc or bc.get("fbeam") is None or bc.get("umu0") is None:
            return ""
        fb, mu = torch.broadcast_tensors(torch.as_tensor(bc["fbeam"]), torch.as_tensor(bc["umu0"]))
        bad = int(((fb > 0.0) & ~((mu > 0.0) & (mu <= 1.0))).sum())
    except Exception:  # the hint must never mask the original error
        return ""
    if not bad:
        return ""
    return (f" -- {bad} solve(s) have fbeam > 0 with umu0 outside (0, 1], which cdisort's "
            "c_chekin rejects; for a day/night batch use "
            "pyharp_amd.night_side_beam(bc, mode='dark' or 'clamp')")


class _DisortState:
    """Subset of cdisort's disort_state exposed by ``DisortOptions.ds()``."""

    def __init__(self):
        self.nlyr = 1
        self.nstr = 4
        self.nmom = 4
        self.nphi = 0
        self.ntau = 0
        self.numu = 0
        self.utau = []

    def __repr__(self):
        return (f"disort_state(nlyr={self.nlyr}, nstr={self.nstr}, nmom={self.nmom}, "
                f"nphi={self.nphi}, ntau={self.ntau}, numu={self.numu})")


def _arg(name, default):
    """harp ADD_ARG idiom: obj.name(value) sets and returns obj; obj.name() reads."""

    def accessor(self, *value):
        if value:
            setattr(self, "_" + name, value[0])
            return self
        return getattr(self, "_" + name, default() if callable(default) else default)

    accessor.__name__ = name
    return accessor


class DisortOptions:
    header = _arg("header", "")
    flags = _arg("flags", "")
    nwave = _arg("nwave", 1)
    ncol = _arg("ncol", 1)
    wave_lower = _arg("wave_lower", list)
    wave_upper = _arg("wave_upper", list)
    user_tau = _arg("user_tau", list)
    user_mu = _arg("user_mu", list)
    user_phi = _arg("user_phi", list)
    device = _arg("device", 0)
    # planet radius for the 'spher' flag (pseudo-spherical beam), in the unit of the level
    # altitudes ``zd`` passed to forward; unused without the flag, as in cdisort
    radius = _arg("radius", 0.0)

    def __init__(self):
        self._ds = _DisortState()

    def ds(self) -> _DisortState:
        return self._ds

    def flag_set(self) -> set:
        return {f.strip() for f in self.flags().split(",") if f.strip()}

    def __repr__(self):
        return (f"DisortOptions(flags='{self.flags()}', nwave={self.nwave()}, "
                f"ncol={self.ncol()}, ds={self._ds})")


_THREAD = threading.local()


def _context(device: int) -> _lib.Context:
    """The calling host thread's hd_context on ``device`` (SURVEY 8(b) "Threading":
    one context per (device, host thread)).  Modules of one thread share it; the
    library orders their solves on any streams behind each other (hd_solve waits
    for the context's previous solve), so scratch is never used twice at once."""
    ctxs = getattr(_THREAD, "contexts", None)
    if ctxs is None:
        ctxs = _THREAD.contexts = {}
    ctx = ctxs.get(device)
    if ctx is None:
        ctx = _lib.Context(device)
        ctxs[device] = ctx
    return ctx


class Disort(RTSolver):
    """MI355X flux-only DISORT module (drop-in for pydisort's DisortImpl)."""

    def __init__(self, options: Optional[DisortOptions] = None):
        self.options = options if options is not None else DisortOptions()
        self._waves = None
        self.reset()

    def reset(self):
        op = self.options
        flags = op.flag_set()
        check_flags(flags)
        ds = op.ds()
        if ds.nstr < 2 or ds.nstr % 2 or ds.nstr > 32:
            raise RuntimeError(f"Disort: nstr={ds.nstr} must be even and in [2, 32]")
        if ds.nlyr < 1:
            raise RuntimeError(f"Disort: nlyr={ds.nlyr} must be >= 1")
        if "lamber" not in flags:
            raise RuntimeError("Disort: only Lambertian lower boundaries are supported "
                               "(set the 'lamber' flag)")
        self.planck = "planck" in flags
        if self.planck:
            if len(op.wave_lower()) != op.nwave() or len(op.wave_upper()) != op.nwave():
                raise RuntimeError("Disort: planck needs wave_lower/wave_upper of size nwave")
        # intensity path: radiances (onlyfl off) and/or fluxes at user depths
        self.onlyfl = "onlyfl" in flags
        self.usrtau = "usrtau" in flags
        self.usrang = "usrang" in flags
        self.radiance = (not self.onlyfl) or self.usrtau
        # pseudo-spherical beam geometry: the flux paths only
        self.spher = "spher" in flags
        if self.spher:
            r = float(op.radius())
            if not (math.isfinite(r) and r > 0.0):
                raise RuntimeError("Disort: flag 'spher': pseudo-spherical geometry needs "
                                   "DisortOptions.radius (finite, > 0)")
            if self.radiance:
                raise RuntimeError("Disort: flag 'spher': pseudo-spherical radiances are not "
                                   "implemented (set 'onlyfl', clear 'usrtau')")
        # Nakajima-Tanaka correction, TMS + IMS: cdisort applies it with both
        # intensity_correction and old_intensity_correction; old_intensity_correction
        # alone applies none (check_flags refuses the new method)
        self.corint = {"intensity_correction", "old_intensity_correction"} <= flags
        self._rad = None
        if self.radiance:
            if self.usrtau:
                ut = [float(x) for x in op.user_tau()]
                if not ut:
                    raise RuntimeError("Disort: usrtau set but user_tau is empty")
                if any(x < 0 for x in ut) or any(b < a for a, b in zip(ut, ut[1:])):
                    raise RuntimeError("Disort: user_tau must be >= 0 and ascending")
                ds.utau = ut
                ds.ntau = len(ut)
            else:
                ds.utau = []
                ds.ntau = ds.nlyr + 1
            if self.usrang:
                umu = [float(x) for x in op.user_mu()]
                if not umu or any(x == 0 or abs(x) > 1 for x in umu):
                    raise RuntimeError("Disort: usrang needs user_mu in [-1,0)U(0,1]")
            else:
                mu, _ = _lib.quadrature(ds.nstr) if _lib_loaded() else _gauss(ds.nstr)
                umu = [-x for x in reversed(mu)] + list(mu)
            phi = [float(x) for x in op.user_phi()] or [0.0]
            self._umu, self._phi = umu, phi
            ds.numu, ds.nphi = (len(umu), len(phi)) if not self.onlyfl else (0, 0)

    def ds(self):
        return self.options.ds()

    def get_rad(self, *args, **kwargs) -> torch.Tensor:
        """Radiances of the last forward, (nwave, ncol, nphi, ntau, numu)
        (pydisort DisortImpl::get_rad, tests/test_disort.cpp:52)."""
        if self.onlyfl:
            raise RuntimeError("Disort.get_rad: radiances are off (onlyfl flag)")
        if self._rad is None:
            raise RuntimeError("Disort.get_rad: call forward first")
        return self._rad

    # ------------------------------------------------------------------ #
    def forward(self, prop: torch.Tensor, bc: Optional[Dict[str, torch.Tensor]] = None,
                temf: Optional[torch.Tensor] = None, *, status: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None,
                zd: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``zd`` (with the 'spher' flag, and only then): the level altitudes above
        ``DisortOptions.radius``, bottom -> top, a float64 device tensor (nlyr+1,) shared by
        all columns or (ncol, nlyr+1) -- harp's ``x1f`` minus the planet radius."""
        try:
            return self._forward(prop, bc, temf, status=status, out=out, zd=zd)
        except RuntimeError as err:
            if "at least one solve failed" in str(err) and _beam_hint(bc):
                raise RuntimeError(str(err) + _beam_hint(bc)) from err
            raise

    def forward_band(self, prop: torch.Tensor, bc: Optional[Dict[str, torch.Tensor]] = None,
                     temf: Optional[torch.Tensor] = None, *, weights: torch.Tensor,
                     out: Optional[torch.Tensor] = None, flux: Optional[torch.Tensor] = None,
                     status: Optional[torch.Tensor] = None,
                     zd: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The band flux (ncol, nlyr+1, 2) = sum_w weights[w] F_w of this batch, with
        the sum fused into the solve (hd_solve_band): what every harp caller does
        with forward's result next (examples/amars_lw.cpp:84-88
        ``(flux * weights.view({-1,1,1,1})).sum(0)``; amars_sw.cpp:169-196 with
        weights = d(wavenumber)).  Per-point fluxes are stored only if ``flux``
        (nwave, ncol, nlyr+1, 2) is given.  Fixed summation order, no atomics.  ``zd``: as
        ``forward`` (the 'spher' flag)."""
        if self.radiance:
            raise RuntimeError("Disort.forward_band: the fused band sum is a flux-only path "
                               "(onlyfl without usrtau)")
        try:
            return self._forward(prop, bc, temf, status=status, out=flux, band=(weights, out),
                                 zd=zd)
        except RuntimeError as err:
            if "at least one solve failed" in str(err) and _beam_hint(bc):
                raise RuntimeError(str(err) + _beam_hint(bc)) from err
            raise

    def forward_flx(self, prop: torch.Tensor, bc: Optional[Dict[str, torch.Tensor]] = None,
                    temf: Optional[torch.Tensor] = None, *,
                    status: Optional[torch.Tensor] = None,
                    out: Optional[torch.Tensor] = None,
                    zd: Optional[torch.Tensor] = None) -> torch.Tensor:
        """DISORT's full flux record at every level, (nwave, ncol, nlyr+1, NFLX) in the
        component order of cdisort's disort_radiant (index.IRFLDIR .. IUAVGSO): direct
        beam, diffuse down, up, flux divergence dF/dtau, mean intensity and its down /
        up / direct-beam parts (hd_solve_flx; definitions in include/hdisort.h).  Level
        0 is the surface.  On the input's device: CPU tensors are staged with torch
        copies and the record comes back on the CPU.  ``zd``: as ``forward`` (the 'spher'
        flag; rfldir then on the unscaled slant depth, uavgso on the scaled one)."""
        if self.usrtau:
            raise RuntimeError("Disort.forward_flx: the flux record is at the layer boundaries "
                               "(clear the 'usrtau' flag)")
        if not self.onlyfl:
            raise RuntimeError("Disort.forward_flx: a flux-only path (set the 'onlyfl' flag)")
        try:
            return self._forward(prop, bc, temf, status=status, out=out, flx=True, zd=zd)
        except RuntimeError as err:
            if "at least one solve failed" in str(err) and _beam_hint(bc):
                raise RuntimeError(str(err) + _beam_hint(bc)) from err
            raise

    def forward_rays(self, prop: torch.Tensor, bc: Optional[Dict[str, torch.Tensor]] = None,
                     temf: Optional[torch.Tensor] = None, *, umu: torch.Tensor,
                     phi: torch.Tensor, out: Optional[torch.Tensor] = None,
                     flux: Optional[torch.Tensor] = None,
                     status: Optional[torch.Tensor] = None,
                     zd: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Radiances (nwave, ncol, ntau, nray) along nray paired outgoing directions
        (hd_solve_rays): ``umu`` / ``phi`` are float64 tensors (nray,) -- shared by every
        column -- or (ncol, nray) -- each column's own rays; umu the polar cosine
        (nonzero, > 0 upward), phi the azimuth in DEGREES.  This is harp's ``outdirs``
        list (``parse_radiation_directions``) evaluated exactly at every ray, where the
        legacy driver interpolated a grid solve (rt_solver_disort.cpp_:210-286).  Needs a
        module without ``onlyfl``; depths are ``user_tau`` with ``usrtau``, else the
        layer boundaries; the intensity correction follows the flags; the options'
        ``user_mu`` / ``user_phi`` are not used.  ``flux`` (nwave, ncol, ntau, 2), if
        given, receives the fluxes at those depths.  CPU inputs (prop, bc, temf, umu, phi)
        are staged with torch copies and the result comes back on the CPU; caller-supplied
        ``out`` / ``flux`` / ``status`` buffers are written by the device and must be on the
        solve device (``cuda:<options.device()>`` for CPU inputs), as for ``forward``.  A ray with umu = 0, |umu| > 1 or
        a non-finite umu fails its column's solves (HD_STATUS_BAD_INPUT) and is NaN.

        ``zd`` given: the pseudo-spherical beam (hd_solve_rays_spher)
        with ``DisortOptions.radius`` as the planet radius -- the level altitudes above it,
        bottom -> top, a float64 tensor (nlyr+1,) shared by all columns or (ncol, nlyr+1),
        staged to the solve device like ``umu``.  nstr <= 16.  The 'spher' flag is not
        needed (and cannot be set on a module with radiances); without ``zd`` the call is
        the plane-parallel one.  A column whose zd is not finite or not strictly increasing
        fails its solves (HD_STATUS_BAD_INPUT), which run with the beam off.  ``flux`` at the
        layer boundaries (no ``usrtau``) is then the flux solve's own output, bitwise
        ``forward(zd=)`` of an 'onlyfl,spher' module on the same inputs."""
        try:
            return self._forward_rays(prop, bc, temf, umu, phi, out, flux, status, None, zd)
        except RuntimeError as err:
            if "at least one solve failed" in str(err) and _beam_hint(bc):
                raise RuntimeError(str(err) + _beam_hint(bc)) from err
            raise

    def forward_rays_band(self, prop: torch.Tensor,
                          bc: Optional[Dict[str, torch.Tensor]] = None,
                          temf: Optional[torch.Tensor] = None, *, umu: torch.Tensor,
                          phi: torch.Tensor, weights: torch.Tensor,
                          out: Optional[torch.Tensor] = None,
                          rad: Optional[torch.Tensor] = None,
                          flux: Optional[torch.Tensor] = None,
                          status: Optional[torch.Tensor] = None,
                          zd: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The band radiance (ncol, ntau, nray) = sum_w weights[w] rad_w of
        ``forward_rays``, with the sum fused into the solve (the legacy driver's
        ``btoa(n) += wght[b] * toa(b, n)``).  Per-wave radiances are stored only if
        ``rad`` (nwave, ncol, ntau, nray) is given.  One fma per wave in wave order, no
        atomics: bitwise equal to ``spectral.band_rad(forward_rays(...), weights)``.
        ``zd``: as ``forward_rays`` (the pseudo-spherical beam)."""
        try:
            return self._forward_rays(prop, bc, temf, umu, phi, rad, flux, status,
                                      (weights, out), zd)
        except RuntimeError as err:
            if "at least one solve failed" in str(err) and _beam_hint(bc):
                raise RuntimeError(str(err) + _beam_hint(bc)) from err
            raise

    def _forward_rays(self, prop, bc, temf, umu, phi, rad, flux, status, band, zd=None):
        import ctypes
        who = "Disort.forward_rays" + ("_band" if band is not None else "")
        ds = self.options.ds()
        f64 = torch.float64
        if self.onlyfl:
            raise RuntimeError(f"{who}: radiances are off (clear the 'onlyfl' flag)")
        if prop.dim() != 4:
            raise RuntimeError(f"{who}: prop must be (nwave, ncol, nlyr, nprop), got "
                               f"{tuple(prop.shape)}")
        nwave, ncol = prop.shape[0], prop.shape[1]
        if zd is not None:  # the pseudo-spherical beam: checked before the device is touched
            r = float(self.options.radius())
            if not (math.isfinite(r) and r > 0.0):
                raise RuntimeError(f"{who}: zd given: pseudo-spherical geometry needs "
                                   "DisortOptions.radius (finite, > 0)")
            if not isinstance(zd, torch.Tensor) or zd.dtype != f64:
                raise RuntimeError(f"{who}: zd must be a float64 tensor")
            if zd.dim() not in (1, 2) or zd.shape[-1] != ds.nlyr + 1 or \
                    (zd.dim() == 2 and zd.shape[0] != ncol):
                raise RuntimeError(f"{who}: zd must be (nlyr+1,) or (ncol, nlyr+1) = "
                                   f"({ncol}, {ds.nlyr + 1}), got {tuple(zd.shape)}")
            if ds.nstr > 16:
                raise RuntimeError(f"{who}: zd given: pseudo-spherical ray radiances support "
                                   f"nstr <= 16, got nstr={ds.nstr}")
        for name, t in (("umu", umu), ("phi", phi)):
            if not isinstance(t, torch.Tensor) or t.dtype != f64:
                raise RuntimeError(f"{who}: {name} must be a float64 tensor")
        if umu.dim() not in (1, 2) or umu.shape[-1] < 1 or \
                (umu.dim() == 2 and umu.shape[0] != ncol):
            raise RuntimeError(f"{who}: umu must be (nray,) or (ncol, nray) = ({ncol}, nray), "
                               f"got {tuple(umu.shape)}")
        if phi.shape != umu.shape:
            raise RuntimeError(f"{who}: phi {tuple(phi.shape)} must have umu's shape "
                               f"{tuple(umu.shape)}")
        if phi.device != umu.device:
            raise RuntimeError(f"{who}: umu and phi must be on one device")
        nray = umu.shape[-1]
        if band is not None:
            wts = torch.as_tensor(band[0], dtype=f64).reshape(-1)
            if wts.numel() != nwave:
                raise RuntimeError(f"{who}: {wts.numel()} weights for {nwave} waves")
        bc = {} if bc is None else bc
        nwave, ncol, nlyr, nprop, in_dev, dev = self._check_inputs(prop, bc, temf)
        cfg, inp, keep = self._stage(prop, bc, temf, dev)
        ntau = ds.ntau

        def given(t, shape, name):
            if t is not None and (t.device != dev or t.dtype != f64 or not t.is_contiguous()
                                  or tuple(t.shape) != shape):
                raise RuntimeError(f"{who}: {name} must be a contiguous float64 tensor of "
                                   f"shape {shape} on {dev}")
            return t

        rshape = (nwave, ncol, ntau, nray)
        given(rad, rshape, "rad" if band is not None else "out")
        given(flux, (nwave, ncol, ntau, 2), "flux")
        if status is not None and (status.device != dev or status.dtype != torch.int32
                                   or not status.is_contiguous()
                                   or status.numel() < nwave * ncol):
            raise RuntimeError(f"{who}: status must be a contiguous int32 tensor of "
                               f">= {nwave * ncol} elements on {dev}")
        brad = None
        if band is not None:
            brad = given(band[1], (ncol, ntau, nray), "out")
            if brad is None:
                brad = torch.empty((ncol, ntau, nray), dtype=f64, device=dev)
            wts = wts.to(dev).contiguous()
            keep.append(wts)
        elif rad is None:
            rad = torch.empty(rshape, dtype=f64, device=dev)
        mu_d, ph_d = umu.to(dev).contiguous(), phi.to(dev).contiguous()
        keep += [mu_d, ph_d]
        phi0 = None
        if bc.get("phi0") is not None:
            phi0 = torch.as_tensor(bc["phi0"], dtype=f64).expand((nwave, ncol)).to(dev)
            phi0 = phi0.contiguous()
            keep.append(phi0)
        ut = (ctypes.c_double * max(1, len(ds.utau)))(*ds.utau)
        rays = _lib.HdRays(nray=nray, per_column=int(umu.dim() == 2), umu=mu_d.data_ptr(),
                           phi=ph_d.data_ptr(), ntau=len(ds.utau) if self.usrtau else 0,
                           utau=ctypes.cast(ut, ctypes.c_void_p),
                           phi0=phi0.data_ptr() if phi0 is not None else None,
                           corint=int(self.corint),
                           weight=wts.data_ptr() if band is not None else None,
                           brad=brad.data_ptr() if brad is not None else None)
        stream = torch.cuda.current_stream(dev)
        ptrs = (flux.data_ptr() if flux is not None else None,
                rad.data_ptr() if rad is not None else None,
                status.data_ptr() if status is not None else None, stream.cuda_stream)
        with torch.cuda.device(dev):
            if zd is not None:
                z_d = zd.to(dev).contiguous()
                keep.append(z_d)
                sph = _lib.HdSphere(radius=float(self.options.radius()), zd=z_d.data_ptr(),
                                    per_column=int(z_d.dim() == 2))
                _context(dev.index).solve_rays_spher(cfg, inp, sph, rays, *ptrs)
            else:
                _context(dev.index).solve_rays(cfg, inp, rays, *ptrs)
        del keep
        res = brad if band is not None else rad
        return res.to(in_dev) if in_dev.type != "cuda" else res

    def _check_inputs(self, prop, bc, temf):
        """The shape and option checks every forward_* shares, before anything is staged;
        returns (nwave, ncol, nlyr, nprop, the input's device, the solve's device)."""
        op = self.options
        ds = op.ds()
        if prop.dim() != 4:
            raise RuntimeError(f"Disort.forward: prop must be (nwave, ncol, nlyr, nprop), got "
                               f"{tuple(prop.shape)}")
        nwave, ncol, nlyr, nprop = prop.shape
        if nlyr != ds.nlyr:
            raise RuntimeError(f"Disort.forward: prop has {nlyr} layers, ds().nlyr = {ds.nlyr}")
        for k in bc:
            if k not in _BC_KEYS and k not in _BC_IGNORED:
                raise RuntimeError(f"Disort.forward: unknown boundary condition '{k}'")
        if self.planck and temf is None:
            raise RuntimeError("Disort.forward: planck flag set but temf not given")
        if self.planck and not (nwave == len(op.wave_lower()) == len(op.wave_upper())):
            # the kernels read wave_lower/upper[w] for every w < prop.shape[0]
            raise RuntimeError(f"Disort.forward: planck: prop has {nwave} waves but "
                               f"wave_lower/wave_upper hold {len(op.wave_lower())}/"
                               f"{len(op.wave_upper())}")
        if not torch.cuda.is_available():
            raise RuntimeError("Disort.forward: no HIP device available (pyharp_amd has no "
                               "CPU path)")
        in_dev = prop.device
        dev = in_dev if in_dev.type == "cuda" else torch.device("cuda", int(op.device()))
        return nwave, ncol, nlyr, nprop, in_dev, dev

    def _stage(self, prop, bc, temf, dev):
        """The inputs as contiguous float64 tensors on ``dev`` and the library's view of
        them: (hd_config, hd_inputs, the tensors to keep alive over the call)."""
        op = self.options
        ds = op.ds()
        nwave, ncol, nlyr, nprop = prop.shape
        f64 = torch.float64

        def dev_tensor(x, shape=None):
            if x is None:
                return None
            t = torch.as_tensor(x, dtype=f64)
            if shape is not None:
                t = t.expand(shape) if t.dim() < len(shape) or t.shape != shape else t
            return t.to(dev).contiguous()

        p = dev_tensor(prop)
        keep = [p]
        bct = {}
        for k in _BC_KEYS:
            if k in bc and bc[k] is not None:
                t = dev_tensor(bc[k], (nwave, ncol))
                if tuple(t.shape) != (nwave, ncol):
                    raise RuntimeError(f"Disort.forward: bc['{k}'] must be (nwave, ncol)")
                bct[k] = t
                keep.append(t)
        tf = wl = wu = None
        if self.planck:
            tf = dev_tensor(temf)
            if tuple(tf.shape) != (ncol, nlyr + 1):
                raise RuntimeError(f"Disort.forward: temf must be (ncol, nlyr+1) = "
                                   f"{(ncol, nlyr + 1)}, got {tuple(tf.shape)}")
            # cached per device: no host->device copy per call (keeps forward
            # capturable into a HIP graph once warmed up)
            key = (str(dev), tuple(op.wave_lower()), tuple(op.wave_upper()))
            if self._waves is None or self._waves[0] != key:
                self._waves = (key, torch.tensor(op.wave_lower(), dtype=f64, device=dev),
                               torch.tensor(op.wave_upper(), dtype=f64, device=dev))
            wl, wu = self._waves[1], self._waves[2]
            keep += [tf, wl, wu]

        def ptr(t):
            return t.data_ptr() if t is not None else None

        cfg = _lib.HdConfig(nstr=ds.nstr, nmom=ds.nmom, nlyr=nlyr, nprop=nprop,
                            flags=_lib.HD_FLAG_LAMBER | _lib.HD_FLAG_ONLYFL |
                            (_lib.HD_FLAG_PLANCK if self.planck else 0))
        inp = _lib.HdInputs(nwave=nwave, ncol=ncol, prop=ptr(p),
                            fbeam=ptr(bct.get("fbeam")), umu0=ptr(bct.get("umu0")),
                            albedo=ptr(bct.get("albedo")), btemp=ptr(bct.get("btemp")),
                            ttemp=ptr(bct.get("ttemp")), temis=ptr(bct.get("temis")),
                            fisot=ptr(bct.get("fisot")), temf=ptr(tf), wave_lower=ptr(wl),
                            wave_upper=ptr(wu))
        return cfg, inp, keep

    def _check_sphere(self, prop, zd):
        """The 'spher' flag and ``zd`` come together, on the device; returns the
        hd_sphere of the call or None."""
        if not self.spher:
            if zd is not None:
                raise RuntimeError("Disort.forward: zd given without the 'spher' flag (it would "
                                   "be ignored)")
            return None
        if zd is None:
            raise RuntimeError("Disort.forward: the 'spher' flag needs the level altitudes zd=")
        nlyr = self.options.ds().nlyr
        if not isinstance(zd, torch.Tensor) or zd.dtype != torch.float64:
            raise RuntimeError("Disort.forward: zd must be a float64 tensor")
        if prop.device.type != "cuda" or zd.device != prop.device:
            raise RuntimeError("Disort.forward: 'spher' takes prop and zd on one HIP device "
                               "(there are no host-array pseudo-spherical calls)")
        if prop.dim() == 4 and (zd.dim() not in (1, 2) or zd.shape[-1] != nlyr + 1 or
                                (zd.dim() == 2 and zd.shape[0] != prop.shape[1])):
            raise RuntimeError(f"Disort.forward: zd must be (nlyr+1,) or (ncol, nlyr+1) = "
                               f"({prop.shape[1]}, {nlyr + 1}), got {tuple(zd.shape)}")
        z = zd.contiguous()
        return _lib.HdSphere(radius=float(self.options.radius()), zd=z.data_ptr(),
                             per_column=int(z.dim() == 2)), z

    def _forward(self, prop, bc, temf, *, status=None, out=None, band=None, flx=False, zd=None):
        ds = self.options.ds()
        bc = {} if bc is None else bc
        sph = self._check_sphere(prop, zd)
        nwave, ncol, nlyr, nprop, in_dev, dev = self._check_inputs(prop, bc, temf)
        f64 = torch.float64
        if (in_dev.type != "cuda" and not self.radiance and out is None and status is None
                and not flx):
            # pydisort's CPU-tensor contract: the library's host-array entry points
            # (hd_solve_host / hd_solve_band_host) copy the arrays over in pieces
            # beside the solve of the previous piece
            return self._forward_host(prop, bc, temf, band, dev, nwave, ncol, nlyr, nprop)
        cfg, inp, keep = self._stage(prop, bc, temf, dev)
        if sph is not None:
            sph, zkeep = sph
            keep.append(zkeep)
        nlev = ds.ntau if self.radiance else nlyr + 1
        ncomp = NFLX if flx else 2
        if out is None:
            flux = None if band is not None else \
                torch.empty((nwave, ncol, nlev, ncomp), dtype=f64, device=dev)
        else:
            if (out.device != dev or out.dtype != f64 or not out.is_contiguous()
                    or tuple(out.shape) != (nwave, ncol, nlev, ncomp)):
                who = "Disort.forward_flx" if flx else "Disort.forward"
                raise RuntimeError(f"{who}: out must be a contiguous float64 tensor "
                                   f"of shape {(nwave, ncol, nlev, ncomp)} on {dev}")
            flux = out
        if status is not None and (status.device != dev or status.dtype != torch.int32
                                   or not status.is_contiguous()
                                   or status.numel() < nwave * ncol):
            raise RuntimeError(f"Disort.forward: status must be a contiguous int32 tensor of "
                               f">= {nwave * ncol} elements on {dev}")

        def ptr(t):
            return t.data_ptr() if t is not None else None

        stream = torch.cuda.current_stream(dev)
        if band is not None:
            wts = torch.as_tensor(band[0], dtype=f64).to(dev).reshape(-1).contiguous()
            if wts.numel() != nwave:
                raise RuntimeError(f"Disort.forward_band: {wts.numel()} weights for {nwave} "
                                   "waves")
            bout = band[1]
            if bout is None:
                bout = torch.empty((ncol, nlyr + 1, 2), dtype=f64, device=dev)
            elif (bout.device != dev or bout.dtype != f64 or not bout.is_contiguous()
                  or tuple(bout.shape) != (ncol, nlyr + 1, 2)):
                raise RuntimeError("Disort.forward_band: out must be a contiguous float64 "
                                   f"tensor of shape {(ncol, nlyr + 1, 2)} on {dev}")
            keep.append(wts)
            hb = _lib.HdBand(weight=wts.data_ptr(), bflux=bout.data_ptr())
            with torch.cuda.device(dev):
                if sph is not None:
                    _context(dev.index).solve_spher(
                        cfg, inp, sph, hb, ptr(flux),
                        status.data_ptr() if status is not None else None, stream.cuda_stream)
                else:
                    _context(dev.index).solve_band(
                        cfg, inp, hb, ptr(flux),
                        status.data_ptr() if status is not None else None, stream.cuda_stream)
            del keep
            return bout.to(in_dev) if in_dev.type != "cuda" else bout
        if sph is not None:
            st = status.data_ptr() if status is not None else None
            with torch.cuda.device(dev):
                if flx:
                    _context(dev.index).solve_flx_spher(cfg, inp, sph, flux.data_ptr(), st,
                                                        stream.cuda_stream)
                else:
                    _context(dev.index).solve_spher(cfg, inp, sph, None, flux.data_ptr(), st,
                                                    stream.cuda_stream)
        elif flx:
            with torch.cuda.device(dev):
                _context(dev.index).solve_flx(cfg, inp, flux.data_ptr(),
                                              status.data_ptr() if status is not None else None,
                                              stream.cuda_stream)
        elif self.radiance:
            self._forward_radiance(cfg, inp, flux, status, stream, bc, dev, keep, nwave, ncol)
        else:
            with torch.cuda.device(dev):
                _context(dev.index).solve(cfg, inp, flux.data_ptr(),
                                          status.data_ptr() if status is not None else None,
                                          stream.cuda_stream)
        del keep
        if self._rad is not None and in_dev.type != "cuda":
            self._rad = self._rad.to(in_dev)
        if in_dev.type != "cuda":
            return flux.to(in_dev)
        return flux

    def _forward_host(self, prop, bc, temf, band, dev, nwave, ncol, nlyr, nprop):
        ds = self.options.ds()
        op = self.options
        f64 = torch.float64

        def host(x, shape=None):
            if x is None:
                return None
            t = torch.as_tensor(x, dtype=f64, device="cpu")
            if shape is not None and tuple(t.shape) != shape:
                t = t.expand(shape)
            return t.contiguous()

        keep = [host(prop)]
        bct = {}
        for k in _BC_KEYS:
            if k in bc and bc[k] is not None:
                t = host(bc[k], (nwave, ncol))
                if tuple(t.shape) != (nwave, ncol):
                    raise RuntimeError(f"Disort.forward: bc['{k}'] must be (nwave, ncol)")
                bct[k] = t
                keep.append(t)
        tf = wl = wu = None
        if self.planck:
            tf = host(temf)
            if tuple(tf.shape) != (ncol, nlyr + 1):
                raise RuntimeError(f"Disort.forward: temf must be (ncol, nlyr+1) = "
                                   f"{(ncol, nlyr + 1)}, got {tuple(tf.shape)}")
            wl = torch.tensor(op.wave_lower(), dtype=f64)
            wu = torch.tensor(op.wave_upper(), dtype=f64)
            keep += [tf, wl, wu]

        def ptr(t):
            return t.data_ptr() if t is not None else None

        cfg = _lib.HdConfig(nstr=ds.nstr, nmom=ds.nmom, nlyr=nlyr, nprop=nprop,
                            flags=_lib.HD_FLAG_LAMBER | _lib.HD_FLAG_ONLYFL |
                            (_lib.HD_FLAG_PLANCK if self.planck else 0))
        inp = _lib.HdInputs(nwave=nwave, ncol=ncol, prop=ptr(keep[0]),
                            fbeam=ptr(bct.get("fbeam")), umu0=ptr(bct.get("umu0")),
                            albedo=ptr(bct.get("albedo")), btemp=ptr(bct.get("btemp")),
                            ttemp=ptr(bct.get("ttemp")), temis=ptr(bct.get("temis")),
                            fisot=ptr(bct.get("fisot")), temf=ptr(tf), wave_lower=ptr(wl),
                            wave_upper=ptr(wu))
        ctx = _context(dev.index)
        if band is not None:
            wts = host(band[0]).reshape(-1).contiguous()
            if wts.numel() != nwave:
                raise RuntimeError(f"Disort.forward_band: {wts.numel()} weights for {nwave} "
                                   "waves")
            bout = torch.empty((ncol, nlyr + 1, 2), dtype=f64)
            with torch.cuda.device(dev):
                ctx.solve_band_host(cfg, inp, wts.data_ptr(), bout.data_ptr(), None)
            if band[1] is not None:
                band[1].copy_(bout)
                return band[1]
            return bout
        flux = torch.empty((nwave, ncol, nlyr + 1, 2), dtype=f64)
        with torch.cuda.device(dev):
            ctx.solve_host(cfg, inp, flux.data_ptr())
        return flux

    def _forward_radiance(self, cfg, inp, flux, status, stream, bc, dev, keep, nwave, ncol):
        import ctypes
        ds = self.options.ds()
        f64 = torch.float64
        phi0 = None
        if bc.get("phi0") is not None:
            phi0 = torch.as_tensor(bc["phi0"], dtype=f64).expand((nwave, ncol)).to(dev)
            phi0 = phi0.contiguous()
            keep.append(phi0)
        arr = lambda xs: (ctypes.c_double * max(1, len(xs)))(*xs)  # noqa: E731
        ut, mu, ph = arr(ds.utau), arr(self._umu), arr(self._phi)
        rad = _lib.HdRadiance(ntau=len(ds.utau) if self.usrtau else 0,
                              utau=ctypes.cast(ut, ctypes.c_void_p),
                              numu=len(self._umu), umu=ctypes.cast(mu, ctypes.c_void_p),
                              nphi=len(self._phi), phi=ctypes.cast(ph, ctypes.c_void_p),
                              phi0=phi0.data_ptr() if phi0 is not None else None,
                              onlyfl=int(self.onlyfl), corint=int(self.corint))
        uu = None
        if not self.onlyfl:
            uu = torch.empty((nwave, ncol, len(self._phi), ds.ntau, len(self._umu)), dtype=f64,
                             device=dev)
        with torch.cuda.device(dev):
            _context(dev.index).solve_radiance(
                cfg, inp, rad, flux.data_ptr(), uu.data_ptr() if uu is not None else None,
                status.data_ptr() if status is not None else None, stream.cuda_stream)
        self._rad = uu


def _lib_loaded() -> bool:
    try:
        _lib.load()
        return True
    except OSError:
        return False


def _gauss(nstr):
    import numpy as np
    x, w = np.polynomial.legendre.leggauss(nstr // 2)
    return list(0.5 * (x + 1.0)), list(0.5 * w)
