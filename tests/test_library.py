"""The C-ABI library and the host-side module, without a GPU.

Checks that libhdisort.so builds/loads and exports every symbol declared in
include/hdisort.h, the host helpers, option validation and the loud failure
when no HIP device is present (no CPU fallback).
"""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_functions(header="hdisort.h"):
    with open(os.path.join(ROOT, "include", header)) as f:
        src = f.read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(hd_[a-z_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    from pyharp_amd import _build, _lib
    _build.build()
    return _lib.load()


def test_exports_every_declared_symbol(lib):
    from pyharp_amd import _lib
    names = _declared_functions()
    assert "hd_solve" in names and len(names) >= 10
    for name in names:
        assert hasattr(lib, name), name
    assert set(names) == set(_lib.EXPORTED)


def test_exports_every_harp_symbol(lib):
    from pyharp_amd import _lib
    names = _declared_functions("hdharp.h")
    assert set(names) == set(_lib.HARP_EXPORTED)
    for name in names:
        assert hasattr(lib, name), name


def test_exports_every_netcdf_symbol(lib):
    from pyharp_amd import _lib
    names = _declared_functions("hdnc.h")
    assert set(names) == set(_lib.NC_EXPORTED)
    for name in names:
        assert hasattr(lib, name), name


def test_harp_ops_refuse_cpu_tensors():
    from pyharp_amd.spectral import band_flux, heating_rate
    with pytest.raises(RuntimeError, match="device"):
        band_flux(torch.zeros((2, 1, 3, 2), dtype=torch.float64), torch.ones(2))
    with pytest.raises(RuntimeError, match="device"):
        heating_rate(torch.zeros((1, 3, 2), dtype=torch.float64), torch.ones(2), torch.ones(2), 1.0)


def test_version(lib):
    assert lib.hd_version() == 100


@pytest.mark.parametrize("nstr", [2, 4, 8, 16])
def test_quadrature_matches_gauss_legendre(nstr):
    from pyharp_amd import _lib
    mu, w = _lib.quadrature(nstr)
    x, wx = np.polynomial.legendre.leggauss(nstr // 2)
    np.testing.assert_allclose(mu, 0.5 * (x + 1), rtol=0, atol=1e-15)
    np.testing.assert_allclose(w, 0.5 * wx, rtol=0, atol=1e-15)


def test_quadrature_rejects_odd(lib):
    mu = (ctypes.c_double * 4)()
    assert lib.hd_quadrature(5, mu, mu) == 1


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_no_device_fails_loudly(lib):
    h = ctypes.c_void_p()
    rc = lib.hd_context_create(ctypes.byref(h), 0)
    assert rc != 0
    from pyharp_amd import Disort, DisortOptions
    op = DisortOptions().flags("lamber,onlyfl").nwave(1).ncol(1)
    op.ds().nlyr, op.ds().nstr, op.ds().nmom = 2, 4, 4
    with pytest.raises(RuntimeError, match="no HIP device"):
        Disort(op).forward(torch.zeros((1, 1, 2, 6), dtype=torch.float64), {})


def test_null_context_rejected(lib):
    from pyharp_amd import _lib
    cfg = _lib.HdConfig(nstr=4, nmom=4, nlyr=2, nprop=6, flags=1)
    inp = _lib.HdInputs(nwave=1, ncol=1)
    assert lib.hd_solve(None, ctypes.byref(cfg), ctypes.byref(inp), None, None, None) == 1


def test_options_validation():
    from pyharp_amd import Disort, DisortOptions
    op = DisortOptions().flags("lamber,onlyfl,bogus")
    with pytest.raises(RuntimeError, match="unknown flags"):
        Disort(op)
    op = DisortOptions().flags("lamber")
    op.ds().nstr = 5
    with pytest.raises(RuntimeError, match="nstr"):
        Disort(op)
    op = DisortOptions().flags("onlyfl")
    with pytest.raises(RuntimeError, match="Lambertian"):
        Disort(op)
    op = DisortOptions().flags("lamber,planck").nwave(2)
    with pytest.raises(RuntimeError, match="wave_lower"):
        Disort(op)


# (flag string, expected error pattern or None): the boundary's flag semantics
# (cdisort's flag names, examples/amarsw-ck.yaml:74-90)
_FLAG_CASES = [
    ("lamber,quiet,onlyfl", None),
    ("lamber,quiet,onlyfl,intensity_correction,old_intensity_correction", None),
    # the BASELINE configs' yaml (amarsw-ck.yaml:79-82): new correction + onlyfl --
    # cdisort corrects radiances only, so the flux path is unaffected
    ("lamber,quiet,onlyfl,intensity_correction", None),
    ("lamber,intensity_correction,old_intensity_correction", None),
    ("lamber,old_intensity_correction", None),
    ("lamber,intensity_correction", "Buras-Emde-Dowling"),
    ("lamber,onlyfl,ibcnd", "ibcnd"),
    ("lamber,ibcnd", "ibcnd"),
    ("lamber,onlyfl,spher", "pseudo-spherical"),
    ("lamber,onlyfl,general_source", "general"),
    ("lamber,onlyfl,output_uum", "uum"),
    ("lamber,onlyfl,deltam", "unknown"),
    ("lamber,onlyfl,lyrcut", "unknown"),
]


@pytest.mark.parametrize("flags,err", _FLAG_CASES)
def test_flag_semantics(flags, err):
    """ibcnd is refused as harp's DISORT driver refuses it (rt_solver_disort.cpp_:67-68);
    spher / general_source / output_uum and cdisort's new intensity correction are not
    implemented and refused; names cdisort does not have (deltam, lyrcut) are unknown."""
    from pyharp_amd import Disort, DisortOptions
    op = DisortOptions().flags(flags).nwave(1).ncol(1)
    op.ds().nlyr, op.ds().nstr, op.ds().nmom = 4, 8, 8
    if err is None:
        Disort(op)
    else:
        with pytest.raises(RuntimeError, match=err):
            Disort(op)


def test_correction_flags_select_nakajima_tanaka_only_with_both():
    from pyharp_amd import Disort, DisortOptions

    def corint(flags):
        op = DisortOptions().flags(flags).nwave(1).ncol(1)
        op.ds().nlyr, op.ds().nstr, op.ds().nmom = 4, 8, 8
        return Disort(op).corint

    assert corint("lamber,intensity_correction,old_intensity_correction")
    assert not corint("lamber,old_intensity_correction")  # cdisort: no correction
    assert not corint("lamber")


def test_cpp_flag_semantics():
    """The C++ drop-in (include/harp_amd/disort.hpp) accepts and refuses exactly the
    flag strings the Python binding does (tests/cpp/flags_check.cpp, no GPU needed)."""
    import subprocess
    exe = os.path.join(os.path.dirname(__file__), "cpp", "flags_check")
    src = exe + ".cpp"
    hdr = os.path.join(os.path.dirname(__file__), "..", "include", "harp_amd", "disort.hpp")
    lib = os.path.join(os.path.dirname(__file__), "..", "pyharp_amd", "libhdisort.so")
    if not os.path.exists(lib):
        pytest.skip("libhdisort.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    if not os.path.exists(exe) and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc to build tests/cpp/flags_check")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src),
                                                              os.path.getmtime(hdr)):
        torch_dir = os.path.dirname(torch.__file__)
        root = os.path.join(os.path.dirname(__file__), "..")
        abi = int(torch._C._GLIBCXX_USE_CXX11_ABI)
        subprocess.run(
            ["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", f"-D_GLIBCXX_USE_CXX11_ABI={abi}",
             "-D__HIP_PLATFORM_AMD__", "-DUSE_ROCM", f"-I{root}/include",
             f"-I{torch_dir}/include", f"-I{torch_dir}/include/torch/csrc/api/include", src,
             "-o", exe, f"-L{torch_dir}/lib", f"-Wl,-rpath,{torch_dir}/lib", "-ltorch",
             "-ltorch_cpu", "-lc10", "-ltorch_hip", "-lc10_hip", f"-L{root}/pyharp_amd",
             "-Wl,-rpath,$ORIGIN/../../pyharp_amd", "-lhdisort", "-lz"],
            check=True, capture_output=True)
    out = subprocess.run([exe] + [f for f, _ in _FLAG_CASES], check=True, capture_output=True,
                         text=True).stdout.strip().split("\n")
    assert len(out) == len(_FLAG_CASES)
    for line, (flags, err) in zip(out, _FLAG_CASES):
        if err is None:
            assert line == f"OK {flags}", line
        else:
            assert line.startswith(f"REJECT {flags}:") and re.search(err, line), line


def test_option_accessors_follow_add_arg_idiom():
    from pyharp_amd import DisortOptions
    op = DisortOptions()
    assert op.nwave(7) is op and op.nwave() == 7
    op.ds().nlyr = 40
    assert op.ds().nlyr == 40


def test_rtsolver_base_raises():
    from pyharp_amd import RTSolver
    with pytest.raises(RuntimeError, match="not implemented"):
        RTSolver().forward(None, {})


def test_forward_shape_errors():
    from pyharp_amd import Disort, DisortOptions
    op = DisortOptions().flags("lamber,onlyfl").nwave(1).ncol(1)
    op.ds().nlyr, op.ds().nstr = 3, 4
    d = Disort(op)
    with pytest.raises(RuntimeError, match="layers"):
        d.forward(torch.zeros((1, 1, 2, 6), dtype=torch.float64), {})
    with pytest.raises(RuntimeError, match="unknown boundary"):
        d.forward(torch.zeros((1, 1, 3, 6), dtype=torch.float64), {"fbam": torch.ones(1, 1)})


def test_planck_wave_count_must_match_prop():
    """With planck the kernels read wave_lower/upper[w] for every w < prop.shape[0]:
    a prop with more (or fewer) waves than the options' bounds is refused."""
    from pyharp_amd import Disort, DisortOptions
    op = DisortOptions().flags("lamber,onlyfl,planck").nwave(2).ncol(1)
    op.wave_lower([1.0, 2.0]).wave_upper([2.0, 3.0])
    op.ds().nlyr, op.ds().nstr = 3, 4
    d = Disort(op)
    temf = torch.full((1, 4), 250.0, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="waves"):
        d.forward(torch.zeros((3, 1, 3, 6), dtype=torch.float64), {}, temf)
    with pytest.raises(RuntimeError, match="waves"):
        d.forward(torch.zeros((1, 1, 3, 6), dtype=torch.float64), {}, temf)


def test_layer2level_torch_matches_reference_run():
    from pyharp_amd import layer2level
    out = layer2level(torch.tensor([[300.0, 280.0, 260.0, 250.0, 240.0]], dtype=torch.float64))
    np.testing.assert_allclose(out[0].numpy(),
                               [310.0, 290.0, 269.1666666667, 254.1666666667, 245.0, 240.0],
                               rtol=1e-10)


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "pyharp_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".cpp", ".hip", ".hpp", ".h")):
                with open(os.path.join(dirpath, fn)) as f:
                    src = f.read()
                assert not re.search(r"^\s*(from|import)\s+oracle", src, re.M), fn
                assert "hdoracle" not in src, fn
                assert not re.search(r"^\s*(from|import)\s+mpmath", src, re.M), fn


def test_scattering_moments():
    from pyharp_amd import PhaseMomentOptions, scattering_moments
    from pyharp_amd.scattering import kHenyeyGreenstein, kIsotropic, kRayleigh
    assert scattering_moments(16, PhaseMomentOptions().type(kIsotropic)).abs().sum() == 0
    r = scattering_moments(8, PhaseMomentOptions().type(kRayleigh))
    assert r[1] == 0.1 and r.abs().sum() == 0.1
    h = scattering_moments(4, PhaseMomentOptions().type(kHenyeyGreenstein).gg(0.5))
    assert torch.allclose(h, torch.tensor([0.5, 0.25, 0.125, 0.0625], dtype=torch.float64))


def test_night_side_beam():
    """pyharp_amd.night_side_beam: 'dark' switches the beam off where umu0 <= 0,
    'clamp' floors umu0 at 1e-3 where fbeam > 0 (harp's legacy convention); the
    caller's tensors are left alone and umu0 > 1 is not hidden."""
    from pyharp_amd import night_side_beam
    fb = torch.ones(2, 3)
    mu = torch.tensor([[0.5, -0.1, 0.0], [1.0, 0.2, 1.5]])
    d = night_side_beam({"fbeam": fb, "umu0": mu, "albedo": 0.3 * fb}, "dark")
    assert torch.equal(d["fbeam"], torch.tensor([[1.0, 0.0, 0.0], [1.0, 1.0, 1.0]]))
    assert d["umu0"] is mu and torch.equal(fb, torch.ones(2, 3))
    c = night_side_beam({"fbeam": torch.tensor([[1.0, 1.0, 0.0], [1.0, 1.0, 1.0]]), "umu0": mu},
                        "clamp")
    assert torch.equal(c["umu0"], torch.tensor([[0.5, 1e-3, 0.0], [1.0, 0.2, 1.5]]))
    assert night_side_beam({"albedo": fb}) == {"albedo": fb}
    with pytest.raises(ValueError):
        night_side_beam({"fbeam": fb, "umu0": mu}, "floor")


def test_chunk_plan(lib):
    """The automatic chunking (hd_chunk_solves; no device needed).  Register path
    (nstr <= 16): chunks of ~32 768 solves (~40 960 when that gives fewer than five), so
    that the next chunk's layer kernel keeps 40-50 % of the SIMDs while a chunk's sweep
    runs -- C4 640 000 solves in 20 chunks, the 8-GPU rank shape 80 000 in 2
    (profiles/r05/chunk_sweep.txt).  Team path (nstr 18..32): a 16 GB
    scratch budget bounds the chunk (C5 64 000 solves: 4 chunks of 16 000); the 8-GPU
    C5 rank shape (8 g-points x 1 000 columns) stays one chunk -- split in two it ran
    9 % slower (profiles/r05/c5_rank_shape.txt)."""
    from pyharp_amd import _lib
    assert _lib.chunk_solves(16, 80, 640000) == 32000
    assert _lib.chunk_solves(16, 80, 160000) == 32000
    assert _lib.chunk_solves(16, 80, 65536) == 32768
    assert _lib.chunk_solves(16, 80, 80000) == 40000
    assert _lib.chunk_solves(16, 80, 16) == 16
    assert _lib.chunk_solves(32, 80, 64000) == 16000
    assert _lib.chunk_solves(32, 80, 8000) == 8000
    assert _lib.chunk_solves(32, 80, 16384) == 16384
    assert _lib.chunk_solves(32, 80, 16385) == 8193
    with pytest.raises(RuntimeError):
        _lib.chunk_solves(15, 80, 100)
